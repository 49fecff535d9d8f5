"""CPU suite of region decode (hgi_decode_region_u8_dev / hgi_decode_region_u8): the library exports both entry points, the
ctypes table matches their declarations, the Python mirror refuses bad windows and bad `out=` buffers before it touches a
device, and the new translation unit compiles for gfx950 to the SDWA tile kernels with no scratch and no spills."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rustyhgi_amd import _ffi

sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("hgi_decode_region_u8_dev", "hgi_decode_region_u8")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgi.h")).read(), flags=re.S)
    m = re.search(r"HGI_API\s+hgi_status\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_both_region_entry_points():
    L = ctypes.CDLL(_ffi.LIB_PATH)
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in table, n
        assert hasattr(_ffi.lib(), n)


def test_ctypes_table_matches_the_header():
    ctype_of = {"hgi_ctx *": _ffi._vp, "const void *": _ffi._vp, "void *": _ffi._vp, "const uint8_t *": _ffi._vp,
                "uint8_t *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz, "hgi_interp": _ffi._int}
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        args = _declaration(n)
        want = []
        for a in args:
            t = re.match(r"(.*?)\s*\w+$", a).group(1).replace(" *", " *").strip()
            t = re.sub(r"\s*\*\s*", " *", t)
            assert t in ctype_of, (n, a)
            want.append(ctype_of[t])
        _, res, got = table[n]
        assert res is _ffi._int and got == want, (n, args)
    assert len(_declaration("hgi_decode_region_u8_dev")) == 15 and len(_declaration("hgi_decode_region_u8")) == 12


def _decoder():
    from rustyhgi_amd import Decoder
    from rustyhgi_amd.interpolator import Crossed
    return Decoder(Crossed())        # constructing one touches no device


@pytest.mark.parametrize("rect", [(2 ** 32 - 1, 0, 1, 1), (0, 2 ** 32 - 1, 1, 1), (0, 0, 2 ** 32, 1), (120, 0, 9, 1), (0, 60, 1, 5),
                                  (128, 0, 1, 1), (0, 64, 1, 1), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1), (0, 0, 1, -2)])
def test_python_mirror_refuses_bad_windows_before_any_device_call(rect):
    """A 128 x 64 frame: every window here is outside it or has a negative coordinate or size.  The refusal is a ValueError raised
    before a context exists (on a machine without a GPU, reaching the library would raise HgiError EDEVICE instead)."""
    dec = _decoder()
    grid = np.zeros((64, 128), np.uint8)
    with pytest.raises(ValueError, match="region"):
        dec.decode_region((128, 64), 4, grid, rect)
    with pytest.raises(ValueError, match="region"):
        dec.decode_region_batch(np.zeros((2, 64, 128), np.uint8), 4, rect)
    with pytest.raises(ValueError):
        dec.decode_region((128, 64), 4, grid, (0, 0, 1))           # not four numbers


def test_python_mirror_refuses_bad_out_before_any_device_call():
    dec = _decoder()
    grids = np.zeros((3, 64, 128), np.uint8)
    rect = (5, 7, 20, 10)
    bad = [np.zeros((3, 20, 10), np.uint8),                        # (w, h) swapped
           np.zeros((2, 10, 20), np.uint8),                        # batch
           np.zeros((3, 10, 20), np.int16),                        # dtype
           np.zeros((3, 20, 10), np.uint8).transpose(0, 2, 1),     # right shape, not C-contiguous
           np.zeros((3, 10, 40), np.uint8)[:, :, ::2]]             # strided view
    for out in bad:
        with pytest.raises(ValueError, match="out"):
            dec.decode_region_batch(grids, 4, rect, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        dec.decode_region_batch(grids, 4, (0, 0, 128, 64), out=grids)
    torch = pytest.importorskip("torch")
    tg = torch.zeros((3, 64, 128), dtype=torch.uint8)
    for out in (torch.zeros((3, 10, 20), dtype=torch.int32), torch.zeros((3, 20, 10), dtype=torch.uint8),
                torch.zeros((3, 20, 10), dtype=torch.uint8).transpose(1, 2), np.zeros((3, 10, 20), np.uint8)):
        with pytest.raises(ValueError, match="out"):
            dec.decode_region_batch(tg, 4, rect, out=out)
    # a valid `out` passes the checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        dec.decode_region_batch(tg, 4, rect, out=torch.zeros((3, 10, 20), dtype=torch.uint8))


def test_c_abi_refuses_a_null_ctx_and_bad_arguments_without_a_device():
    """What the C entry points decide before touching a device: a NULL ctx, levels beyond 31, an unknown interpolator."""
    L = _ffi.lib()
    g = np.zeros(64, np.uint8)
    o = np.zeros(64, np.uint8)
    assert L.hgi_decode_region_u8(None, g.ctypes.data, 8, 8, 2, 1, 0, 0, 2, 2, o.ctypes.data, 2) == _ffi.EINVAL
    assert L.hgi_decode_region_u8_dev(None, g.ctypes.data, 8, 8, 2, 1, 0, 0, 2, 2, o.ctypes.data, 2, 1, 64, 4) == _ffi.EINVAL


def _isa(tmp_path, tu):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / (tu + ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "rustyhgi_amd", "csrc", tu), "-o", out], stderr=subprocess.DEVNULL)
    return out


@pytest.mark.timeout(900)
def test_region_unit_is_the_sdwa_build_without_scratch(tmp_path):
    """k_dec_region<interp, unseeded | cone>: four kernels, the SDWA finest level really there, and the hazard rules of
    tools/check_isa.py (no scratch, no spills, no DPP next to SDWA asm, wide-store data held two wait states)."""
    import check_isa
    r = check_isa.check(_isa(tmp_path, "hgi_fused_region.hip"))
    assert r["kernels"] == 4, r
    assert r["partial_writes"] > 100, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(str(tmp_path / "hgi_fused_region.hip.s")).read()
    assert len(set(re.findall(r"\b(_Z\w*k_dec_region\w*):", text))) == 4
    assert "k_dec_tiles" not in text          # the full decode's kernels stay in their own unit


def test_region_unit_is_in_the_library_build():
    mk = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/hgi_fused_region.o" in mk
