"""CPU suite of scaled decode (hgi_decode_scaled_u8_dev / hgi_decode_scaled_u8): the library exports both entry points, the
ctypes table matches their declarations, the C ABI and the Python mirror refuse bad arguments before they touch a device, the new
translation unit compiles for gfx950 with no scratch and no spills, and the identity the feature rests on holds on the oracle:
decode(grid, levels)[::2^s, ::2^s] == decode(grid[::2^s, ::2^s], max(levels - s, 0))."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEED0
from rustyhgi_amd import _ffi

sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("hgi_decode_scaled_u8_dev", "hgi_decode_scaled_u8")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgi.h")).read(), flags=re.S)
    m = re.search(r"HGI_API\s+hgi_status\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_both_scaled_entry_points():
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
            t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
            assert t in ctype_of, (n, a)
            want.append(ctype_of[t])
        _, res, got = table[n]
        assert res is _ffi._int and got == want, (n, args)
    assert len(_declaration("hgi_decode_scaled_u8_dev")) == 12 and len(_declaration("hgi_decode_scaled_u8")) == 9


def test_c_abi_refuses_bad_arguments_without_a_device():
    """What the C entry points decide before touching a device: a NULL ctx, a shift beyond 31, an unknown interpolator.  The
    last two are tested before the ctx is used for anything, so a zeroed stand-in serves as one here."""
    L = _ffi.lib()
    g = np.zeros(64, np.uint8)
    o = np.zeros(64, np.uint8)
    assert L.hgi_decode_scaled_u8(None, g.ctypes.data, 8, 8, 2, 1, 1, o.ctypes.data, 4) == _ffi.EINVAL
    assert L.hgi_decode_scaled_u8_dev(None, g.ctypes.data, 8, 8, 2, 1, 1, o.ctypes.data, 4, 1, 64, 16) == _ffi.EINVAL
    stand_in = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(stand_in)
    assert L.hgi_decode_scaled_u8(ctx, g.ctypes.data, 8, 8, 2, 1, 32, o.ctypes.data, 1) == _ffi.EINVAL
    assert L.hgi_decode_scaled_u8_dev(ctx, g.ctypes.data, 8, 8, 2, 1, 32, o.ctypes.data, 1, 1, 64, 1) == _ffi.EINVAL
    assert L.hgi_decode_scaled_u8(ctx, g.ctypes.data, 8, 8, 2, 7, 1, o.ctypes.data, 4) == _ffi.EUNSUPPORTED
    assert L.hgi_decode_scaled_u8_dev(ctx, g.ctypes.data, 8, 8, 2, 7, 1, o.ctypes.data, 4, 1, 64, 16) == _ffi.EUNSUPPORTED
    assert L.hgi_decode_scaled_u8(ctx, g.ctypes.data, 8, 8, 32, 1, 1, o.ctypes.data, 4) == _ffi.EINVAL       # levels


def _decoder():
    from rustyhgi_amd import Decoder
    from rustyhgi_amd.interpolator import Crossed
    return Decoder(Crossed())        # constructing one touches no device


@pytest.mark.parametrize("shift", [-1, 32, 1.5, "2", None, True, 2 ** 40])
def test_python_mirror_refuses_bad_shifts_before_any_device_call(shift):
    dec = _decoder()
    grid = np.zeros((64, 128), np.uint8)
    with pytest.raises(ValueError, match="shift"):
        dec.decode_scaled((128, 64), 4, grid, shift)
    with pytest.raises(ValueError, match="shift"):
        dec.decode_scaled_batch(np.zeros((2, 64, 128), np.uint8), 4, shift)


def test_python_mirror_refuses_bad_out_before_any_device_call():
    dec = _decoder()
    grids = np.zeros((3, 64, 129), np.uint8)      # shift 2: 33 x 16
    bad = [np.zeros((3, 33, 16), np.uint8),                        # (w, h) swapped
           np.zeros((2, 16, 33), np.uint8),                        # batch
           np.zeros((3, 16, 32), np.uint8),                        # floor instead of ceil
           np.zeros((3, 16, 33), np.int16),                        # dtype
           np.zeros((3, 33, 16), np.uint8).transpose(0, 2, 1),     # right shape, not C-contiguous
           np.zeros((3, 16, 66), np.uint8)[:, :, ::2]]             # strided view
    ro = np.zeros((3, 16, 33), np.uint8)
    ro.setflags(write=False)
    bad.append(ro)                                                 # read-only
    for out in bad:
        with pytest.raises(ValueError, match="out"):
            dec.decode_scaled_batch(grids, 4, 2, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        dec.decode_scaled_batch(grids, 4, 0, out=grids)
    with pytest.raises(ValueError, match="overlaps"):
        dec.decode_scaled_batch(grids, 4, 2, out=grids.reshape(-1)[:3 * 16 * 33].reshape(3, 16, 33))
    torch = pytest.importorskip("torch")
    tg = torch.zeros((3, 64, 129), dtype=torch.uint8)
    for out in (torch.zeros((3, 16, 33), dtype=torch.int32), torch.zeros((3, 33, 16), dtype=torch.uint8),
                torch.zeros((3, 33, 16), dtype=torch.uint8).transpose(1, 2), np.zeros((3, 16, 33), np.uint8)):
        with pytest.raises(ValueError, match="out"):
            dec.decode_scaled_batch(tg, 4, 2, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        dec.decode_scaled_batch(tg, 4, 2, out=tg.reshape(-1)[:3 * 16 * 33].reshape(3, 16, 33))
    # a valid `out` passes the checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        dec.decode_scaled_batch(tg, 4, 2, out=torch.zeros((3, 16, 33), dtype=torch.uint8))


def test_scaled_size_is_the_ceiling_in_any_width():
    from rustyhgi_amd.codec import scaled_size
    assert scaled_size(1, 1, 31) == (1, 1)
    assert scaled_size(2 ** 32 - 1, 5, 31) == (2, 1)
    assert scaled_size(129, 64, 2) == (33, 16)
    assert scaled_size(1920, 1080, 0) == (1920, 1080)


def _isa(tmp_path, tu):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / (tu + ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "rustyhgi_amd", "csrc", tu), "-o", out], stderr=subprocess.DEVNULL)
    return out


@pytest.mark.timeout(900)
def test_scaled_unit_is_the_sdwa_build_without_scratch(tmp_path):
    """k_dec_scaled<interp, unseeded | cone, load form>: twelve tile kernels plus the lattice gather, the SDWA finest level really
    there, and the hazard rules of tools/check_isa.py (no scratch, no spills, no DPP next to SDWA asm, wide-store data held two
    wait states)."""
    import check_isa
    r = check_isa.check(_isa(tmp_path, "hgi_fused_scaled.hip"))
    assert r["kernels"] == 13, r
    assert r["partial_writes"] > 100, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(str(tmp_path / "hgi_fused_scaled.hip.s")).read()
    assert len(set(re.findall(r"\b(_Z\w*k_dec_scaled\w*):", text))) == 12
    assert "k_dec_tiles" not in text and "k_dec_region" not in text      # the other decoders' kernels stay in their own units


def test_scaled_unit_is_in_the_library_build():
    mk = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/hgi_fused_scaled.o" in mk


def test_lattice_identity_on_the_oracle():
    """decode(grid, L)[::S, ::S] == decode(grid[::S, ::S], max(L - s, 0)), S = 2^s: random shapes from 1 x 1 up, levels 0 .. 12,
    both interpolators, every s from 0 to L + 2, random grids (any byte is a valid grid)."""
    from oracle import hgi_numpy as N
    rng = np.random.default_rng(SEED0 + 70)
    shapes = [(1, 1), (1, 9), (9, 1), (2, 3), (128, 64), (129, 65), (255, 257), (299, 199)]
    shapes += [(int(rng.integers(1, 300)), int(rng.integers(1, 200))) for _ in range(10)]
    n = 0
    for i, (w, h) in enumerate(shapes):
        grid = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for interp in (N.LEFTTOP, N.CROSSED):
            for levels in sorted({i % 4, 4 + i % 5, 12 if i % 3 == 0 else 9}):
                full = N.decode(grid, levels, interp)
                for s in range(levels + 3):
                    S = 1 << s
                    want = full[::S, ::S]
                    got = N.decode(grid[::S, ::S], max(levels - s, 0), interp)
                    assert got.shape == want.shape and (got == want).all(), (w, h, levels, interp, s)
                    n += 1
    assert n > 500
