"""CPU suite of frame lists (hgi_encode_u8_list_dev / hgi_decode_u8_list_dev): the library exports both entry points, the ctypes
table matches their declarations, the C ABI and the Python mirror refuse bad lists and bad `out=` before they touch a device, the
two new translation units compile for gfx950 to the SDWA tile kernels with no scratch, and the host plan and block -> tile map
(csrc/hgi_framelist.h) pass their randomized test under ASan + UBSan."""
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

NAMES = ("hgi_encode_u8_list_dev", "hgi_decode_u8_list_dev")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgi.h")).read(), flags=re.S)
    m = re.search(r"HGI_API\s+hgi_status\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_both_list_entry_points():
    L = ctypes.CDLL(_ffi.LIB_PATH)
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in table, n
        assert hasattr(_ffi.lib(), n)


def test_ctypes_table_matches_the_header():
    ctype_of = {"hgi_ctx *": _ffi._vp, "const void *const *": _ffi._vp, "void *const *": _ffi._vp, "const uint32_t *": _ffi._vp,
                "const uint8_t": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz, "hgi_interp": _ffi._int}
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        want = []
        for a in _declaration(n):
            a = re.sub(r"\[\d+\]$", "", a)                      # const uint8_t lut[256]: a pointer
            t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
            t = t.replace("* *", "**").replace(" *const *", " *const *")
            assert t in ctype_of, (n, a, t)
            want.append(ctype_of[t])
        _, res, got = table[n]
        assert res is _ffi._int and got == want, (n, got, want)
    assert len(_declaration("hgi_encode_u8_list_dev")) == 9 and len(_declaration("hgi_decode_u8_list_dev")) == 8


def test_c_abi_refuses_a_null_ctx_without_a_device():
    """A NULL ctx is refused first, whatever the arrays hold: nothing here needs a device."""
    L = _ffi.lib()
    ptrs = (ctypes.c_void_p * 2)(None, None)
    dims = (ctypes.c_uint32 * 2)(8, 8)
    lut = np.arange(256, dtype=np.uint8)
    assert L.hgi_encode_u8_list_dev(None, ptrs, dims, dims, 4, 1, lut.ctypes.data, ptrs, 2) == _ffi.EINVAL
    assert b"ctx" in L.hgi_last_error()
    assert L.hgi_decode_u8_list_dev(None, ptrs, dims, dims, 4, 1, ptrs, 2) == _ffi.EINVAL
    assert L.hgi_decode_u8_list_dev(None, None, None, None, 4, 1, None, 0) == _ffi.EINVAL
    assert L.hgi_decode_u8_list_dev(None, None, None, None, 40, 9, None, 3) == _ffi.EINVAL


def _codec():
    from rustyhgi_amd import Decoder, Encoder
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    # constructing them touches no device
    return Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4), Decoder(Crossed())


def test_python_mirror_refuses_bad_lists_before_any_device_call():
    """Every refusal is a ValueError raised before a context exists (on a machine without a GPU, reaching the library would raise
    HgiError EDEVICE instead)."""
    enc, dec = _codec()
    good = [np.zeros((4, 5), np.uint8), np.zeros((7, 3), np.uint8)]
    bad_lists = [np.zeros((2, 4, 5), np.uint8),                          # a stack, not a list
                 [np.zeros((2, 4, 5), np.uint8)],                        # a 3-D frame
                 [np.zeros(5, np.uint8)],                                # a 1-D frame
                 [np.zeros((4, 5), np.int16)],                           # dtype
                 [np.zeros((4, 5), np.uint8), [[1, 2]]],                 # not an array
                 "frames"]
    for frames in bad_lists:
        with pytest.raises(ValueError):
            enc.encode_list(frames)
        with pytest.raises(ValueError):
            dec.decode_list(frames, 4)
    bad_outs = [[np.zeros((4, 5), np.uint8)],                            # length
                [np.zeros((5, 4), np.uint8), np.zeros((7, 3), np.uint8)],            # shape
                [np.zeros((4, 5), np.int32), np.zeros((7, 3), np.uint8)],            # dtype
                [np.zeros((5, 4), np.uint8).T, np.zeros((7, 3), np.uint8)],          # not C-contiguous
                [np.zeros((4, 10), np.uint8)[:, ::2], np.zeros((7, 3), np.uint8)],   # strided view
                np.zeros((2, 4, 5), np.uint8)]                           # not a list
    for out in bad_outs:
        with pytest.raises(ValueError, match="out"):
            enc.encode_list(good, out=out)
        with pytest.raises(ValueError, match="out"):
            dec.decode_list(good, 4, out=out)
    shared = np.zeros(64, np.uint8)
    with pytest.raises(ValueError, match="overlap"):            # two outputs in one buffer
        dec.decode_list(good[:1] * 2, 4, out=[shared[:20].reshape(4, 5), shared[10:30].reshape(4, 5)])
    with pytest.raises(ValueError, match="overlap"):            # an output on an input
        dec.decode_list(good, 4, out=[good[0], np.zeros((7, 3), np.uint8)])
    torch = pytest.importorskip("torch")
    tl = [torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((7, 3), dtype=torch.uint8)]
    for frames in ([tl[0], good[1]],                                      # mixed
                   [torch.zeros((4, 5), dtype=torch.int32)],              # dtype
                   [torch.zeros((2, 4, 5), dtype=torch.uint8)],           # rank
                   [torch.zeros((5, 4), dtype=torch.uint8).t()]):         # not contiguous
        with pytest.raises(ValueError):
            enc.encode_list(frames)
    with pytest.raises(ValueError, match="out"):
        dec.decode_list(tl, 4, out=[torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((3, 7), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="out"):
        dec.decode_list(tl, 4, out=[np.zeros((4, 5), np.uint8), np.zeros((7, 3), np.uint8)])
    # a valid list passes the checks and only then meets the CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        dec.decode_list(tl, 4)
    assert enc.encode_list([]) == [] and dec.decode_list([], 4) == []


def test_python_overlap_rule_matches_brute_force():
    from rustyhgi_amd.codec import _spans_meet
    rng = np.random.default_rng(5)
    for _ in range(3000):
        n = int(rng.integers(1, 12))
        spans = []
        for _ in range(n):
            lo = int(rng.integers(0, 400))
            spans.append((lo, lo + int(rng.integers(0, 60)), bool(rng.integers(0, 2))))
        want = any(a[1] > a[0] and b[1] > b[0] and a[0] < b[1] and b[0] < a[1] and (a[2] or b[2])
                   for i, a in enumerate(spans) for b in spans[i + 1:])
        assert _spans_meet(spans) == want, spans


def _isa(tmp_path, tu):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / (tu + ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "rustyhgi_amd", "csrc", tu), "-o", out], stderr=subprocess.DEVNULL)
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tu,name,kernels,sdwa", [("hgi_fused_list_dec.hip", "k_dec_list", 4, 100),
                                                  ("hgi_fused_list_enc.hip", "k_enc_list", 8, 400)])
def test_list_units_are_the_sdwa_builds_without_scratch(tmp_path, tu, name, kernels, sdwa):
    """k_dec_list<interp, unseeded | cone> and k_enc_list<interp, ident, unseeded | cone>: the SDWA paths really there, the hazard
    rules of tools/check_isa.py, no scratch, no spills, no traps; the table is read with scalar loads."""
    import check_isa
    path = _isa(tmp_path, tu)
    r = check_isa.check(path)
    assert r["kernels"] == kernels, r
    assert r["partial_writes"] > sdwa, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*" + name + r"\w*):", text))) == kernels
    assert "k_dec_tiles" not in text and "k_enc_tiles" not in text      # the uniform kernels stay in their own units
    assert "s_load_dwordx4" in text


def test_list_units_are_in_the_library_build():
    mk = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/hgi_fused_list_dec.o" in mk and "$(OBJ)/hgi_fused_list_enc.o" in mk
    assert "hgi_framelist.h" in mk and "hgi_fused_list.h" in mk


def test_plan_and_block_map_under_asan_ubsan(tmp_path):
    """tests/cpp/test_framelist_plan.cpp: random lists walked block by block through the map the kernels run, and the overlap
    rule against a brute force (see the file's head for what it checks)."""
    exe = str(tmp_path / "test_framelist_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_framelist_plan.cpp"), "-o", exe])
    p = subprocess.run([exe, "300", "0x48474937"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "300 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
