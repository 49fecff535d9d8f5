"""CPU suite of pitched frames (hgi_encode_u8_pitched_dev / hgi_decode_u8_pitched_dev / hgi_encode_u8_pitched /
hgi_decode_u8_pitched): the library exports the four entry points, the ctypes table matches their declarations, the C ABI and
the Python mirror (Encoder.encode_view / Decoder.decode_view) refuse bad arguments before they touch a device, the view layouts
are accepted and refused as documented, the two new translation units compile for gfx950 within the uniform kernels' register
and LDS budget and pass tools/check_isa.py, and the host plan holds under ASan / UBSan."""
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

NAMES = ("hgi_encode_u8_pitched_dev", "hgi_decode_u8_pitched_dev", "hgi_encode_u8_pitched", "hgi_decode_u8_pitched")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgi.h")).read(), flags=re.S)


def _declaration(name):
    m = re.search(r"HGI_API\s+hgi_status\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_library_exports_the_four_pitched_entry_points():
    L = ctypes.CDLL(_ffi.LIB_PATH)
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in table, n
        assert hasattr(_ffi.lib(), n)
    # the version script exports the hgi_ prefix and nothing else; the header declares 43 entry points (39 + these four), all of them bound
    script = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi.map")).read()
    assert re.search(r"global:\s*hgi_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", _header()))
    assert len(declared) == 43 and set(NAMES) <= declared
    assert declared == set(s[0] for s in _ffi.SYMBOLS)
    nm = shutil.which("nm")
    if nm:
        out = subprocess.check_output([nm, "-D", "--defined-only", _ffi.LIB_PATH], text=True)
        exported = set(l.split()[-1].split("@")[0] for l in out.splitlines() if " T " in l)
        assert exported == declared, (exported ^ declared)


def test_ctypes_table_matches_the_header():
    ctype_of = {"hgi_ctx *": _ffi._vp, "const void *": _ffi._vp, "void *": _ffi._vp, "const uint8_t *": _ffi._vp,
                "uint8_t *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz, "hgi_interp": _ffi._int}
    table = dict((s[0], s) for s in _ffi.SYMBOLS)
    for n in NAMES:
        want = []
        for a in _declaration(n):
            a = re.sub(r"\[\d+\]$", "", a)
            if a.endswith("lut"):
                a = a.replace("uint8_t lut", "uint8_t *lut")       # `const uint8_t lut[256]` is a pointer
            t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
            assert t in ctype_of, (n, a)
            want.append(ctype_of[t])
        _, res, got = table[n]
        assert res is _ffi._int and got == want, (n, _declaration(n))
    assert [len(_declaration(n)) for n in NAMES] == [13, 12, 10, 9]


def test_c_abi_refuses_bad_arguments_without_a_device():
    """What the C entry points decide before touching a device.  Everything but the NULL ctx is tested before the ctx is used
    for anything but its path field, so a zeroed stand-in (path 0 = AUTO) serves as one here."""
    L = _ffi.lib()
    a = np.zeros(4096, np.uint8)
    o = np.zeros(4096, np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    A, O, T = a.ctypes.data, o.ctypes.data, lut.ctypes.data
    E, U = _ffi.EINVAL, _ffi.EUNSUPPORTED

    def enc_dev(c, src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, batch=1, sfs=320, dfs=384):
        return L.hgi_encode_u8_pitched_dev(c, src, sp, w, h, levels, interp, lut, dst, dp, batch, sfs, dfs)

    def dec_dev(c, src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, batch=1, sfs=320, dfs=384):
        return L.hgi_decode_u8_pitched_dev(c, src, sp, w, h, levels, interp, dst, dp, batch, sfs, dfs)

    def enc_host(c, src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, **_):
        return L.hgi_encode_u8_pitched(c, src, sp, w, h, levels, interp, lut, dst, dp)

    def dec_host(c, src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, **_):
        return L.hgi_decode_u8_pitched(c, src, sp, w, h, levels, interp, dst, dp)

    stand_in = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(stand_in)
    for call in (enc_dev, dec_dev, enc_host, dec_host):
        assert call(None) == E and b"NULL" in L.hgi_last_error()
        assert call(ctx, sp=31) == E and b"pitch" in L.hgi_last_error()
        assert call(ctx, dp=31) == E and b"pitch" in L.hgi_last_error()
        assert call(ctx, levels=32) == E
        assert call(ctx, interp=7) == U
        assert call(ctx, src=None) == E and call(ctx, dst=None) == E
        # overlapping spans: the same buffer, the output inside the input's span, and a window beside the input's in its rows
        assert call(ctx, dst=A) == E and b"overlap" in L.hgi_last_error()
        assert call(ctx, dst=A + 7 * 40 + 31) == E
        assert call(ctx, dst=A + 33) == E
    for call in (enc_dev, dec_dev):
        assert call(ctx, batch=2, sfs=7 * 40 + 31) == E and b"stride" in L.hgi_last_error()
        assert call(ctx, batch=2, dfs=7 * 48 + 31) == E and b"stride" in L.hgi_last_error()
        assert call(ctx, batch=2, sfs=7 * 40 + 32, dst=A + 2 * (7 * 40 + 32) - 1) == E      # the second input frame's last byte
        assert call(ctx, batch=2 ** 31) == E
    assert enc_dev(ctx, lut=None) == E and enc_host(ctx, lut=None) == E
    # a ctx set to the level-wise path: unsupported (hgi_ctx_set_path on the stand-in only stores the field)
    assert L.hgi_ctx_set_path(ctx, _ffi.PATH_LEVELWISE) == _ffi.OK
    for call in (enc_dev, dec_dev, enc_host, dec_host):
        assert call(ctx) == U and b"LEVELWISE" in L.hgi_last_error()


def _codec():
    from rustyhgi_amd import Decoder, Encoder
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    return Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4), Decoder(Crossed())      # constructing them touches no device


def test_view_layouts_accepted_and_refused():
    """_view_layout on numpy arrays and (CPU) torch tensors: any slice t[f0:f1, y0:y1, x0:x1] of a contiguous buffer passes with
    the parent's strides; steps, negative steps, transposes, expanded dimensions, other dtypes and ranks are refused."""
    from rustyhgi_amd.codec import _view_layout
    base = np.zeros((5, 60, 80), np.uint8)
    p0 = base.ctypes.data
    assert _view_layout(base, "t") == (p0, 5, 60, 80, 80, 4800, 4800)
    assert _view_layout(base[1:4, 7:50, 3:70], "t") == (p0 + 4800 + 7 * 80 + 3, 3, 43, 67, 80, 4800, 42 * 80 + 67)
    assert _view_layout(base[2, 7:50, 3:70], "t") == (p0 + 2 * 4800 + 7 * 80 + 3, 1, 43, 67, 80, 42 * 80 + 67, 42 * 80 + 67)
    assert _view_layout(base[::2, :, :], "t")[5] == 9600                       # a uniform frame stride of any size
    assert _view_layout(base[:, 5:6, :], "t")[4:] == (80, 4800, 80)            # one row: the pitch is the width
    assert _view_layout(base[:, ::2, :1], "t")[3:5] == (1, 160)                # one column: any row stride, the last stride is moot
    assert _view_layout(base[:, :0, :], "t")[1:4] == (5, 0, 80)                # empty: nothing to check
    for bad in (base[:, :, ::2], base[:, ::-1, :], base[::-1], base[:, :, ::-1], base.transpose(0, 2, 1), base.transpose(1, 0, 2)[:, :2],
                np.broadcast_to(base[:1], (3, 60, 80)), np.broadcast_to(base[0, :1], (60, 80)), base.astype(np.int16), base[0, 0],
                base[None], [[1, 2]], None):
        with pytest.raises(ValueError):
            _view_layout(bad, "t")
    torch = pytest.importorskip("torch")
    t = torch.zeros((5, 60, 80), dtype=torch.uint8)
    q0 = t.data_ptr()
    assert _view_layout(t[1:4, 7:50, 3:70], "t") == (q0 + 4800 + 7 * 80 + 3, 3, 43, 67, 80, 4800, 42 * 80 + 67)
    assert _view_layout(t[2, 7:50, 3:70], "t")[1:5] == (1, 43, 67, 80)
    for bad in (t[:, :, ::2], t.transpose(1, 2), t[:1].expand(3, 60, 80), t.to(torch.int32), t[0, 0], t[:, :, 1::2]):
        with pytest.raises(ValueError):
            _view_layout(bad, "t")


def test_python_mirror_refuses_bad_views_before_any_device_call():
    enc, dec = _codec()
    base = np.zeros((3, 64, 160), np.uint8)
    v = base[:, 8:40, 16:100]
    calls = (lambda x, **k: enc.encode_view(x, **k), lambda x, **k: dec.decode_view(x, 4, **k))
    for call in calls:
        for bad in (base[:, :, ::2], base[:, ::-1], base.astype(np.float32), base.reshape(-1), base.transpose(0, 2, 1)):
            with pytest.raises(ValueError):
                call(bad)
        other = np.zeros((3, 64, 160), np.uint8)
        ro = np.zeros((3, 32, 84), np.uint8)
        ro.setflags(write=False)
        for out in (other[:, 8:40, 16:99], other[:2, 8:40, 16:100], other[:, 8:40, 16:184:2], other[:, 8:40, 16:100].astype(np.int8), ro,
                    [1], other[:, 39:7:-1, 16:100]):
            with pytest.raises(ValueError, match="out"):
                call(v, out=out)
        # `out` sharing memory with the input: the same view, a window beside it in the parent's rows, the parent itself
        for out in (v, base[:, 8:40, 70:154], base[:, 30:62, 16:100]):
            with pytest.raises(ValueError, match="shares memory"):
                call(v, out=out)
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, 64, 160), dtype=torch.uint8)
    tv = t[:, 8:40, 16:100]
    for call in calls:
        with pytest.raises(ValueError, match="out"):
            call(tv, out=np.zeros((3, 32, 84), np.uint8))
        with pytest.raises(ValueError, match="out"):
            call(v, out=torch.zeros((3, 32, 84), dtype=torch.uint8))
        with pytest.raises(ValueError):
            call(t[:, :, ::2])
        # a valid view passes the layout checks and only then meets the CPU tensor
        with pytest.raises(ValueError, match="GPU"):
            call(tv)
        with pytest.raises(ValueError, match="GPU"):
            call(tv, out=torch.zeros((3, 32, 84), dtype=torch.uint8))
    # the existing calls keep refusing what is not C-contiguous
    with pytest.raises(ValueError, match="contiguous"):
        dec.decode_batch(np.zeros((3, 32, 84), np.uint8), 4, out=other[:, 8:40, 16:100])
    # empty views need no device
    assert enc.encode_view(base[:, :0]).shape == (3, 0, 160) and dec.decode_view(base[:0], 4).shape == (0, 64, 160)


def _isa(tmp_path, tu):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / (tu + ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "rustyhgi_amd", "csrc", tu), "-o", out], stderr=subprocess.DEVNULL)
    return out


def _kernel_resources(text, name):
    """{kernel: (vgprs, static LDS bytes, scratch bytes)} from the metadata of an ISA listing."""
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)",
                         text, flags=re.S):
        if name in m.group(2):
            res[m.group(2)] = (int(m.group(4)), int(m.group(1)), int(m.group(3)))
    return res


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tu,name,kernels,sdwa", [("hgi_fused_pitched_dec.hip", "k_dec_pitched", 4, 100),
                                                  ("hgi_fused_pitched_enc.hip", "k_enc_pitched", 8, 400)])
def test_pitched_units_are_the_sdwa_builds_within_the_uniform_budget(tmp_path, tu, name, kernels, sdwa):
    """k_dec_pitched<interp, unseeded | cone> and k_enc_pitched<interp, ident, unseeded | cone>: the SDWA paths really there, the
    hazard rules of tools/check_isa.py, no scratch, no spills, no traps, no static LDS (the encoder's table sits at LDS offset 0),
    and the occupancy of the uniform kernels: a plain decode tile within 64 VGPRs (eight waves per SIMD), a cone decode within
    80 (six), every encode within 94 (five)."""
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
    res = _kernel_resources(text, name)
    assert len(res) == kernels, res
    for k, (vgprs, lds, scratch) in res.items():
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        if name == "k_enc_pitched":
            assert vgprs <= 94, (k, vgprs)
        else:
            cone = "ELi2EEE" in k      # <INTERP, SEEDED = 2>
            assert vgprs <= (80 if cone else 64), (k, vgprs)


def test_dynamic_lds_of_a_pitched_tile_is_the_uniform_tile():
    """The pitched kernels allocate what the uniform 64-row kernels allocate (the launchers use the same buf_bytes / rbuf_bytes):
    4 848 bytes per decode tile and 7 648 per encode tile at four levels, as DESIGN.md states for the uniform build."""
    src = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_pitched_dec.hip")).read()
    assert "lds_for_waves((size_t)buf_bytes(nh), dec_resident_tiles(" in src
    src = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_pitched_enc.hip")).read()
    assert "lds_for_waves(enc_lds_bytes(nh), HGI_KNOB(HGI_ENC_WAVES, 0))" in src
    src = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_launch.h")).read()
    assert "enc_lds_bytes(int nh) { return (size_t)buf_bytes(nh) + ((rbuf_bytes(nh) + 15) & ~15) + 256; }" in src
    S, HR, HP, TH, nh = 128, 6, 40, 64, 4
    assert HR * HP + (TH // 2 + nh) * S == 4848
    assert 4848 + ((HR * HP + (TH // 2 + nh) * (S // 2) + 15) & ~15) + 256 == 7648


def test_pitched_units_are_in_the_library_build():
    mk = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "Makefile")).read()
    assert "$(OBJ)/hgi_fused_pitched_dec.o" in mk and "$(OBJ)/hgi_fused_pitched_enc.o" in mk
    assert "hgi_pitched.h" in mk and "hgi_fused_pitched.h" in mk


def test_plan_and_block_map_under_asan_ubsan(tmp_path):
    """tests/cpp/test_pitched_plan.cpp: random shapes, pitches, alignments and batches; every block walked through the map the
    kernels run, every 32-bit offset bounded, pitch == width against fused_geom's rule (see the file's head)."""
    exe = str(tmp_path / "test_pitched_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_pitched_plan.cpp"), "-o", exe])
    p = subprocess.run([exe, "1500", "0x48474938"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "1500 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
