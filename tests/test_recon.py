"""CPU suite of encode with reconstruction (libhgi_recon.so, include/hgi_recon.h, Encoder.encode_with_reconstruction): the
companion library exports its three entry points and nothing else, names no tuning switch and reads no environment; the ctypes
table matches the header; the C entry point and the Python mirror refuse bad arguments before they touch a device; the kernel
unit compiles for gfx950 within the encoder's register and LDS budget and passes tools/check_isa.py; the three-sided host plan
and the interval tests hold under ASan / UBSan (a stand-alone program)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import companion_layer as CL
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

RECON_DIR = os.path.join(ROOT, "rustyhgi_amd", "recon")
NAMES = ("hgi_recon_encode_u8_dev", "hgi_recon_last_error", "hgi_recon_version")


@pytest.fixture(scope="module")
def R():
    return CL.binding("recon")


def _header():
    return CL.header("recon")


def test_library_exports_exactly_the_three_entry_points(R):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", R.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(RECON_DIR, "hgi_recon.map")).read()
    assert re.search(r"global:\s*hgi_recon_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", _header()))
    assert declared == set(NAMES) == set(s[0] for s in R.SYMBOLS)
    assert b"gfx950" in R.lib().hgi_recon_version()
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    if strings:
        text = subprocess.check_output([strings, R.LIB_PATH], text=True)
        assert re.findall(r"HGI_[A-Z0-9_]+", text) == []
    CL.check_sources(RECON_DIR, ["Makefile", "hgi_fused_recon_enc.hip", "hgi_recon.hip", "hgi_recon.map", "hgi_recon_kernels.h", "hgi_recon_plan.h"])
    mk = CL.makefile(RECON_DIR, "recon", "hgi_fused_enc.hip")
    assert "-fvisibility=hidden" in mk and "-lhgi_hip" not in mk and "--version-script=hgi_recon.map" in mk
    for dep in re.findall(r'#include "(?:\.\./csrc/)?(hgi_[\w.]+)"', open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_impl.h")).read()):
        assert "$(CSRC)/" + dep in mk, dep + " is included by the tile procedure and missing from the Makefile's dependencies"
    readelf = shutil.which("readelf")
    if readelf:
        assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", R.LIB_PATH], text=True)


def test_ctypes_table_matches_the_header(R):
    from rustyhgi_amd import _ffi
    ctype_of = {"const void *": _ffi._vp, "void *": _ffi._vp, "const uint8_t *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz,
                "hgi_interp": _ffi._int}
    m = re.search(r"HGI_API\s+hgi_status\s+hgi_recon_encode_u8_dev\s*\(([^)]*)\)", _header())
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    want = []
    for a in decl:
        a = re.sub(r"\[\d+\]$", "", a)
        if a.endswith("lut"):
            a = a.replace("uint8_t lut", "uint8_t *lut")       # `const uint8_t lut[256]` is a pointer
        t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
        assert t in ctype_of, a
        want.append(ctype_of[t])
    table = dict((s[0], s) for s in R.SYMBOLS)
    _, res, got = table["hgi_recon_encode_u8_dev"]
    assert len(decl) == 16 and res is _ffi._int and got == want, decl
    for n in ("hgi_recon_last_error", "hgi_recon_version"):
        assert re.search(r"HGI_API\s+const\s+char\s*\*\s*" + n + r"\s*\(\s*void\s*\)", _header()), n
        assert table[n][1] is ctypes.c_char_p and table[n][2] == []
    # the header takes hgi_status / hgi_interp from hgi.h and declares no type of its own
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_recon.h")).read()
    assert not re.search(r"\b(typedef|struct|enum)\b", _header())


def test_c_abi_refuses_bad_arguments_without_a_device(R):
    """Every HGI_EINVAL / HGI_EUNSUPPORTED rule of include/hgi_recon.h, decided before the first HIP call: the buffers here are
    host memory (or plain numbers where the shape is too large to exist) and are never touched."""
    from rustyhgi_amd import _ffi
    L = R.lib()
    a, o, r = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    A, O, Rc, T = a.ctypes.data, o.ctypes.data, r.ctypes.data, lut.ctypes.data
    E, U = _ffi.EINVAL, _ffi.EUNSUPPORTED
    err = L.hgi_recon_last_error

    def call(src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, rec=Rc, rp=36, batch=1, sfs=320, dfs=384, rfs=300, stream=None):
        return L.hgi_recon_encode_u8_dev(stream, src, sp, w, h, levels, interp, lut, dst, dp, rec, rp, batch, sfs, dfs, rfs)

    # HGI_EINVAL
    assert call(lut=None) == E and b"lut" in err()
    assert call(src=None) == E and b"NULL" in err()
    assert call(dst=None) == E and call(rec=None) == E and b"NULL" in err()
    assert call(sp=31) == E and b"image pitch" in err()
    assert call(dp=31) == E and b"grid pitch" in err()
    assert call(rp=31) == E and b"reconstruction pitch" in err()
    assert call(batch=2, sfs=7 * 40 + 31) == E and b"image frame stride" in err()
    assert call(batch=2, dfs=7 * 48 + 31) == E and b"grid frame stride" in err()
    assert call(batch=2, rfs=7 * 36 + 31) == E and b"reconstruction frame stride" in err()
    assert call(levels=32) == E and b"levels" in err()
    assert call(levels=2 ** 32 - 1) == E
    assert call(batch=2 ** 31) == E and b"batch" in err()
    # more tiles than a launch holds: 65536 x 32768 tiles of one frame (numbers only)
    assert call(src=1 << 50, dst=2 << 50, rec=3 << 50, w=128 << 16, h=64 << 15, sp=128 << 16, dp=128 << 16, rp=128 << 16) == E and b"tiles" in err()
    # the three pairwise overlaps (conservative byte intervals), and in-place
    assert call(dst=A) == E and b"grid span overlaps the image span" in err()
    assert call(dst=A + 7 * 40 + 31) == E and b"grid span overlaps the image span" in err()      # the input's last byte
    assert call(dst=A + 33) == E                                                                 # a window beside the input's in its rows
    assert call(rec=A + 100) == E and b"reconstruction span overlaps the image span" in err()
    assert call(rec=O + 7 * 48 + 31) == E and b"reconstruction span overlaps the grid span" in err()
    assert call(rec=O - (7 * 36 + 31)) == E and b"reconstruction span overlaps the grid span" in err()
    assert call(rec=A) == E and b"in-place" in err()
    assert call(batch=2, sfs=7 * 40 + 32, rec=A + 2 * (7 * 40 + 32) - 1) == E                    # the second input frame's last byte
    # HGI_EUNSUPPORTED: depth, interpolator, 32-bit offsets, the tail rule
    for levels in (0, 9, 31):
        assert call(levels=levels) == U and b"levels" in err()
    assert call(interp=7) == U and b"interpolator" in err()
    assert call(interp=-1) == U
    for side in ("sp", "dp", "rp"):      # (8 + 192) * 2^25 >= 2^32 on one side at a time (numbers only)
        assert call(src=1 << 50, dst=2 << 50, rec=3 << 50, **{side: 1 << 25}) == U and b"32-bit" in err(), side
    # width % 4 != 0 and the span's last byte at offset 4095 of its page: the three tail bytes leave the page
    raw, page = CL.page_aligned(3 * 4096)
    w, h, sp = 30, 8, 40
    span = (h - 1) * sp + w
    assert call(src=page + 4096 - span, w=w, rp=36) == U and b"tail" in err() and b"4-KiB" in err()
    assert call(src=page + 4096 - span - 1, w=w) == U and call(src=page + 4096 - span - 2, w=w) == U
    assert call(batch=2, sfs=span + 5, src=page + 2 * 4096 - (span + 5) - span, w=w) == U and b"tail" in err()
    # ... a refusal, not a crash, when an EINVAL rule is broken too: the argument rules come first
    assert call(src=page + 4096 - span, w=w, rp=29) == E
    # empty calls succeed and do nothing (NULL buffers are fine there)
    assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    assert call(batch=0, src=None, dst=None, rec=None) == _ffi.OK
    # ... whatever their other arguments are: the empty test is decided first
    for kw in (dict(levels=0), dict(levels=9), dict(levels=32), dict(lut=None), dict(interp=7), dict(sp=1, dp=1, rp=1), dict(dst=A, rec=A)):
        assert call(batch=0, **kw) == _ffi.OK and call(w=0, **kw) == _ffi.OK and call(h=0, **kw) == _ffi.OK, kw
    assert (a == 0).all() and (o == 0).all() and (r == 0).all() and (raw == 0).all()


@pytest.mark.timeout(900)
def test_recon_unit_is_the_sdwa_build_within_the_encoder_budget(tmp_path):
    """k_enc_recon<interp, ident, unseeded | cone>: eight kernels, the SDWA quantizer really there, the hazard rules of
    tools/check_isa.py (rule 4 covers the four row stores of a task: they go through store_row_pair / store_rows_edge), no
    scratch, no spills, no DPP, no traps, no static LDS (the table sits at LDS offset 0), at most 128 VGPRs -- and, what DESIGN.md
    4.10 records, within the 102 of five waves per SIMD.  The uniform and pitched kernels stay in their own units."""
    import check_isa
    path = CL.isa("recon", tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 8, r
    assert r["partial_writes"] > 400, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_enc_recon\w*):", text))) == 8
    assert "k_enc_tiles" not in text and "k_enc_pitched" not in text
    res = CL.resources(text, "k_enc_recon")
    assert len(res) == 8, res
    for k, (vgprs, lds, scratch) in res.items():
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        assert vgprs <= 128, (k, vgprs)
        assert vgprs <= 102, (k, vgprs)      # five waves per SIMD, the encoder's occupancy


def test_dynamic_lds_is_the_uniform_encoders():
    """The formula stands once, in csrc/hgi_launch.h; the unit's launcher calls it, and the kernel lays the table, `buf` and
    `rbuf` out as the uniform encoder does."""
    src = CL.unit_source("recon", "hgi_fused_enc.hip")
    assert "u8 *buf = smem + 256 - HCOL;" in src and "u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;" in src


def test_plan_and_intervals_under_asan_ubsan(tmp_path):
    """tests/cpp/test_recon_plan.cpp, a stand-alone program: random shapes, pitches, alignments and batches; every block walked
    through the map, every 32-bit offset of all three sides bounded, the `fast` rule and the interval tests against brute force."""
    CL.run_plan_program("recon", tmp_path)


def _encoder():
    from rustyhgi_amd import Encoder
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    return Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)      # constructing it touches no device


def test_python_mirror_refuses_bad_views_before_any_device_call(R):
    enc = _encoder()
    call = enc.encode_with_reconstruction
    base = np.zeros((3, 64, 160), np.uint8)
    v = base[:, 8:40, 16:100]
    for bad in (base[:, :, ::2], base[:, ::-1], base.astype(np.float32), base.reshape(-1), base.transpose(0, 2, 1), None, [[1, 2]]):
        with pytest.raises(ValueError):
            call(bad)
    other = np.zeros((3, 64, 160), np.uint8)
    third = np.zeros((3, 64, 160), np.uint8)
    ro = np.zeros((3, 32, 84), np.uint8)
    ro.setflags(write=False)
    bad_bufs = (other[:, 8:40, 16:99], other[:2, 8:40, 16:100], other[:, 8:40, 16:184:2], other[:, 8:40, 16:100].astype(np.int8), ro, [1],
                other[:, 39:7:-1, 16:100])
    for buf in bad_bufs:
        with pytest.raises(ValueError, match="out"):
            call(v, out=buf)
        with pytest.raises(ValueError, match="recon"):
            call(v, recon=buf)
        with pytest.raises(ValueError, match="recon"):
            call(v, out=third[:, 8:40, 16:100], recon=buf)
    # shared memory: either output with the input (the same view, a window beside it in the parent's rows, the parent's later
    # rows), and the outputs with each other
    for buf in (v, base[:, 8:40, 70:154], base[:, 30:62, 16:100]):
        with pytest.raises(ValueError, match="`out` shares memory"):
            call(v, out=buf)
        with pytest.raises(ValueError, match="`recon` shares memory"):
            call(v, recon=buf)
    for (o, r) in ((other[:, 8:40, 16:100], other[:, 8:40, 16:100]), (other[:, 8:40, 0:84], other[:, 8:40, 76:160]),
                   (other[:, 0:32, 16:100], other[:, 31:63, 16:100])):
        with pytest.raises(ValueError, match="`recon` shares memory with `out`"):
            call(v, out=o, recon=r)
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, 64, 160), dtype=torch.uint8)
    tv = t[:, 8:40, 16:100]
    with pytest.raises(ValueError, match="out"):
        call(tv, out=np.zeros((3, 32, 84), np.uint8))
    with pytest.raises(ValueError, match="recon"):
        call(tv, recon=np.zeros((3, 32, 84), np.uint8))
    with pytest.raises(ValueError, match="recon"):
        call(v, recon=torch.zeros((3, 32, 84), dtype=torch.uint8))
    with pytest.raises(ValueError):
        call(t[:, :, ::2])
    # a valid view passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        call(tv)
    with pytest.raises(ValueError, match="GPU"):
        call(tv, out=torch.zeros((3, 32, 84), dtype=torch.uint8), recon=torch.zeros((3, 32, 84), dtype=torch.uint8))
    # empty views need no device
    g, r = call(base[:, :0])
    assert g.shape == (3, 0, 160) and r.shape == (3, 0, 160)
    g, r = call(base[:0], out=np.zeros((0, 64, 160), np.uint8))
    assert g.shape == (0, 64, 160) and r.shape == (0, 64, 160)
    g, r = call(np.zeros((5, 0), np.uint8))
    assert g.shape == (5, 0) and r.shape == (5, 0)


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("recon")
