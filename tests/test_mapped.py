"""CPU suite of mapped decode (libhgi_map.so, include/hgi_map.h, Decoder.decode_mapped, rustyhgi_amd.mapping): the companion
library exports its three entry points and nothing else, names no tuning switch and reads no environment; the ctypes table
matches the header; the C entry point and the Python mirror refuse bad arguments before they touch a device; the kernel unit
compiles for gfx950 within its declared register budgets, with no static LDS, and passes tools/check_isa.py; the two-sided host
plan and the interval tests hold under ASan / UBSan (a stand-alone program); affine_table is the float32 arithmetic it says."""
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

MAP_DIR = os.path.join(ROOT, "rustyhgi_amd", "map")
NAMES = ("hgi_map_decode_dev", "hgi_map_last_error", "hgi_map_version")


@pytest.fixture(scope="module")
def M():
    return CL.binding("map")


def _header():
    return CL.header("map")


def test_library_exports_exactly_the_three_entry_points(M):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", M.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(MAP_DIR, "hgi_map.map")).read()
    assert re.search(r"global:\s*hgi_map_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", _header()))
    assert declared == set(NAMES) == set(s[0] for s in M.SYMBOLS)
    version = M.lib().hgi_map_version()
    assert version.startswith(b"hgi_map 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    text = subprocess.check_output([strings, M.LIB_PATH], text=True)
    assert re.findall(r"HGI_[A-Z0-9_]+", text) == []
    CL.check_sources(MAP_DIR, ["Makefile", "hgi_fused_map_dec.hip", "hgi_map.hip", "hgi_map.map", "hgi_map_kernels.h", "hgi_map_plan.h"])
    mk = CL.makefile(MAP_DIR, "map", "hgi_fused_dec.hip")
    assert "-fvisibility=hidden" in mk and "-lhgi_hip" not in mk and "--version-script=hgi_map.map" in mk
    for dep in re.findall(r'#include "(?:\.\./csrc/)?(hgi_[\w.]+)"', open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_impl.h")).read()):
        assert "$(CSRC)/" + dep in mk, dep + " is included by the tile procedure and missing from the Makefile's dependencies"
    for dep in ("hgi_fused_impl.h", "hgi_fused_dec.hip", "hgi_fused_pitched.h", "hgi_pitched.h", "hgi_kernels.h"):
        assert "$(CSRC)/" + dep in mk, dep
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", M.LIB_PATH], text=True)


def test_ctypes_table_matches_the_header(M):
    from rustyhgi_amd import _ffi
    ctype_of = {"const void *": _ffi._vp, "void *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz, "hgi_interp": _ffi._int}
    m = re.search(r"HGI_API\s+hgi_status\s+hgi_map_decode_dev\s*\(([^)]*)\)", _header())
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    want = []
    for a in decl:
        t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
        assert t in ctype_of, a
        want.append(ctype_of[t])
    names = [re.search(r"(\w+)$", a).group(1) for a in decl]
    assert names == ["hip_stream", "d_grid", "grid_pitch", "width", "height", "levels", "interp", "d_table", "elem_size", "d_out",
                     "out_pitch", "batch", "grid_frame_stride", "out_frame_stride"]
    table = dict((s[0], s) for s in M.SYMBOLS)
    _, res, got = table["hgi_map_decode_dev"]
    assert len(decl) == 14 and res is _ffi._int and got == want, decl
    for n in ("hgi_map_last_error", "hgi_map_version"):
        assert re.search(r"HGI_API\s+const\s+char\s*\*\s*" + n + r"\s*\(\s*void\s*\)", _header()), n
        assert table[n][1] is ctypes.c_char_p and table[n][2] == []
    # the header takes hgi_status / hgi_interp from hgi.h and declares no type of its own
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_map.h")).read()
    assert not re.search(r"\b(typedef|struct|enum)\b", _header())


def test_c_abi_refuses_bad_arguments_without_a_device(M):
    """Every HGI_EINVAL / HGI_EUNSUPPORTED rule of include/hgi_map.h, decided before the first HIP call: the buffers here are
    host memory (or plain numbers where the shape is too large to exist) and are never touched -- a call that reached the
    launch would fail with HGI_EDEVICE on a machine without a GPU, or write, and neither happens."""
    from rustyhgi_amd import _ffi
    L = M.lib()
    g, o, t = np.zeros(4096, np.uint8), np.zeros(8192, np.uint8), np.zeros(2048, np.uint8)
    G, O, T = g.ctypes.data, o.ctypes.data + (-o.ctypes.data) % 4, t.ctypes.data
    E, U = _ffi.EINVAL, _ffi.EUNSUPPORTED
    err = L.hgi_map_last_error

    def call(grid=G, gp=40, w=32, h=8, levels=2, interp=1, table=T, elem=2, out=O, op=72, batch=1, gfs=320, ofs=600, stream=None):
        return L.hgi_map_decode_dev(stream, grid, gp, w, h, levels, interp, table, elem, out, op, batch, gfs, ofs)

    # HGI_EINVAL
    assert call(grid=None) == E and b"NULL" in err()
    assert call(table=None) == E and call(out=None) == E and b"NULL" in err()
    assert call(levels=32) == E and b"levels" in err()
    assert call(levels=2 ** 32 - 1) == E
    assert call(interp=7) == E and b"interpolator" in err()
    assert call(interp=-1) == E
    for elem in (0, 1, 3, 8):
        assert call(elem=elem, op=32 * max(elem, 1)) == E and b"elem_size" in err(), elem
    assert call(out=O + 1) == E and b"aligned" in err()                       # an odd d_out at E = 2
    assert call(out=O + 2, elem=4, op=128) == E and b"aligned" in err()
    assert call(op=62) == E and b"output pitch" in err()                      # short
    assert call(op=65) == E and b"multiple" in err()                          # not whole elements
    assert call(elem=4, op=130) == E and b"multiple" in err()
    assert call(elem=4, op=124) == E and b"output pitch" in err()
    assert call(gp=31) == E and b"grid pitch" in err()
    assert call(batch=2, gfs=7 * 40 + 31) == E and b"grid frame stride" in err()
    assert call(batch=2, ofs=7 * 72 + 62) == E and b"output frame stride" in err()
    assert call(batch=2, ofs=7 * 72 + 65) == E and b"multiple" in err()
    assert call(batch=2 ** 31) == E and b"batch" in err()
    # more tiles than a launch holds: 65536 x 32768 tiles of one frame (numbers only)
    assert call(grid=1 << 50, out=2 << 50, table=3 << 50, w=128 << 16, h=64 << 15, gp=128 << 16, op=256 << 16) == E and b"tiles" in err()
    # the three pairwise overlaps (conservative byte intervals)
    assert call(table=O) == E and b"table overlaps the output" in err()
    assert call(table=O + 7 * 72 + 63) == E and b"table overlaps the output" in err()          # the output's last byte
    assert call(table=O - 511) == E and b"table overlaps the output" in err()                  # the table's last byte
    assert call(table=G + 100) == E and b"table overlaps the grid" in err()
    assert call(table=G - 511) == E and b"table overlaps the grid" in err()
    assert call(elem=4, op=128, table=G - 1023) == E and b"table overlaps the grid" in err()   # 1 KiB at E = 4
    assert call(out=G) == E and b"output span overlaps the grid" in err()
    assert call(out=G + 7 * 40 + 30) == E and b"output span overlaps the grid" in err()        # the grid's last bytes
    assert call(out=G - (7 * 72 + 62)) == E and b"output span overlaps the grid" in err()      # the output's last bytes
    assert call(batch=2, gfs=7 * 40 + 32, out=G + 2 * (7 * 40 + 32) - 2) == E                  # the second grid frame's last bytes
    # HGI_EUNSUPPORTED: depth, 32-bit offsets on either side, the tail rule
    for levels in (0, 9, 31):
        assert call(levels=levels) == U and b"levels" in err()
    for side in ("gp", "op"):      # (8 + 192) * 2^25 >= 2^32 on one side at a time (numbers only)
        assert call(grid=1 << 50, out=2 << 50, table=3 << 50, **{side: 1 << 25}) == U and b"32-bit" in err(), side
    assert call(grid=1 << 50, out=2 << 50, table=3 << 50, gp=1 << 32) == U and b"32-bit" in err()      # a pitch >= 2^32
    assert call(grid=1 << 50, out=2 << 50, table=3 << 50, op=1 << 32) == U and b"32-bit" in err()
    # the same byte pitch is what counts: 2^24 elements of 4 bytes are refused, of 2 bytes served as far as the rules go
    assert call(grid=1 << 50, out=2 << 50, table=3 << 50, elem=4, op=4 << 24) == U
    # width % 4 != 0 and the span's last byte at offset 4095 of its page: the three tail bytes leave the page (a synthetic address)
    raw, page = CL.page_aligned(3 * 4096)
    w, h, gp = 30, 8, 40
    span = (h - 1) * gp + w
    assert call(grid=page + 4096 - span, w=w) == U and b"tail" in err() and b"4-KiB" in err()
    assert call(grid=page + 4096 - span - 1, w=w) == U and call(grid=page + 4096 - span - 2, w=w) == U
    assert call(batch=2, gfs=span + 5, grid=page + 2 * 4096 - (span + 5) - span, w=w) == U and b"tail" in err()
    assert call(grid=(1 << 50) + 4096 - span, out=2 << 50, table=3 << 50, w=w) == U and b"tail" in err()
    # ... a refusal, not a crash, when an EINVAL rule is broken too: the argument rules come first
    assert call(grid=page + 4096 - span, w=w, op=59) == E
    assert call(levels=0, elem=3) == E and call(levels=9, out=G) == E
    # empty calls succeed and do nothing (NULL buffers are fine there)
    assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    assert call(batch=0, grid=None, out=None, table=None) == _ffi.OK
    # ... whatever their other arguments are: the empty test is decided first
    for kw in (dict(levels=0), dict(levels=9), dict(levels=32), dict(table=None), dict(interp=7), dict(gp=1, op=1), dict(out=G, table=G),
               dict(elem=3), dict(out=O + 1)):
        assert call(batch=0, **kw) == _ffi.OK and call(w=0, **kw) == _ffi.OK and call(h=0, **kw) == _ffi.OK, kw
    assert (g == 0).all() and (o == 0).all() and (t == 0).all() and (raw == 0).all()


def test_entry_point_decides_every_rule_before_the_first_hip_call():
    """hgi_map.hip: in the entry point no HIP call stands before the launch, and the launch stands behind the last refusal."""
    CL.check_rule_order("map", "hgi_map_decode_dev", "launch_decode_map")


@pytest.mark.timeout(900)
def test_map_unit_is_within_its_budgets(tmp_path):
    """k_dec_map<interp, unseeded | cone, E>: eight kernels, dec_fine_fast's SDWA byte adds really there, the hazard rules of
    tools/check_isa.py (rule 4 covers the E-byte row stores: they all go through store_map_rows), no scratch, no spills, no DPP,
    no traps, no static LDS (the table's place is counted from LDS offset 0), and the VGPRs within the waves per SIMD each kernel
    declares -- DESIGN.md 4.11: E = 4 at the decoder's 8 (64), E = 2 at 7 (72), the cone two fewer (80 / 96).  The uniform and
    pitched kernels stay in their own units."""
    import check_isa
    path = CL.isa("map", tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 8, r
    assert r["partial_writes"] > 400, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_dec_map\w*):", text))) == 8
    assert "k_dec_tiles" not in text and "k_dec_pitched" not in text
    # the lookups are LDS reads of the element size, the wide stores nt
    assert "ds_read_b32" in text and "ds_read_u16" in text
    assert re.search(r"buffer_store_dwordx4 .* nt", text)
    res = CL.resources(text, "k_dec_map")
    assert len(res) == 8, res
    # 512 VGPRs per SIMD lane, allocated in eights: waves w -> at most (512 / w) rounded down to a multiple of 8
    budget = {(0, 4): 64, (0, 2): 72, (2, 4): 80, (2, 2): 96}      # (SEEDED, E) -> 8, 7, 6, 5 waves per SIMD
    seen = set()
    for k, (vgprs, lds, scratch) in res.items():
        m = re.search(r"k_dec_mapILi(\d)ELi(\d)ELi(\d)E", k)
        assert m, k
        interp, seeded, e = (int(v) for v in m.groups())
        seen.add((interp, seeded, e))
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        assert vgprs <= budget[(seeded, e)], (k, vgprs)
    assert seen == {(i, s, e) for i in (0, 1) for s in (0, 2) for e in (2, 4)}
    src = open(os.path.join(MAP_DIR, "hgi_fused_map_dec.hip")).read()
    assert "#define HGI_MAP_WAVES_PER_EU_E4 HGI_DEC_WAVES_PER_EU" in src and "#define HGI_MAP_WAVES_PER_EU_E2 (HGI_DEC_WAVES_PER_EU - 1)" in src


def test_dynamic_lds_is_the_decoders_plus_the_table_and_the_staging_rows():
    """The decoder's own layout first (no offset of the included procedure moves), the 256 * E bytes of the table behind it, then
    the 2 KiB of staging rows through which the lanes of a row exchange pixels; no static LDS."""
    src = CL.unit_source("map", "hgi_fused_dec.hip")
    assert "lds_for_waves((size_t)buf_bytes(t.nh) + 256 * (size_t)elem + kMapStageBytes, waves)" in src and "kMapStageBytes = 2 * TW * (NL / CH)" in src
    assert "u8 *tab = smem + buf_bytes(nh);" in src and "const_cast<u8 *>(tab) + 256 * E + 2 * TW * (lane >> LCH)" in src


def test_plan_and_intervals_under_asan_ubsan(tmp_path):
    """tests/cpp/test_map_plan.cpp, a stand-alone program: random shapes, pitches, alignments, batches and element sizes; every
    block walked through the map, every 32-bit offset of both sides bounded against the records, the fits, tail and interval
    rules against brute force."""
    CL.run_plan_program("map", tmp_path)


def _decoder():
    from rustyhgi_amd import Decoder
    from rustyhgi_amd.interpolator import Crossed
    return Decoder(Crossed())      # constructing it touches no device


def test_python_mirror_refuses_bad_arguments_before_any_device_call(M):
    call = _decoder().decode_mapped
    tab = np.arange(256, dtype=np.float16)
    base = np.zeros((3, 64, 160), np.uint8)
    v = base[:, 8:40, 16:100]
    # bad views
    for bad in (base[:, :, ::2], base[:, ::-1], base.astype(np.float32), base.reshape(-1), base.transpose(0, 2, 1), None, [[1, 2]]):
        with pytest.raises(ValueError):
            call(bad, 4, tab)
    # a bad table: 255 entries, 2-D, 1- and 8-byte dtypes, a stepped one, not an array
    for bad in (tab[:255], np.zeros((2, 256), np.float16), np.zeros((256, 1), np.float32), np.zeros(256, np.uint8), np.zeros(256, np.float64),
                np.zeros(512, np.float32)[::2], list(range(256)), None):
        with pytest.raises(ValueError, match="table"):
            call(v, 4, bad)
    # a bad `out`: wrong dtype, stepped, reversed, read-only, wrong shape, not an array
    other = np.zeros((3, 64, 200), np.float16)
    ro = np.zeros((3, 32, 84), np.float16)
    ro.setflags(write=False)
    bad_outs = (other[:, 8:40, 16:99], other[:2, 8:40, 16:100], other[:, 8:40, 16:184:2], other[:, 8:40, 16:100].astype(np.float32),
                other[:, 8:40, 16:100].view(np.uint16), np.zeros((3, 32, 84), np.uint8), ro, [1], other[:, 39:7:-1, 16:100])
    for buf in bad_outs:
        with pytest.raises(ValueError, match="out"):
            call(v, 4, tab, out=buf)
    with pytest.raises(ValueError, match="out"):
        call(v, 4, np.arange(256, dtype=np.float32), out=other[:, 8:40, 16:100])      # float16 out, float32 table
    # shared memory: out with the grids, out with the table, the table with the grids
    raw = np.zeros(3 * 64 * 160 * 2, np.uint8)
    gv = raw[:3 * 64 * 160].reshape(3, 64, 160)[:, 8:40, 16:100]
    ov = raw.view(np.float16).reshape(3, 64, 160)[:, 8:40, 16:100]
    with pytest.raises(ValueError, match="`out` shares memory with the grids"):
        call(gv, 4, tab, out=ov)
    tv = other.reshape(-1)[40 * 200:40 * 200 + 256]
    with pytest.raises(ValueError, match="`out` shares memory with `table`"):
        call(v, 4, tv, out=other[:, 8:40, 16:100])
    with pytest.raises(ValueError, match="`table` shares memory with the grids"):
        call(gv, 4, raw[2000:2512].view(np.float16))
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, 64, 160), dtype=torch.uint8)
    tview = t[:, 8:40, 16:100]
    ttab = torch.arange(256, dtype=torch.float32).to(torch.bfloat16)
    # the wrong kind: a torch table with numpy grids, a numpy `out` with torch grids
    with pytest.raises(ValueError, match="table"):
        call(v, 4, ttab)
    with pytest.raises(ValueError, match="out"):
        call(tview, 4, ttab, out=np.zeros((3, 32, 84), np.float16))
    for bad in (ttab[:255], ttab.reshape(2, 128), torch.zeros(256, dtype=torch.uint8), torch.zeros(256, dtype=torch.float64),
                torch.zeros(512, dtype=torch.float16)[::2], torch.zeros(256, dtype=torch.float16, device="meta")):
        with pytest.raises(ValueError, match="table"):
            call(tview, 4, bad)
    with pytest.raises(ValueError, match="out"):
        call(tview, 4, ttab, out=torch.zeros((3, 32, 84), dtype=torch.float16))
    with pytest.raises(ValueError):
        call(t[:, :, ::2], 4, ttab)
    # a valid view passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        call(tview, 4, ttab)
    with pytest.raises(ValueError, match="GPU"):
        call(tview, 4, ttab, out=torch.zeros((3, 32, 84), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="GPU"):
        call(tview, 4, np.arange(256, dtype=np.float32))      # a numpy table with torch grids is fine as far as the layouts go
    # empty views need no device
    r = call(base[:, :0], 4, tab)
    assert r.shape == (3, 0, 160) and r.dtype == np.float16
    r = call(base[:0], 4, np.zeros(256, np.float32), out=np.zeros((0, 64, 160), np.float32))
    assert r.shape == (0, 64, 160) and r.dtype == np.float32
    r = call(np.zeros((5, 0), np.uint8), 4, tab)
    assert r.shape == (5, 0)


def test_typed_layout_is_a_sibling_and_the_uint8_one_is_as_strict_as_before():
    from rustyhgi_amd import codec
    a = np.zeros((2, 10, 24), np.float32)
    ptr, b, h, w, pitch, fs, span = codec._typed_view_layout(a[:, 2:8, 4:20], "t", np.dtype(np.float32), 4)
    assert (ptr, b, h, w) == (a[:, 2:8, 4:20].ctypes.data, 2, 6, 16) and (pitch, fs, span) == (96, 960, 5 * 96 + 64)
    with pytest.raises(ValueError):
        codec._view_layout(a, "u8")      # the uint8 layout still takes uint8 alone
    with pytest.raises(ValueError):
        codec._typed_view_layout(np.zeros((2, 10, 24), np.uint8), "t", np.dtype(np.float32), 4)


def test_affine_table_is_the_float32_arithmetic_it_says():
    import rustyhgi_amd
    from rustyhgi_amd.mapping import affine_table
    assert rustyhgi_amd.affine_table is affine_table
    for dtype in (np.float16, np.float32):
        for scale, bias in ((1 / 255, 0.0), (1 / 255 / 0.229, -0.485 / 0.229), (2.0, -255.0)):
            got = affine_table(dtype, scale, bias)
            want = (np.arange(256, dtype=np.float32) * np.float32(scale) + np.float32(bias)).astype(dtype)
            assert got.dtype == np.dtype(dtype) and got.shape == (256,) and got.flags["C_CONTIGUOUS"]
            assert (got.view(np.uint16 if dtype is np.float16 else np.uint32) == want.view(np.uint16 if dtype is np.float16 else np.uint32)).all()
    d = affine_table(np.float16)
    assert d[0] == 0 and d[255] == 1 and (d.view(np.uint16) == (np.arange(256, dtype=np.float32) * np.float32(1 / 255)).astype(np.float16).view(np.uint16)).all()
    torch = pytest.importorskip("torch")
    for scale, bias in ((1 / 255, 0.0), (1 / 255 / 0.229, -0.485 / 0.229)):
        got = affine_table(torch.bfloat16, scale, bias)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (256,) and got.is_contiguous() and got.device.type == "cpu"
        f32 = np.arange(256, dtype=np.float32) * np.float32(scale) + np.float32(bias)
        want = torch.from_numpy(f32).to(torch.bfloat16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    t16 = affine_table(np.float16, device="cpu")
    assert t16.dtype == torch.float16 and torch.equal(t16.view(torch.int16), torch.from_numpy(d).view(torch.int16))


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("map", after="recon")
