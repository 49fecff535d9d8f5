"""CPU suite of requantize (libhgi_requant.so, include/hgi_requant.h, Encoder.requantize): the companion library exports its
three entry points and nothing else, names no tuning switch and reads no environment; the ctypes table matches the header; the C
entry point and the Python mirror refuse bad arguments before they touch a device; the kernel unit compiles for gfx950 within
the encoder's register and LDS budget and passes tools/check_isa.py; the two-sided host plan and the interval test hold under
ASan / UBSan (a stand-alone program); and the two facts of the oracle the design rests on: under the identity table re-coding
gives the source back (why the library refuses that table), and the lossless lift of the coverage designs decodes to the
designs (what the GPU suite feeds the kernels)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import geometry_designs as G
import operand_designs as D
import companion_layer as CL
from conftest import ROOT, SEED0

sys.path.insert(0, os.path.join(ROOT, "tools"))

REQUANT_DIR = os.path.join(ROOT, "rustyhgi_amd", "requant")
NAMES = ("hgi_requant_dev", "hgi_requant_last_error", "hgi_requant_version")


@pytest.fixture(scope="module")
def Q():
    return CL.binding("requant")


def _header():
    return CL.header("requant")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_three_entry_points(Q):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", Q.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(REQUANT_DIR, "hgi_requant.map")).read()
    assert re.search(r"global:\s*hgi_requant_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", _header()))
    assert declared == set(NAMES) == set(s[0] for s in Q.SYMBOLS)
    version = Q.lib().hgi_requant_version()
    assert version.startswith(b"hgi_requant 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    text = subprocess.check_output([strings, Q.LIB_PATH], text=True)
    assert re.findall(r"HGI_[A-Z0-9_]+", text) == []
    CL.check_sources(REQUANT_DIR, ["Makefile", "hgi_fused_requant.hip", "hgi_requant.hip", "hgi_requant.map", "hgi_requant_kernels.h", "hgi_requant_plan.h"])
    mk = CL.makefile(REQUANT_DIR, "requant", "hgi_fused_enc.hip")
    assert "-fvisibility=hidden" in mk and "-lhgi_hip" not in mk and "--version-script=hgi_requant.map" in mk
    for dep in re.findall(r'#include "(?:\.\./csrc/)?(hgi_[\w.]+)"', open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_impl.h")).read()):
        assert "$(CSRC)/" + dep in mk, dep + " is included by the tile procedure and missing from the Makefile's dependencies"
    for dep in ("hgi_fused_impl.h", "hgi_fused_enc.hip", "hgi_fused_pitched.h", "hgi_pitched.h", "hgi_kernels.h"):
        assert "$(CSRC)/" + dep in mk, dep
    # the same compiler flags as the three sibling libraries
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, flags=re.M).group(1)
    for sib, fused in (("recon", "hgi_fused_enc.hip"), ("map", "hgi_fused_dec.hip"), ("typed", "hgi_fused_enc.hip")):
        sib_mk = CL.makefile(os.path.join(ROOT, "rustyhgi_amd", sib), sib, fused)      # (no flags of its own: the fragment's)
        assert [m for m in re.findall(r"^CXXFLAGS \?= (.*)$", sib_mk, flags=re.M)] == [flags], sib
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", Q.LIB_PATH], text=True)


def test_ctypes_table_matches_the_header(Q):
    from rustyhgi_amd import _ffi
    ctype_of = {"const void *": _ffi._vp, "void *": _ffi._vp, "const uint8_t *": _ffi._vp, "uint32_t": _ffi._u32, "size_t": _ffi._sz,
                "hgi_interp": _ffi._int}
    m = re.search(r"HGI_API\s+hgi_status\s+hgi_requant_dev\s*\(([^)]*)\)", _header())
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    want, names = [], []
    for a in decl:
        a = re.sub(r"\[\d+\]$", "", a)
        if a.endswith("lut"):
            a = a.replace("uint8_t lut", "uint8_t *lut")       # `const uint8_t lut[256]` is a pointer
        names.append(re.search(r"(\w+)$", a).group(1))
        t = re.sub(r"\s*\*\s*", " *", re.match(r"(.*?)\s*\w+$", a).group(1)).strip()
        assert t in ctype_of, a
        want.append(ctype_of[t])
    assert names == ["hip_stream", "d_src", "src_pitch", "width", "height", "levels", "interp", "lut", "d_dst", "dst_pitch", "batch",
                     "src_frame_stride", "dst_frame_stride"]
    table = dict((s[0], s) for s in Q.SYMBOLS)
    _, res, got = table["hgi_requant_dev"]
    assert len(decl) == 13 and res is _ffi._int and got == want, decl
    for n in ("hgi_requant_last_error", "hgi_requant_version"):
        assert re.search(r"HGI_API\s+const\s+char\s*\*\s*" + n + r"\s*\(\s*void\s*\)", _header()), n
        assert table[n][1] is ctypes.c_char_p and table[n][2] == []
    # the header takes hgi_status / hgi_interp from hgi.h and declares no type of its own
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_requant.h")).read()
    assert not re.search(r"\b(typedef|struct|enum)\b", _header())


# ---------------------------------------------------------------------------------------------------- argument rules
def test_c_abi_refuses_bad_arguments_without_a_device(Q):
    """Every HGI_EINVAL / HGI_EUNSUPPORTED rule of include/hgi_requant.h, decided before the first HIP call: the buffers here
    are host memory (or plain numbers where the shape is too large to exist) and are never touched."""
    from rustyhgi_amd import _ffi
    L = Q.lib()
    a, o = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
    lut = (np.arange(256) // 2 * 2).astype(np.uint8)
    ident = np.arange(256, dtype=np.uint8)
    A, O, T, I = a.ctypes.data, o.ctypes.data, lut.ctypes.data, ident.ctypes.data
    E, U = _ffi.EINVAL, _ffi.EUNSUPPORTED
    err = L.hgi_requant_last_error

    def call(src=A, sp=40, w=32, h=8, levels=2, interp=1, lut=T, dst=O, dp=48, batch=1, sfs=320, dfs=384, stream=None):
        return L.hgi_requant_dev(stream, src, sp, w, h, levels, interp, lut, dst, dp, batch, sfs, dfs)

    # HGI_EINVAL
    assert call(lut=None) == E and b"lut" in err()
    assert call(src=None) == E and b"NULL" in err()
    assert call(dst=None) == E and b"NULL" in err()
    assert call(sp=31) == E and b"source pitch" in err()
    assert call(dp=31) == E and b"destination pitch" in err()
    assert call(batch=2, sfs=7 * 40 + 31) == E and b"source frame stride" in err()
    assert call(batch=2, dfs=7 * 48 + 31) == E and b"destination frame stride" in err()
    assert call(levels=32) == E and b"levels" in err()
    assert call(levels=2 ** 32 - 1) == E
    assert call(batch=2 ** 31) == E and b"batch" in err()
    # more tiles than a launch holds: 65536 x 32768 tiles of one frame (numbers only)
    assert call(src=1 << 50, dst=2 << 50, w=128 << 16, h=64 << 15, sp=128 << 16, dp=128 << 16) == E and b"tiles" in err()
    # in place, and overlapping byte intervals (conservative)
    assert call(dst=A) == E and b"in-place" in err()
    assert call(dst=A + 7 * 40 + 31) == E and b"overlaps the source span" in err()      # the source's last byte
    assert call(dst=A + 33) == E and b"overlaps" in err()                               # a window beside the source's in its rows
    assert call(src=A + 7 * 48 + 31, dst=A) == E and b"overlaps" in err()               # the destination's last byte
    assert call(batch=2, sfs=7 * 40 + 32, dst=A + 2 * (7 * 40 + 32) - 1) == E           # the second source frame's last byte
    # HGI_EUNSUPPORTED: depth, interpolator, 32-bit offsets, the tail rule, the identity table
    for levels in (0, 9, 31):
        assert call(levels=levels) == U and b"levels" in err()
    assert call(interp=7) == U and b"interpolator" in err()
    assert call(interp=-1) == U
    for side in ("sp", "dp"):      # (8 + 192) * 2^25 >= 2^32 on one side at a time (numbers only)
        assert call(src=1 << 50, dst=2 << 50, **{side: 1 << 25}) == U and b"32-bit" in err(), side
    assert call(lut=I) == U and b"identity" in err() and b"copy the source" in err()
    # width % 4 != 0 and the span's last byte at offset 4095 of its page: the three tail bytes leave the page
    raw, page = CL.page_aligned(3 * 4096)
    w, h, sp = 30, 8, 40
    span = (h - 1) * sp + w
    assert call(src=page + 4096 - span, w=w) == U and b"tail" in err() and b"4-KiB" in err()
    assert call(src=page + 4096 - span - 1, w=w) == U and call(src=page + 4096 - span - 2, w=w) == U
    assert call(batch=2, sfs=span + 5, src=page + 2 * 4096 - (span + 5) - span, w=w) == U and b"tail" in err()
    # ... HGI_EINVAL decides first when a rule of each kind is broken
    assert call(src=page + 4096 - span, w=w, dp=29) == E
    assert call(levels=9, dp=31) == E and call(levels=0, dst=A) == E and call(lut=I, dst=A + 5) == E and call(interp=7, lut=None) == E
    assert call(lut=I, levels=32) == E
    # empty calls succeed and do nothing (NULL buffers are fine there)
    assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    assert call(batch=0, src=None, dst=None) == _ffi.OK
    # ... whatever their other arguments are: the empty test is decided first
    for kw in (dict(levels=0), dict(levels=9), dict(levels=32), dict(lut=None), dict(lut=I), dict(interp=7), dict(sp=1, dp=1), dict(dst=A)):
        assert call(batch=0, **kw) == _ffi.OK and call(w=0, **kw) == _ffi.OK and call(h=0, **kw) == _ffi.OK, kw
    assert (a == 0).all() and (o == 0).all() and (raw == 0).all()


def test_entry_point_decides_every_rule_before_the_first_hip_call():
    """hgi_requant.hip: in the entry point no HIP call stands before the launch, the launch stands behind the last refusal, and
    every HGI_EINVAL rule stands before the first HGI_EUNSUPPORTED one."""
    CL.check_rule_order("requant", "hgi_requant_dev", "launch_requant")


# ------------------------------------------------------------------------------------------------------ kernel unit
@pytest.mark.timeout(900)
def test_requant_unit_is_within_the_encoder_budget(tmp_path):
    """k_requant<interp, unseeded | cone>: four kernels and no other -- none for the identity table --, the SDWA byte chains of
    both directions really there, the hazard rules of tools/check_isa.py (rule 4 covers the row stores: they go through
    store_row_pair / store_rows_edge), no scratch, no spills, no DPP, no traps, no static LDS (the table sits at LDS offset 0),
    and the VGPRs within the 96 of the five waves per SIMD the launch bounds declare."""
    import check_isa
    path = CL.isa("requant", tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 4, r
    assert r["partial_writes"] > 400, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_requant\w*):", text))) == 4
    assert "k_enc_tiles" not in text and "k_enc_pitched" not in text and "k_dec_tiles" not in text
    assert re.search(r"buffer_store_dwordx4 .* nt", text)
    res = CL.resources(text, "k_requant")
    assert len(res) == 4, res
    seen = set()
    for k, (vgprs, lds, scratch) in res.items():
        m = re.search(r"k_requantILi(\d)ELi(\d)E", k)
        assert m, k
        seen.add(tuple(int(v) for v in m.groups()))
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        # 512 VGPRs per SIMD lane, allocated in eights: five waves -> at most 96
        assert vgprs <= 96, (k, vgprs)
    assert seen == {(i, s) for i in (0, 1) for s in (0, 2)}
    src = CL.unit_source("requant", "hgi_fused_enc.hip")      # ... the uniform encoder's dynamic LDS, nothing added
    assert "amdgpu_waves_per_eu(HGI_ENC_WAVES_PER_EU)" in src


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_and_intervals_under_asan_ubsan(tmp_path):
    """tests/cpp/test_requant_plan.cpp, a stand-alone program: random shapes, pitches, alignments and batches; every block
    walked through the map, every 32-bit offset of both sides bounded, the `fast` rule, the tail rule and the interval test
    against plain 64-bit arithmetic and brute force."""
    CL.run_plan_program("requant", tmp_path, flags=("-Werror",))


# ------------------------------------------------------------------------------ oracle facts the design rests on
@pytest.mark.parametrize("interp", (1, 0))
def test_identity_table_gives_the_source_back(oracle, lena, interp):
    """encode(decode(g), noop_lut) == g, for grids of random bytes and for lossless encodes of images, at levels 0 ... 10 and 12: under
    the identity table the encoder keeps every residual d = a - p, and a and p are what the decoder made of the same grid.
    Decode is a bijection on grids (every level adds a prediction made of coarser points only) and this encode is its inverse,
    so the fact holds at any depth.  This is why hgi_requant_dev refuses the identity table and Encoder.requantize copies the
    rows, whatever its scale_level."""
    rng = np.random.default_rng(SEED0 + 77 + interp)
    noop = oracle.noop_lut()
    # 1 ... 8: what the library would serve; 0 and 9 ... 12: what Encoder.requantize answers with the same row copy
    for levels in list(range(1, 9)) + [0, 9, 10, 12]:
        for (w, h) in ((64, 128), (67, 131), (130, 260), (1, 1), (5, 3)):
            g = rng.integers(0, 256, (h, w), dtype=np.uint8)
            assert (oracle.encode(oracle.decode(g, levels, interp), levels, noop, interp) == g).all(), (w, h, levels)
        for img in (lena, lena[:131, :67], G.content(130, 67)):
            g = oracle.encode(np.ascontiguousarray(img), levels, noop, interp)
            assert (oracle.encode(oracle.decode(g, levels, interp), levels, noop, interp) == g).all(), (img.shape, levels)


def test_lossless_lift_of_the_designs_decodes_to_the_designs(oracle):
    """decode(encode(design, noop_lut)) == design for the quantizer designs and the predictor frames of the operand suite (both
    interpolators) and for the geometry suite's content: the lift tests/test_requant_gpu.py feeds hgi_requant_dev."""
    noop = oracle.noop_lut()
    frames = {}
    for name, frame, lv, _ in D.quant_designs():
        frames.setdefault((frame, lv), D.quant_frame(frame))
    for frame, (lv, _) in D.PRED_FRAMES.items():
        frames[(frame, lv)] = D.pred_frame(frame)
    for (frame, lv), img in sorted(frames.items()):
        for interp in (1, 0):
            assert (oracle.decode(oracle.encode(img, lv, noop, interp), lv, interp) == img).all(), (frame, lv, interp)
    for k, (w, h) in enumerate(G.shape_set("D")[::7] + G.shape_set("R")[::41]):
        img = G.content(w, h)
        for lv in (4, 5, 8):
            assert (oracle.decode(oracle.encode(img, lv, noop, k & 1), lv, k & 1) == img).all(), (w, h, lv)


# ------------------------------------------------------------------ the tile's planes between the two chains, as a model
_TW, _TH, _OFFS = 128, 64, (0, 4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def _staged(k):
    """The positions of a tile's halo frame that staging puts into `buf` (stage_issue / pitched_issue, stage_commit): the even
    body rows, the k halo rows TH + {0, 4, 8, ..}, and on each of those rows the halo columns TW + {0, 4, 8}, TW + 16 / 32 / 64
    on the rows = 0 mod 16 / 32 / 64 from 4 / 5 / 6 levels on."""
    nh = k if k >= 2 else 1
    out = set()
    for y in list(range(0, _TH, 2)) + [_TH + o for o in _OFFS[:nh]]:
        out |= {(x, y) for x in range(_TW)}
        out |= {(_TW + o, y) for i, o in enumerate(_OFFS) if i < 3 or (k >= i + 1 and y % o == 0)}
    return frozenset(out)


def _body_cells(s, inside):
    """dec_cells<CHECK> / enc_cells<CHECK> (the same loop in both): (corners, new points) of every body cell of level s."""
    step = 2 * s
    for y0 in range(0, _TH, step):
        for x0 in range(0, _TW, step):
            if not inside(x0, y0):
                continue
            new = [q for q, on in (((x0 + s, y0), inside(x0 + s, y0)), ((x0, y0 + s), inside(x0, y0 + s)),
                                   ((x0 + s, y0 + s), inside(x0 + s, y0) and inside(x0, y0 + s))) if on]
            yield [(x0, y0), (x0, y0 + step), (x0 + step, y0), (x0 + step, y0 + step)], new


def _dec_halo_cells(s, inside):
    """dec_halo_cells, statement by statement."""
    step, deep = 2 * s, s >= 4
    if inside(_TW, 0):
        for lane in range((_TH // step) + 1):
            y0 = lane * step
            if not inside(0, y0):
                continue
            corner = y0 == _TH
            xin = deep and inside(_TW + s, 0)
            yin = (deep or not corner) and inside(0, y0 + s)
            new = ([(_TW + s, y0)] if xin else []) + ([(_TW, y0 + s)] if yin else []) + ([(_TW + s, y0 + s)] if xin and yin else [])
            yield [(_TW, y0), (_TW, y0 + step), (_TW + step, y0), (_TW + step, y0 + step)], new
    if inside(0, _TH):
        for lane in range(_TW // step):
            x0 = lane * step
            if not inside(x0, 0):
                continue
            xin = inside(x0 + s, 0)
            yin = deep and inside(0, _TH + s)
            new = ([(x0 + s, _TH)] if xin else []) + ([(x0, _TH + s)] if yin else []) + ([(x0 + s, _TH + s)] if xin and yin else [])
            yield [(x0, _TH), (x0, _TH + step), (x0 + step, _TH), (x0 + step, _TH + step)], new


def _enc_halo_cells(s, inside):
    """enc_halo_cell for j = 0 ... ncy + ncx, field by field (lt / rt / lb / rb, nx / ny / nxy, xw / yw, active)."""
    step, deep = 2 * s, s >= 4
    ncx, ncy = _TW // step, _TH // step
    for j in range(ncy + 1 + ncx):
        col = j <= ncy
        y0 = j * step
        corner = y0 == _TH
        x0 = (j - ncy - 1) * step
        active = (inside(_TW, 0) and inside(0, y0)) if col else (inside(0, _TH) and inside(x0, 0))
        if not active:
            continue
        if col:
            xw, yw = deep and inside(_TW + s, 0), (deep or not corner) and inside(0, y0 + s)
            cs, pts = [(_TW, y0), (_TW, y0 + step), (_TW + step, y0), (_TW + step, y0 + step)], [(_TW + s, y0), (_TW, y0 + s), (_TW + s, y0 + s)]
        else:
            xw, yw = inside(x0 + s, 0), deep and inside(0, _TH + s)
            cs, pts = [(x0, _TH), (x0, _TH + step), (x0 + step, _TH), (x0 + step, _TH + step)], [(x0 + s, _TH), (x0, _TH + s), (x0 + s, _TH + s)]
        yield cs, [q for q, on in zip(pts, (xw, yw, xw and yw)) if on]


def _tile_model(k, cols, rows):
    """One tile whose image ends `cols` columns and `rows` rows behind its origin (beyond TW / TH: neighbours exist).  Walks the
    decoder's chain, then the encoder's, on sets of positions; returns nothing, asserts the claim of DESIGN.md 4.13."""
    def inside(x, y):
        return x < cols and y < rows
    staged = _staged(k)
    b = 1 << k
    zero = {q for q in staged if not inside(*q)}                          # staged as 0, and nothing may write them
    decoded = {q for q in staged if inside(*q) and q[0] % b == 0 and q[1] % b == 0}      # the base lattice is its own decoded value

    def value(q, have, what):
        # a corner is a staged position that holds a final value, or lies outside the image (0 by rule, staged or not)
        assert (q in have) or not inside(*q), (what, k, cols, rows, q)
        assert q in staged or not inside(*q), (what + ": read of a position staging never loaded", k, cols, rows, q)

    for lv in range(k - 1, 0, -1):
        s, new = 1 << lv, set()
        for cs, pts in list(_body_cells(s, inside)) + list(_dec_halo_cells(s, inside)):
            for q in cs:
                value(q, decoded, "decoder corner at s = %d" % s)
            for q in pts:
                assert q in staged and q not in zero and q not in decoded, ("decoder target at s = %d" % s, k, cols, rows, q)
                new.add(q)
        decoded |= new
    for y0 in range(0, min(_TH, rows), 2):                                # dec_fine_keep: the even rows' odd columns
        for x0 in range(0, min(_TW, cols), 2):
            for q in ((x0, y0), (x0, y0 + 2), (x0 + 2, y0), (x0 + 2, y0 + 2)):
                value(q, decoded, "dec_fine_keep corner")
            if inside(x0 + 1, y0):
                decoded.add((x0 + 1, y0))
    # the encoder's chain on what the decoder left: every original it reads from buf is decoded, every corner it reads from
    # rbuf is the base lattice (lattice_fast copied a DECODED value) or a point this chain has reconstructed
    rec = {q for q in decoded if q[0] % b == 0 and q[1] % b == 0}
    for lv in range(k - 1, 0, -1):
        s, new = 1 << lv, set()
        for cs, pts in list(_body_cells(s, inside)) + list(_enc_halo_cells(s, inside)):
            for q in cs:
                value(q, rec, "encoder corner at s = %d" % s)
            for q in pts:
                assert q in decoded and q not in zero, ("the encoder reads an undecoded byte at s = %d" % s, k, cols, rows, q)
                new.add(q)
        rec |= new
    for y0 in range(0, min(_TH, rows), 2):                                # enc_fine_fast
        for x0 in range(0, min(_TW, cols), 2):
            for q in ((x0, y0), (x0, y0 + 2), (x0 + 2, y0), (x0 + 2, y0 + 2)):
                value(q, rec, "enc_fine_fast corner")
            assert (x0, y0) in decoded and ((x0 + 1, y0) in decoded or not inside(x0 + 1, y0)), (k, cols, rows, x0, y0)


def test_encoder_chain_reads_only_bytes_the_decoder_chain_decoded():
    """The claim the kernel rests on, on a model of one tile's halo frame: the passes of both chains restated as
    sets of positions from hgi_fused_impl.h -- the shared body loop, dec_halo_cells statement by statement, enc_halo_cell field
    by field, the staging map of the halo columns (offset `off` only on rows = 0 mod off).  For every depth a tile holds and
    every way the image can end in or behind the tile: every byte the encoder's chain reads from `buf` is a byte the decoder's
    chain has decoded, every corner either chain reads holds its final value or lies outside the image, no pass writes a
    position outside the image or one staging never loaded, and nothing is decoded twice."""
    ends = (1, 5, 33, 63, 64, 65, 69, 127, 128, 129, 133, 137, 145, 161, 193, 256)       # the last: neighbours on every side
    for k in range(1, 7):
        for cols in ends:
            for rows in ends:
                _tile_model(k, cols, rows)


# ------------------------------------------------------------------------------------------------ Python validation
def _encoder():
    from rustyhgi_amd import Encoder
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    return Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)      # constructing it touches no device


def test_python_mirror_refuses_bad_views_before_any_device_call(Q):
    enc = _encoder()
    call = enc.requantize
    base = np.zeros((3, 64, 160), np.uint8)
    v = base[:, 8:40, 16:100]
    for bad in (base[:, :, ::2], base[:, ::-1], base.astype(np.float32), base.astype(np.int8), base.reshape(-1), base.reshape(1, 3, 64, 160),
                base.transpose(0, 2, 1), None, [[1, 2]]):
        with pytest.raises(ValueError):
            call(bad)
    other = np.zeros((3, 64, 160), np.uint8)
    ro = np.zeros((3, 32, 84), np.uint8)
    ro.setflags(write=False)
    for buf in (other[:, 8:40, 16:99], other[:2, 8:40, 16:100], other[:, 8:40, 16:184:2], other[:, 8:40, 16:100].astype(np.int8), ro, [1],
                other[:, 39:7:-1, 16:100]):
        with pytest.raises(ValueError, match="out"):
            call(v, out=buf)
    # shared memory: the same view, a window beside it in the parent's rows, the parent's later rows
    for buf in (v, base[:, 8:40, 70:154], base[:, 30:62, 16:100]):
        with pytest.raises(ValueError, match="`out` shares memory"):
            call(v, out=buf)
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, 64, 160), dtype=torch.uint8)
    tv = t[:, 8:40, 16:100]
    with pytest.raises(ValueError, match="out"):
        call(tv, out=np.zeros((3, 32, 84), np.uint8))
    with pytest.raises(ValueError):
        call(t[:, :, ::2])
    with pytest.raises(ValueError):
        call(t.to(torch.float16))
    with pytest.raises(ValueError, match="shares memory"):
        call(tv, out=tv)
    # a valid view passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        call(tv)
    with pytest.raises(ValueError, match="GPU"):
        call(tv, out=torch.zeros((3, 32, 84), dtype=torch.uint8))
    # empty views need no device
    assert call(base[:, :0]).shape == (3, 0, 160)
    assert call(base[:0], out=np.zeros((0, 64, 160), np.uint8)).shape == (0, 64, 160)
    assert call(np.zeros((5, 0), np.uint8)).shape == (5, 0)
    assert tuple(call(t[:, :0]).shape) == (3, 0, 160)


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("requant")
