"""CPU suite of the typed view lists (libhgi_tviews.so, include/hgi_tviews.h, rustyhgi_amd.tviews): the companion library exports
its five entry points and nothing else, names no tuning switch, reads no environment and links nothing of libhgi_hip.so; the
ctypes table and the two structures match the header; the plan entry makes no HIP call and the launch entry decides its rules
before the first one; the refusals recorded in tests/golden/tviews_refusals.json repeat their status and text without a device;
the kernel unit compiles for gfx950 within the typed encoder's budget and passes tools/check_isa.py; the host plan -- record
geometry with the read side in bytes, aliasing with E-byte elements, boundaries, the per-entry page rule -- holds under ASan /
UBSan (tests/cpp/test_tviews_plan.cpp, a stand-alone program); TypedViewPlan refuses bad layouts before any device call."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import companion_layer as CL
from conftest import GOLDEN_DIR, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

TVIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "tviews")
NAMES = ("hgi_tviews_plan_bytes", "hgi_tviews_plan", "hgi_tviews_encode_dev", "hgi_tviews_last_error", "hgi_tviews_version")
FILES = ["Makefile", "hgi_fused_tviews_enc.hip", "hgi_tviews.hip", "hgi_tviews.map", "hgi_tviews_kernels.h", "hgi_tviews_plan.h"]
UNIT = "hgi_fused_tviews_enc.hip"
WAVES, VGPR_BUDGET = 5, 96      # kTypedWavesPerEu: 512 VGPRs per SIMD lane, allocated in eights


@pytest.fixture(scope="module")
def T():
    return CL.binding("tviews")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_five_entry_points(T):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", T.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(TVIEWS_DIR, "hgi_tviews.map")).read()
    assert re.search(r"global:\s*hgi_tviews_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", CL.header("tviews")))
    assert declared == set(NAMES) == set(s[0] for s in T.SYMBOLS)
    version = T.lib().hgi_tviews_version()
    assert version.startswith(b"hgi_tviews 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, T.LIB_PATH], text=True)) == []
    CL.check_sources(TVIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", T.LIB_PATH], text=True)
    # the Makefile: the fragment the sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(TVIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert len(code) == 4 and code[:2] == ["NAME := tviews", "FUSED := hgi_fused_enc.hip"] and code[3] == "include ../companion/companion.mk", code
    assert code[2].startswith("ALSO := ") and "CXXFLAGS" not in mk and "EXTRA" not in mk
    also = code[2].split()[2:]
    assert all(os.path.isfile(os.path.join(TVIEWS_DIR, f)) for f in also), also
    # ... every file of the sibling directories that the units include, directly or through them, is a dependency
    src = open(os.path.join(TVIEWS_DIR, UNIT)).read()
    assert {"../typed/hgi_fused_typed_enc.hip", "../typed/hgi_typed_kernels.h", "../typed/hgi_typed_plan.h", "../views/hgi_views_tile.h",
            "../views/hgi_views_kernels.h", "../views/hgi_views_plan.h", "../mviews/hgi_mviews_plan.h", "../csrc/hgi_framelist.h",
            "../../include/hgi_views.h", "../../include/hgi_mviews.h"} <= set(also)
    included = set()
    for fn in FILES[1:3] + FILES[4:]:
        included |= set(re.findall(r'#include "(\.\./(?:typed|views|mviews|map)/[^"]+)"', open(os.path.join(TVIEWS_DIR, fn)).read()))
    assert included and included <= set(also), included - set(also)
    # the unit: the typed unit as it stands (which brings the encode direction's unit without its launchers, the pitched
    # staging and the shared tile layer, in that order), the view lists' frame search behind it, the launch through the launch layer
    assert src.index('#include "../typed/hgi_fused_typed_enc.hip"') < src.index('#include "../views/hgi_views_tile.h"') < src.index('#include "hgi_tviews_kernels.h"')
    assert "#define" not in src
    typed = open(os.path.join(ROOT, "rustyhgi_amd", "typed", "hgi_fused_typed_enc.hip")).read()
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in typed and '#include "../csrc/hgi_fused_enc.hip"' in typed
    assert typed.index('"../csrc/hgi_fused_pitched.h"') < typed.index('"../companion/hgi_tile.h"')
    assert "launch_tile_kernel<k_enc_tviews<" in src and "with_choices(" in src and "hipLaunchKernelGGL" not in src
    assert "views_tile_launch(a, k, up)" in src and "enc_lds_bytes(t.nh)" in src
    assert "view_ctx(a)" in src and "amdgpu_waves_per_eu(kTypedWavesPerEu)" in src
    # k_enc_typed's body: the typed staging, the cone on the frame's own samples, the encoder tile
    for piece, times in (("typed_issue<E, false>(", 1), ("typed_issue<E, true>(", 1), ("typed_issue_odd<E>(", 2), ("typed_convert_odd<E>(", 2),
                         ("cone_issue_typed<E>(", 2), ("cone_convert_typed<E>(", 2), ("stage_commit<true>(", 2), ("cone_finish<INTERP, true, IDENT>(", 2),
                         ("enc_seed_commit<SEEDED>(", 2), ("enc_tile_fast<INTERP, IDENT>(", 1), ("enc_tile_edge<INTERP, IDENT, ", 2)):
        assert src.count(piece) == times, piece
    # every store of the unit is the encoder tile's: none of its own
    assert "buffer_store" not in src and "store_rows" not in src and "store_row_pair" not in src
    plan = open(os.path.join(TVIEWS_DIR, "hgi_tviews_plan.h")).read()
    assert '#include "../mviews/hgi_mviews_plan.h"' in plan and '#include "../typed/hgi_typed_plan.h"' in plan
    assert "struct ViewFrame" not in plan and "struct MViewRect" not in plan and not re.search(r"\bhip[A-Z_]\w*", plan)


def test_ctypes_table_and_structures_match_the_header(T):
    head = CL.header("tviews")
    for name, fields in (("hgi_tview_pair", T.TViewPair), ("hgi_tviews_info", T.TViewsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), head, flags=re.S).group(1)
        declared = []
        for stmt in body.split(";"):
            m = re.match(r"\s*(uint32_t|uint64_t)\s+(.*)$", stmt.strip(), flags=re.S)
            if m:
                declared += [(n.strip(), ctypes.c_uint32 if m.group(1) == "uint32_t" else ctypes.c_uint64) for n in m.group(2).split(",")]
        assert declared == [(n, t) for n, t in fields._fields_], (name, declared)
    assert ctypes.sizeof(T.TViewPair) == 40
    # hgi_views_info's layout with the element size in its reserved slot, and nothing behind it
    from rustyhgi_amd import _ffi_mviews, _ffi_views
    theirs, mine = _ffi_views.ViewsInfo._fields_, T.TViewsInfo._fields_
    assert [(n if n != "reserved" else "elem_size", t) for n, t in theirs] == mine and ctypes.sizeof(T.TViewsInfo) == ctypes.sizeof(_ffi_views.ViewsInfo) == 56
    assert [(n, getattr(T.TViewsInfo, n).offset) for n, _ in mine] == [(n, getattr(_ffi_views.ViewsInfo, m).offset) for (n, _), (m, _) in zip(mine, theirs)]
    assert [(n, getattr(T.TViewPair, n).offset) for n, _ in T.TViewPair._fields_] == [(n, getattr(_ffi_views.ViewPair, n).offset) for n, _ in _ffi_views.ViewPair._fields_]
    magic = int(re.search(r"#define HGI_TVIEWS_MAGIC (0x[0-9a-fA-F]+)u", head).group(1), 16)
    assert magic == T.MAGIC and magic not in (_ffi_views.MAGIC, _ffi_mviews.MAGIC)
    table = dict((s[0], s) for s in T.SYMBOLS)
    from rustyhgi_amd import _ffi
    want = {"hgi_tviews_plan_bytes": (_ffi._sz, [_ffi._sz]),
            "hgi_tviews_plan": (_ffi._int, [_ffi._vp, _ffi._sz, _ffi._u32, _ffi._vp, _ffi._sz, _ffi._vp]),
            "hgi_tviews_encode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, ctypes.c_float, ctypes.c_float, _ffi._u32, _ffi._int, _ffi._vp]),
            "hgi_tviews_last_error": (ctypes.c_char_p, []), "hgi_tviews_version": (ctypes.c_char_p, [])}
    assert set(want) == set(table)
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_tviews.h")).read()
    L = T.lib()
    from rustyhgi_amd import _ffi_views as V
    assert [L.hgi_tviews_plan_bytes(n) for n in (0, 1, 4, 5)] == [0, 96, 288, 384] == [V.lib().hgi_views_plan_bytes(n) for n in (0, 1, 4, 5)]


def test_the_plan_makes_no_hip_call_and_the_launch_judges_first():
    """hgi_tviews.hip: nothing of HIP in the plan entry; in the launch entry the judge -- which holds every refusal, the
    HGI_EINVAL ones in front of the HGI_EUNSUPPORTED one, and no HIP call -- stands in front of the launch, and no refusal but the
    HGI_EDEVICE one behind it."""
    src = open(os.path.join(TVIEWS_DIR, "hgi_tviews.hip")).read()
    hip = r"\bhip[A-Z]\w*\s*\(|launch_tviews_\w+\s*\("
    plan = src[src.index("hgi_status hgi_tviews_plan("):src.index("hgi_status hgi_tviews_encode_dev(")]
    assert not re.search(hip, plan)
    assert plan[plan.rindex("return fail("):].count('"unknown verdict"') == 1      # (the default of the verdict switch: never reached)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", plan[:plan.rindex("return fail(")])) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", plan))
    judge = src[src.index("hgi_status judge_launch("):src.index("bool empty_plan(")]
    assert not re.search(hip, judge)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", judge)) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", judge))
    order = [judge.index(k) for k in ('"info is NULL"', "tviews_info_consistent(", '"d_plan is NULL"', "16-byte aligned", '"lut is NULL"', "elem_kind > 1",
                                      "elem_kind == 1 && info->elem_size != 2", "isfinite(scale)", "levels > 31", "interpolator %d unknown",
                                      "levels == 0 || levels > 8")]
    assert order == sorted(order)
    body = src[src.index("hgi_status hgi_tviews_encode_dev("):src.index("const char *hgi_tviews_last_error")]
    first = min(m.start() for m in re.finditer(hip, body))
    assert body[first:].startswith("launch_tviews_encode(") and body.index("judge_launch(") < first
    assert "fail(HGI_EINVAL" not in body and "fail(HGI_EUNSUPPORTED" not in body and body.count("fail(HGI_EDEVICE") == 1
    assert body.index("return HGI_OK;") < body.index("judge_launch(")      # the empty plan is decided first
    # the entry judges its own arguments in front of the list; the plan header judges in the header's order: per entry the NULL
    # side, the three element rules, the grid pitch; then tiles, aliasing; then the 32-bit bound and the page rule
    order = [plan.index(k) for k in ("NULL argument", "plan_bytes %zu <", "elem_size %u: frame elements", "tviews_plan(views")]
    assert order == sorted(order)
    head = open(os.path.join(TVIEWS_DIR, "hgi_tviews_plan.h")).read()
    body = head[head.index("inline TViewsJudged tviews_plan("):]
    order = [body.index(k) for k in ("kTViewsNullEntry", "kTViewsSrcAlign", "kTViewsSrcPitchAlign", "kTViewsSrcPitch", "kTViewsDstPitch", "kTViewsTiles",
                                     "mviews_aliasing(", "kTViewsFits32", "kTViewsTail", "memcpy(blob")]
    assert order == sorted(order)
    assert body.index("kTViewsTiles") < body.index("std::vector<MViewRect>")      # nothing is allocated before the tile count fits


# ---------------------------------------------------------------------------------------------------- argument rules
def _calls():
    with open(os.path.join(GOLDEN_DIR, "tviews_refusals.json")) as f:
        return json.load(f)["calls"]


def _plan(views, elem, keep):
    """hgi_tviews_plan of [[src, dst, w, h, sp, dp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_tviews as F
    n = len(views)
    arr = (F.TViewPair * max(n, 1))(*[F.TViewPair(*v) for v in views])
    size = F.lib().hgi_tviews_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.TViewsInfo()
    st = F.lib().hgi_tviews_plan(ctypes.addressof(arr), n, elem, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def replay(call):
    """One recorded call (tests/golden/make_tviews_refusals.py says what the fields mean): (status, error text)."""
    from rustyhgi_amd import _ffi_tviews as F
    L, keep = F.lib(), []
    if call["fn"] == "plan":
        views = call["views"]
        n = len(views) if views is not None else 1
        arr = (F.TViewPair * max(n, 1))(*[F.TViewPair(*v) for v in (views or [])])
        size = L.hgi_tviews_plan_bytes(n)
        host = np.full(size + 16, 0xEE, np.uint8)
        info = F.TViewsInfo()
        st = L.hgi_tviews_plan(ctypes.addressof(arr) if views is not None else None, n, call["elem"], host.ctypes.data if call["h_plan"] else None,
                               size if call["plan_bytes"] == "enough" else call["plan_bytes"], ctypes.addressof(info) if call["info"] else None)
        # a refused plan leaves the blob untouched and an all-zero info, which no launch accepts
        assert (host == 0xEE).all() and bytes(info) == bytes(ctypes.sizeof(info)), "a refused plan wrote something"
    else:
        info = None
        if call["info"] is not None:
            st0, info, _ = _plan(call["info"], call["elem"], keep)
            assert st0 == 0, F.last_error()
            for k, v in call["damage"].items():
                setattr(info, k, v)
        lut = np.arange(256, dtype=np.uint8)
        st = L.hgi_tviews_encode_dev(None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["kind"], float(call["scale"]),
                                     float(call["bias"]), call["levels"], call["interp"], lut.ctypes.data if call["lut"] else None)
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    calls = _calls()
    solo = [c["rule"] for c in calls if c["kind"] == "solo"]
    assert solo == ["null_argument", "plan_bytes", "elem_size", "null_entry", "src_align", "src_pitch_align", "src_pitch", "dst_pitch", "tiles", "out_out",
                    "out_in", "fits32", "tail", "info_null", "info_inconsistent", "d_plan_null", "d_plan_aligned", "lut_null", "elem_kind", "bf16_elem",
                    "scale_bias", "levels_range", "interp", "levels_launch"]
    assert sum(c["kind"] == "pair" for c in calls) >= 19
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in calls)      # refused before any device call
    assert set(c["call"]["fn"] for c in calls) == {"plan", "encode"}
    # HGI_EINVAL before HGI_EUNSUPPORTED: in every recorded pair that breaks one rule of each kind, the HGI_EINVAL text is recorded
    status = dict((c["rule"], c["status"]) for c in calls if c["kind"] == "solo")
    unsupported = set(r for r, s in status.items() if s == _ffi.EUNSUPPORTED)
    assert unsupported == {"fits32", "tail", "levels_launch"}
    mixed = [c for c in calls if c["kind"] == "pair" and (c["rule"] in unsupported) != (c["also_breaks"] in unsupported)]
    assert len(mixed) >= 2 and all(c["status"] == _ffi.EINVAL for c in mixed)


def test_every_recorded_refusal_repeats_its_status_and_text(T):
    calls = _calls()
    for c in calls:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    # the texts name the offending list index
    named = dict((c["rule"], c["error"]) for c in calls if c["kind"] == "solo")
    for rule in ("null_entry", "src_align", "tail"):
        assert named[rule].startswith("view 1:"), named[rule]
    for rule in ("src_pitch_align", "src_pitch", "dst_pitch", "fits32"):
        assert named[rule].startswith("view 0:"), named[rule]
    assert "views 0 and 1" in named["out_out"] and "grid of view 1" in named["out_in"] and "frame of view 0" in named["out_in"]


def test_served_and_empty_plans_without_a_device(T):
    """What is NOT refused, as far as no device is needed: grids side by side in one parent's rows, frames overlapping frames, a
    one-row view beside a window, a grid in the gap of a frame's pitch; the record's read side in bytes with the +2 tail of an
    odd width at E = 2; and the empty plans, which the launch accepts and does nothing for, whatever the other arguments."""
    from rustyhgi_amd import _ffi
    A, B, keep = 1 << 50, 2 << 50, []
    for E in (2, 4):
        side_by_side = [[A, B, 32, 8, 64 * E, 80], [A + 32 * E, B + 32, 32, 8, 64 * E, 80], [A + 8 * 64 * E, B + 8192, 63, 1, 0, 0]]
        st, info, host = _plan(side_by_side, E, keep)
        assert st == _ffi.OK, T.last_error()
        assert info.count == 3 and info.edge_tiles == 3 and info.interior_tiles == 0 and info.max_width == 63 and info.elem_size == E
        assert info.plan_bytes == 3 * 64 + 2 * 16 and (host[int(info.plan_bytes):] == 0xEE).all()
        rec = host[:64].view(np.uint64)
        assert int(rec[0]) == A and int(rec[1]) == B      # addresses and sizes, no host pointer: the blob is position-independent
        words = host[:64].view(np.uint32)
        assert list(words[4:6]) == [32, 8] and list(words[8:12]) == [64 * E, 80, 7 * 64 * E + 32 * E, 7 * 80 + 32]      # sp32, dp32, srec, drec
        one_row = host[128:192].view(np.uint32)
        # a one-row frame's pitch counts as its row, in bytes on the read side; an odd width of 2-byte elements has 2 records more
        assert list(one_row[8:12]) == [63 * E, 63, 63 * E + (2 if E == 2 else 0), 63]
        crops = [[A, B, 32, 8, 40 * E, 32], [A + 5 * E, B + 4096, 32, 8, 40 * E, 32], [A, B + 8192, 32, 8, 40 * E, 32]]
        assert _plan(crops, E, keep)[0] == _ffi.OK
        in_the_gap = [[A, B, 32, 8, 64 * E, 32], [B + 4096, A + 32 * E, 8, 8, 8 * E, 64 * E]]
        assert _plan(in_the_gap, E, keep)[0] == _ffi.OK, T.last_error()
        # the plan depends on the element size only: nothing of a kind, a scale or a table goes into it
    L = T.lib()
    lut = np.arange(256, dtype=np.uint8)
    for views in ([], [[0, 0, 0, 5, 0, 0], [0, 0, 7, 0, 1, 1]]):
        st, info, _ = _plan(views, 4, keep)
        assert st == _ffi.OK and info.magic == T.MAGIC and info.count == 0 and info.plan_bytes == 0
        for levels, interp, d_plan, table, kind, scale in ((4, 1, None, None, 0, 255.0), (0, 7, 8, lut.ctypes.data, 1, float("nan")), (99, -1, None, None, 9, float("inf"))):
            assert L.hgi_tviews_encode_dev(None, d_plan, ctypes.addressof(info), kind, scale, 0.0, levels, interp, table) == _ffi.OK
    assert L.hgi_tviews_plan(None, 0, 0, None, 0, None) == _ffi.OK
    # the view lists' and the mapped view lists' infos are not this library's
    from rustyhgi_amd import _ffi_mviews, _ffi_views
    theirs = _ffi_views.ViewsInfo()
    assert _ffi_views.lib().hgi_views_plan(None, 0, None, 0, ctypes.addressof(theirs)) == _ffi.OK
    mine = T.TViewsInfo()
    ctypes.memmove(ctypes.addressof(mine), ctypes.addressof(theirs), ctypes.sizeof(theirs))
    assert L.hgi_tviews_encode_dev(None, None, ctypes.addressof(mine), 0, 255.0, 0.0, 4, 1, lut.ctypes.data) == _ffi.EINVAL
    theirs = _ffi_mviews.MViewsInfo()
    assert _ffi_mviews.lib().hgi_mviews_plan(None, 0, 4, None, 0, ctypes.addressof(theirs)) == _ffi.OK
    ctypes.memmove(ctypes.addressof(mine), ctypes.addressof(theirs), ctypes.sizeof(mine))
    assert L.hgi_tviews_encode_dev(None, None, ctypes.addressof(mine), 0, 255.0, 0.0, 4, 1, lut.ctypes.data) == _ffi.EINVAL


# ------------------------------------------------------------------------------------------------------ kernel unit
def _metadata(text, kernel):
    """{mangled name: (vgpr_count, vgpr_spill_count, sgpr_spill_count, scratch bytes, static LDS bytes)} from the listing's metadata."""
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+).*?"
                         r"\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)", text, flags=re.S):
        if kernel in m.group(2):
            res[m.group(2)] = (int(m.group(5)), int(m.group(6)), int(m.group(4)), int(m.group(3)), int(m.group(1)))
    return res


@pytest.mark.timeout(900)
def test_unit_is_within_the_typed_encoders_budget(tmp_path):
    """k_enc_tviews<interp, identity | table, unseeded | cone, E = 2 | 4>, sixteen kernels: the hazard rules of tools/check_isa.py
    as the typed unit passes them, no scratch, no spills, no DPP, no traps, no static LDS, and k_enc_typed's occupancy: five
    waves per SIMD, at most 96 VGPRs, read from the listing's metadata.  The listing also holds the sixteen k_enc_typed kernels
    of the included typed unit, which nothing launches: within the same budget.  Nothing here searches the instructions: that
    is check_isa's."""
    import check_isa
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    path = str(tmp_path / UNIT.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(TVIEWS_DIR, UNIT), "-o", path],
                          stderr=subprocess.DEVNULL)
    r = check_isa.check(path)
    assert r["kernels"] == 32, r
    assert r["partial_writes"] > 800, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert VGPR_BUDGET == 512 // WAVES // 8 * 8
    for name in ("k_enc_tviews", "k_enc_typed"):
        res = _metadata(text, name)
        assert len(res) == 16, res
        for k, (vgprs, vspill, sspill, scratch, lds) in res.items():
            assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0, (k, vspill, sspill, scratch, lds)
            assert ("ELi4EEE" in k) != ("ELi2EEE" in k), k
            assert vgprs <= VGPR_BUDGET, (k, vgprs)
        assert set(CL.resources(text, name)) == set(res)


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_program_under_asan_ubsan(tmp_path):
    """tests/cpp/test_tviews_plan.cpp, a stand-alone program: the records of random small lists against typed_plan of a batch of
    one, the view lists' map, the aliasing test against bytes, the boundary rules on both sides, the per-entry page rule (see the
    file's head)."""
    CL.run_plan_program("tviews", tmp_path, flags=("-Werror",))


# ----------------------------------------------------------------------------------------------------------- Python
def test_typed_view_plan_refuses_bad_layouts_before_any_device_call(T):
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import TypedViewPlan
    f = torch.zeros((64, 160), dtype=torch.float16)
    g = torch.zeros((64, 160), dtype=torch.uint8)
    v = f[8:40, 16:100]
    for src, dst in ((f[:, ::2], g[:, :80]), (v, g[8:40, 16:99]), (g, g), (f.reshape(-1), g.reshape(-1)), (np.zeros((4, 4), np.float16), g[:4, :4]),
                     (f.t(), g.t()), (f.to(torch.float32), g), (f.to(torch.bfloat16), g), (f, f), (f[:, :80], g[:, ::2]), (f, np.zeros((64, 160), np.uint8)),
                     (f.to(torch.float64), g)):
        with pytest.raises(ValueError, match="pair 0"):
            TypedViewPlan([(src, dst)], torch.float16)
    with pytest.raises(ValueError, match="pair 1"):
        TypedViewPlan([(v, g[8:40, 16:100]), (f[:, ::2], g[:, :80])], torch.float16)
    for dtype in (torch.uint8, torch.float64, np.float32):
        with pytest.raises(ValueError, match="dtype"):
            TypedViewPlan([(v, g[8:40, 16:100])], dtype)
    # a valid layout passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        TypedViewPlan([(v, g[8:40, 16:100])], torch.float16)
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        p = TypedViewPlan([], dtype)
        assert len(p) == 0 and p.fused and p.blob is None and p.info.count == 0 and p.elem_size == (4 if dtype == torch.float32 else 2)
        assert enc.encode_typed_views(p) == []      # empty plans need no device
        for bad in (float("inf"), float("nan")):
            with pytest.raises(ValueError, match="finite"):
                enc.encode_typed_views(p, scale=bad)
            with pytest.raises(ValueError, match="finite"):
                enc.encode_typed_views(p, bias=bad)


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("tviews", after="mviews")
    import rustyhgi_amd
    assert {"tviews", "TypedViewPlan"} <= set(rustyhgi_amd.__all__)
    assert hasattr(rustyhgi_amd.Encoder, "encode_typed_views")
