"""CPU suite of the scaled view lists (libhgi_sviews.so, include/hgi_sviews.h, rustyhgi_amd.sviews): the companion library exports
its five entry points and nothing else, names no tuning switch, reads no environment and links nothing of the other libraries;
the ctypes table and the two structures match the header; the plan entry makes no HIP call and the launch entry decides its rules
-- one judgement function in a plain C++ header -- before the first one; the refusals recorded in
tests/golden/sviews_refusals.json repeat their status and text without a device; the kernel unit compiles for gfx950 without
spills at k_dec_scaled's wave budgets, passes tools/check_isa.py and runs k_dec_scaled's fast path call for call; the host plan
and the judgement hold under ASan / UBSan (tests/cpp/test_sviews_plan.cpp, a stand-alone program); ScaledViewPlan and
Decoder.decode_scaled_views serve what needs no device without one."""
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

SVIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "sviews")
NAMES = ("hgi_sviews_plan_bytes", "hgi_sviews_plan", "hgi_sviews_decode_dev", "hgi_sviews_last_error", "hgi_sviews_version")
FILES = ["Makefile", "hgi_fused_sviews_dec.hip", "hgi_sviews.hip", "hgi_sviews.map", "hgi_sviews_kernels.h", "hgi_sviews_plan.h"]
UNIT = "hgi_fused_sviews_dec.hip"
# the calls of k_dec_scaled's fast path, in its order: interior staging, ragged staging, the common tail
FAST_PATH = ["scaled_issue_rows<SH, false>", "cone_issue<false>", "stage_commit<false>", "scaled_issue_odd<SH, false>",
             "cone_issue<false>", "scaled_issue_rows<0, true>", "scaled_issue_odd<0, true>", "stage_commit<false>",
             "cone_finish<INTERP, false, true>", "dec_seed_commit", "dec_tile_edge<INTERP, 2>", "dec_tile_fast<INTERP>"]


@pytest.fixture(scope="module")
def S():
    return CL.binding("sviews")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_five_entry_points(S):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", S.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(SVIEWS_DIR, "hgi_sviews.map")).read()
    assert re.search(r"global:\s*hgi_sviews_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", CL.header("sviews")))
    assert declared == set(NAMES) == set(s[0] for s in S.SYMBOLS)
    version = S.lib().hgi_sviews_version()
    assert version.startswith(b"hgi_sviews 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of the other libraries linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, S.LIB_PATH], text=True)) == []
    CL.check_sources(SVIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_" not in subprocess.check_output([readelf, "-d", S.LIB_PATH], text=True).replace("libhgi_sviews", "")
    # the Makefile: the fragment the sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(SVIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert len(code) == 4 and code[:2] == ["NAME := sviews", "FUSED := hgi_fused_dec.hip"] and code[3] == "include ../companion/companion.mk", code
    assert code[2].startswith("ALSO := ") and "CXXFLAGS" not in mk
    also = code[2].split()[2:]
    assert all(os.path.isfile(os.path.join(SVIEWS_DIR, f)) for f in also), also
    assert {"../csrc/hgi_fused_scaled.hip", "../views/hgi_views_tile.h", "../views/hgi_views_kernels.h", "../views/hgi_views_plan.h",
            "../csrc/hgi_framelist.h", "../../include/hgi_views.h"} <= set(also)
    # the unit: the scaled unit as it stands (which brings the decode direction's unit without its launchers), the pitched
    # staging, the shared tile layer and the view lists' frame search behind it, in that order; the launch through the launch layer
    src = open(os.path.join(SVIEWS_DIR, UNIT)).read()
    order = [src.index('#include "%s"' % f) for f in ("../csrc/hgi_fused_scaled.hip", "../csrc/hgi_fused_pitched.h", "../companion/hgi_tile.h",
                                                      "../views/hgi_views_tile.h", "hgi_sviews_kernels.h")]
    assert order == sorted(order) and src.count("#include") == 5 and "#define" not in src
    scaled = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_scaled.hip")).read()
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in scaled and '#include "hgi_fused_dec.hip"' in scaled
    assert "launch_tile_kernel<k_dec_sviews<" in src and "with_choices(" in src and "hipLaunchKernelGGL" not in src
    assert "views_tile_launch(a, k, up)" in src and "dec_resident_tiles((u64)a.nedge + a.nint, max_width, k, t.cone)" in src
    assert "OneOf<2, 0>{t.cone ? 2 : 0}, OneOf<1, 2, 0>{shift == 1 ? 1 : shift == 2 ? 2 : 0}" in src
    # no device function, no store and no byte-checked path of its own
    assert src.count("__device__") == 0 and src.count("__global__") == 1
    assert "buffer_store" not in src and "store_rows" not in src and "store_row_pair" not in src and "_generic" not in src
    plan = open(os.path.join(SVIEWS_DIR, "hgi_sviews_plan.h")).read()
    assert '#include "../views/hgi_views_plan.h"' in plan and "struct ViewFrame" not in plan and not re.search(r"\bhip[A-Z_]\w*", plan)
    assert "views_aliasing(rects)" in plan and "tail_in_page" not in plan      # the view lists' sweep; no page rule
    head = open(os.path.join(ROOT, "include", "hgi_sviews.h")).read()
    assert "NO PAGE RULE" in head and "4-KiB" not in head


def test_kernel_body_is_k_dec_scaleds_fast_path_call_for_call():
    """k_dec_sviews: view_ctx(a), then the calls of k_dec_scaled's `if (fast)` block in its order, with its template arguments,
    and that kernel's wave budget per instantiation."""
    calls = r"\b(scaled_issue_rows<[^>]*>|scaled_issue_odd<[^>]*>|cone_issue<[^>]*>|cone_finish<[^>]*>|stage_commit<[^>]*>|dec_seed_commit|dec_tile_fast<[^>]*>|dec_tile_edge<[^>]*>)\s*\("
    scaled = open(os.path.join(ROOT, "rustyhgi_amd", "csrc", "hgi_fused_scaled.hip")).read()
    kernel = scaled[scaled.index("void k_dec_scaled("):]
    fast = kernel[kernel.index("if (fast) {"):kernel.index("// views whose byte offsets")]
    assert re.findall(calls, fast) == FAST_PATH
    src = open(os.path.join(SVIEWS_DIR, UNIT)).read()
    body = src[src.index("void k_dec_sviews("):src.index("}  // namespace\n")]
    assert re.findall(calls, body) == FAST_PATH
    assert body.index("view_ctx(a)") < body.index("if (vc.idle) return;") < body.index("scaled_issue_rows<")
    assert body.count("LDS_ORDER();") == fast.count("LDS_ORDER();") == 3
    budget = re.search(r"amdgpu_waves_per_eu\(([^\n]*?)\)\)\)\s*void k_dec_scaled\(", scaled).group(1)
    assert re.search(r"amdgpu_waves_per_eu\(([^\n]*?)\)\)\)\s*void k_dec_sviews\(", src).group(1) == budget


def test_ctypes_table_and_structures_match_the_header(S):
    head = CL.header("sviews")
    for name, fields in (("hgi_sview_pair", S.SViewPair), ("hgi_sviews_info", S.SViewsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), head, flags=re.S).group(1)
        declared = []
        for stmt in body.split(";"):
            m = re.match(r"\s*(uint32_t|uint64_t)\s+(.*)$", stmt.strip(), flags=re.S)
            if m:
                declared += [(n.strip(), ctypes.c_uint32 if m.group(1) == "uint32_t" else ctypes.c_uint64) for n in m.group(2).split(",")]
        assert declared == [(n, t) for n, t in fields._fields_], (name, declared)
    assert ctypes.sizeof(S.SViewPair) == 40 and ctypes.sizeof(S.SViewsInfo) == 56
    # hgi_views_info's layout with the shift in its reserved slot; the pair is the view lists'
    from rustyhgi_amd import _ffi_mviews, _ffi_views
    theirs, mine = _ffi_views.ViewsInfo._fields_, S.SViewsInfo._fields_
    assert [(n if n != "reserved" else "shift", t) for n, t in theirs] == mine
    assert [(n, getattr(S.SViewPair, n).offset) for n, _ in S.SViewPair._fields_] == [(n, getattr(_ffi_views.ViewPair, n).offset) for n, _ in _ffi_views.ViewPair._fields_]
    magic = int(re.search(r"#define HGI_SVIEWS_MAGIC (0x[0-9a-fA-F]+)u", head).group(1), 16)
    assert magic == S.MAGIC and magic not in (_ffi_views.MAGIC, _ffi_mviews.MAGIC)
    table = dict((s[0], s) for s in S.SYMBOLS)
    from rustyhgi_amd import _ffi
    want = {"hgi_sviews_plan_bytes": (_ffi._sz, [_ffi._sz]),
            "hgi_sviews_plan": (_ffi._int, [_ffi._vp, _ffi._sz, _ffi._u32, _ffi._vp, _ffi._sz, _ffi._vp]),
            "hgi_sviews_decode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int]),
            "hgi_sviews_last_error": (ctypes.c_char_p, []), "hgi_sviews_version": (ctypes.c_char_p, [])}
    assert set(want) == set(table)
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_sviews.h")).read()
    L = S.lib()
    assert [L.hgi_sviews_plan_bytes(n) for n in (0, 1, 4, 5)] == [0, 96, 288, 384]


def test_the_plan_makes_no_hip_call_and_the_launch_judges_first():
    """hgi_sviews.hip: nothing of HIP in the plan entry; in the launch entry the judgement -- one HIP-free function of the plan
    header, which holds every refusal, the HGI_EINVAL ones in front of the HGI_EUNSUPPORTED ones -- stands in front of the launch,
    and no refusal but the HGI_EDEVICE one behind it."""
    CL.check_rule_order("sviews", "hgi_sviews_decode_dev", "launch_sviews_decode")
    src = open(os.path.join(SVIEWS_DIR, "hgi_sviews.hip")).read()
    hip = r"\bhip[A-Z]\w*\s*\(|launch_sviews_\w+\s*\("
    plan = src[src.index("hgi_status hgi_sviews_plan("):src.index("hgi_status hgi_sviews_decode_dev(")]
    assert not re.search(hip, plan)
    assert plan[plan.rindex("return fail("):].count('"unknown verdict"') == 1      # (the default of the verdict switch: never reached)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", plan[:plan.rindex("return fail(")])) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", plan))
    order = [plan.index(k) for k in ("NULL argument", "plan_bytes %zu <", "shift %u out of range", "sviews_plan(views")]
    assert order == sorted(order)
    body = src[src.index("hgi_status hgi_sviews_decode_dev("):src.index("const char *hgi_sviews_last_error")]
    assert body.index("sviews_judge(") < body.index("return HGI_OK;") < body.index("return fail(") < body.index("launch_sviews_decode(")
    assert body.count("fail(HGI_EDEVICE") == 1 and body.index("launch_sviews_decode(") < body.index("fail(HGI_EDEVICE")
    # the plan header: the rules of a list in the header's order, nothing allocated before the tile count fits; the judgement:
    # one function, no HIP call, the empty plan first, then the rules in the header's order
    head = open(os.path.join(SVIEWS_DIR, "hgi_sviews_plan.h")).read()
    body = head[head.index("inline SViewsJudged sviews_plan("):head.index("// ---- the launch's judgement")]
    order = [body.index(k) for k in ("kSViewsNullEntry", "kSViewsSrcPitch", "kSViewsDstPitch", "kSViewsTiles", "views_aliasing(", "kSViewsShiftZero",
                                     "kSViewsRead32", "kSViewsWrite32", "memcpy(blob")]
    assert order == sorted(order)
    assert body.index("kSViewsTiles") < body.index("std::vector<ViewRect>")
    judge = head[head.index("inline SViewsLaunchJudged sviews_judge("):]
    order = [judge.index(k) for k in ("info->count == 0 && sviews_info_consistent", '"info is NULL"', "!sviews_info_consistent(", '"d_plan is NULL"', "16-byte aligned",
                                      "levels > 31", "interpolator %d unknown", "levels == 0", "levels <= info->shift", "levels - info->shift >= 9", "split_levels(")]
    assert order == sorted(order)
    assert max(m.start() for m in re.finditer(r"refuse\(HGI_EINVAL", judge)) < min(m.start() for m in re.finditer(r"refuse\(HGI_EUNSUPPORTED", judge))


# ---------------------------------------------------------------------------------------------------- argument rules
def _calls():
    with open(os.path.join(GOLDEN_DIR, "sviews_refusals.json")) as f:
        return json.load(f)["calls"]


def _plan(views, shift, keep):
    """hgi_sviews_plan of [[src, dst, w, h, sp, dp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_sviews as F
    n = len(views)
    arr = (F.SViewPair * max(n, 1))(*[F.SViewPair(*v) for v in views])
    size = F.lib().hgi_sviews_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.SViewsInfo()
    st = F.lib().hgi_sviews_plan(ctypes.addressof(arr), n, shift, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def replay(call):
    """One recorded call (tests/golden/make_sviews_refusals.py says what the fields mean): (status, error text)."""
    from rustyhgi_amd import _ffi_sviews as F
    L, keep = F.lib(), []
    if call["fn"] == "plan":
        views = call["views"]
        n = len(views) if views is not None else 1
        arr = (F.SViewPair * max(n, 1))(*[F.SViewPair(*v) for v in (views or [])])
        size = L.hgi_sviews_plan_bytes(n)
        host = np.full(size + 16, 0xEE, np.uint8)
        info = F.SViewsInfo()
        st = L.hgi_sviews_plan(ctypes.addressof(arr) if views is not None else None, n, call["shift"], host.ctypes.data if call["h_plan"] else None,
                               size if call["plan_bytes"] == "enough" else call["plan_bytes"], ctypes.addressof(info) if call["info"] else None)
        # a refused plan leaves the blob untouched and an info that no launch accepts: all zero
        assert (host == 0xEE).all() and bytes(info) == bytes(ctypes.sizeof(info)), "a refused plan wrote something"
    else:
        info = None
        if call["info"] is not None:
            st0, info, _ = _plan(call["info"], call["shift"], keep)
            assert st0 == 0, F.last_error()
            for k, v in call["damage"].items():
                setattr(info, k, v)
        st = L.hgi_sviews_decode_dev(None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["levels"], call["interp"])
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    calls = _calls()
    solo = [c["rule"] for c in calls if c["kind"] == "solo"]
    assert solo == ["null_argument", "plan_bytes", "shift_range", "null_entry", "src_pitch", "dst_pitch", "tiles", "out_out", "out_in", "shift_zero", "read32",
                    "write32", "info_null", "info_inconsistent", "d_plan_null", "d_plan_aligned", "levels_range", "interp", "levels_zero", "levels_shift", "depth"]
    assert sum(c["kind"] == "pair" for c in calls) >= 16
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in calls)      # refused before any device call
    assert set(c["call"]["fn"] for c in calls) == {"plan", "decode"}
    # HGI_EINVAL before HGI_EUNSUPPORTED: in every recorded pair that breaks one rule of each kind, the HGI_EINVAL text is recorded
    status = dict((c["rule"], c["status"]) for c in calls if c["kind"] == "solo")
    unsupported = set(r for r, s in status.items() if s == _ffi.EUNSUPPORTED)
    assert unsupported == {"shift_zero", "read32", "write32", "levels_zero", "levels_shift", "depth"}
    mixed = [c for c in calls if c["kind"] == "pair" and (c["rule"] in unsupported) != (c["also_breaks"] in unsupported)]
    assert len(mixed) >= 3 and all(c["status"] == _ffi.EINVAL for c in mixed)


def test_every_recorded_refusal_repeats_its_status_and_text(S):
    calls = _calls()
    for c in calls:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    # the texts name the offending list index
    named = dict((c["rule"], c["error"]) for c in calls if c["kind"] == "solo")
    for rule in ("null_entry", "write32"):
        assert named[rule].startswith("view 1:"), named[rule]
    for rule in ("src_pitch", "dst_pitch", "read32"):
        assert named[rule].startswith("view 0:"), named[rule]
    assert "views 0 and 1" in named["out_out"] and "output of view 1" in named["out_in"] and "grid of view 0" in named["out_in"]


def test_served_and_empty_plans_without_a_device(S):
    """What is NOT refused, as far as no device is needed: thumbnails side by side in one canvas's rows, grids overlapping grids,
    an image in the gap of a grid's pitch; the record holds the view; and the empty plans, which the launch accepts and does
    nothing for, whatever the other arguments.  The infos of the other view lists are not this library's, and the other way."""
    from rustyhgi_amd import _ffi
    A, B, keep = 1 << 50, 2 << 50, []
    side_by_side = [[A, B, 300, 200, 320, 512], [A + 7, B + 150, 300, 200, 320, 512], [A + (1 << 20), B + 100 * 512, 64, 1, 0, 0]]
    st, info, host = _plan(side_by_side, 1, keep)
    assert st == _ffi.OK, S.last_error()
    assert info.count == 3 and info.edge_tiles == 7 and info.interior_tiles == 2 and info.max_width == 150 and info.shift == 1 and info.magic == S.MAGIC
    assert info.plan_bytes == 3 * 64 + 2 * 16 and (host[int(info.plan_bytes):] == 0xEE).all()
    rec = host[:64].view(np.uint64)
    assert int(rec[0]) == A and int(rec[1]) == B      # addresses and sizes, no host pointer: the blob is position-independent
    words = host[:64].view(np.uint32)
    assert list(words[4:8]) == [150, 100, 1, 1] and list(words[8:12]) == [640, 512, 199 * 320 + 300, 99 * 512 + 150]      # the view; sp32, dp32, srec, drec
    one_row = host[128:192].view(np.uint32)
    assert list(one_row[4:6]) == [32, 1] and list(one_row[8:12]) == [64, 32, 64, 32]      # a one-row view reads behind its span below row 0
    # interior tiles and the last-row rule at shift 1: a 512-wide grid keeps every whole tile -- its last lattice byte is followed by
    # the byte that fills the dword; a 511-wide one gives up the tile rows that reach as far as its last lattice row (96 rows
    # below their origin), packed or at pitch 512: the dword behind that row's last byte lies behind the span either way
    for w, h, pitch, want in ((512, 256, 512, (2, 2)), (511, 255, 511, (2, 1)), (511, 255, 512, (2, 1)), (511, 257, 512, (2, 1)), (511, 511, 512, (2, 3)),
                              (512, 255, 512, (2, 2)), (512, 511, 1024, (2, 4))):
        st, info, host = _plan([[A, B, w, h, pitch, 256]], 1, keep)
        assert st == _ffi.OK, S.last_error()
        full = tuple(int(v) for v in host[:64].view(np.uint32)[6:8])
        assert full == want and info.interior_tiles == want[0] * want[1], (w, h, pitch, full)
    in_the_gap = [[A, B, 32, 8, 64, 16], [B + 1024, A + 32, 64, 8, 64, 64]]
    assert _plan(in_the_gap, 1, keep)[0] == _ffi.OK, S.last_error()
    L = S.lib()
    for views, shift in (([], 1), ([], 0), ([[0, 0, 0, 5, 0, 0], [0, 0, 7, 0, 1, 1]], 3), ([[0, 0, 0, 5, 0, 0]], 0)):
        st, info, _ = _plan(views, shift, keep)
        assert st == _ffi.OK and info.magic == S.MAGIC and info.count == 0 and info.plan_bytes == 0 and info.shift == shift
        for levels, interp, d_plan in ((4, 1, None), (0, 7, 8), (99, -1, None)):
            assert L.hgi_sviews_decode_dev(None, d_plan, ctypes.addressof(info), levels, interp) == _ffi.OK
    assert L.hgi_sviews_plan(None, 0, 99, None, 0, None) == _ffi.OK
    # foreign infos, both ways
    from rustyhgi_amd import _ffi_mviews, _ffi_qviews, _ffi_views
    st, mine, _ = _plan([[A, B, 300, 200, 320, 160]], 1, keep)
    assert st == _ffi.OK
    theirs = _ffi_views.ViewsInfo()
    views = (_ffi_views.ViewPair * 1)(_ffi_views.ViewPair(A, B, 300, 200, 320, 320))
    blob = np.zeros(256, np.uint8)
    assert _ffi_views.lib().hgi_views_plan(ctypes.addressof(views), 1, blob.ctypes.data, 256, ctypes.addressof(theirs)) == _ffi.OK
    as_mine = S.SViewsInfo()
    ctypes.memmove(ctypes.addressof(as_mine), ctypes.addressof(theirs), ctypes.sizeof(theirs))
    assert L.hgi_sviews_decode_dev(None, 1 << 40, ctypes.addressof(as_mine), 4, 1) == _ffi.EINVAL and "info is not" in S.last_error()
    assert _ffi_views.lib().hgi_views_decode_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1) == _ffi.EINVAL
    lut = (ctypes.c_uint8 * 256)(*[255 - i for i in range(256)])
    assert _ffi_views.lib().hgi_views_encode_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1, lut) == _ffi.EINVAL
    assert _ffi_qviews.lib().hgi_qviews_requant_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1, lut) == _ffi.EINVAL
    wide = _ffi_mviews.MViewsInfo()
    ctypes.memmove(ctypes.addressof(wide), ctypes.addressof(mine), ctypes.sizeof(mine))
    assert _ffi_mviews.lib().hgi_mviews_decode_dev(None, 1 << 40, ctypes.addressof(wide), 4, 1, 1 << 41) == _ffi.EINVAL


# ------------------------------------------------------------------------------------------------------ kernel unit
def _listing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    path = str(tmp_path / UNIT.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(SVIEWS_DIR, UNIT), "-o", path],
                          stderr=subprocess.DEVNULL)
    return path


def _metadata(text, kernel):
    """{template arguments: (VGPRs, spilled VGPRs, scratch bytes, static LDS bytes)} of the kernels named `kernel`, from the
    listing's metadata."""
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                         text, flags=re.S):
        k = re.search(r"%sILi(\d)ELi(\d)ELi(\d)E" % kernel, m.group(2))
        if k:
            res[tuple(int(v) for v in k.groups())] = (int(m.group(4)), int(m.group(5)), int(m.group(3)), int(m.group(1)))
    return res


@pytest.mark.timeout(900)
def test_unit_compiles_without_spills_and_passes_check_isa(tmp_path):
    """k_dec_sviews<interp, unseeded | cone, SH = 1 | 2 | 0>, twelve kernels: the hazard rules of tools/check_isa.py, no scratch,
    no spills, no DPP, no traps, no static LDS, at k_dec_scaled's wave budgets -- eight waves per SIMD for the wide loads of
    s = 1 (at most 64 VGPRs), six under the cone (80), four for s = 2 and the byte loads (128).  The listing also holds the twelve
    k_dec_scaled and k_gather_view of the included scaled unit, which nothing launches.  The frame search is scalar: the prefix
    arrays and the record are read with s_load."""
    import check_isa
    path = _listing(tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 25, r
    assert r["partial_writes"] > 1000, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_dec_sviews\w*):", text))) == 12
    assert not re.search(r"k_(dec|enc)_(tiles|pitched|list|views)\b", text)
    mine, model = _metadata(text, "k_dec_sviews"), _metadata(text, "k_dec_scaled")
    assert len(mine) == len(model) == 12 and set(mine) == set(model)
    for key, (vgprs, spills, scratch, lds) in sorted(mine.items()):
        interp, seeded, sh = key
        assert spills == 0 and scratch == 0 and lds == 0, (key, spills, scratch, lds)
        waves = 4 if sh != 1 else 6 if seeded == 2 else 8
        assert vgprs <= 512 // waves // 8 * 8, (key, vgprs)
        assert 512 // (-(-vgprs // 8) * 8) == 512 // (-(-model[key][0] // 8) * 8), (key, vgprs, model[key][0])      # the same waves fit by registers
    bodies = re.findall(r"^_Z\w*k_dec_sviews\w*:.*?^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(bodies) == 12
    for body in bodies:
        assert "k_dec_scaled" not in body and "s_load_dwordx4" in body


@pytest.mark.timeout(900)
def test_unit_is_within_k_dec_scaleds_vgpr_counts(tmp_path):
    """Every k_dec_sviews instantiation within the VGPR count of the k_dec_scaled instantiation of the same template arguments,
    both read from the metadata of one listing.

    Figures of this tree (-O3, gfx950), k_dec_sviews / k_dec_scaled, <interp, SEEDED, SH>, equal for both interpolators:
    <*, 0, 1> 60 / 60, <*, 0, 2> 90 / 90, <*, 0, 0> 83 / 86, <*, 2, 1> 68 / 70, <*, 2, 2> 90 / 92, <*, 2, 0> 90 / 92.  Without the
    layout hint on the interior branch of the s = 1 kernels the cone at s = 1 took 72: the same live values at the ragged tiles'
    masked stage_commit, one more register quad formed by the allocator."""
    text = open(_listing(tmp_path)).read()
    mine, model = _metadata(text, "k_dec_sviews"), _metadata(text, "k_dec_scaled")
    assert len(mine) == len(model) == 12
    for key in sorted(mine):
        print("k_dec_sviews<%d, %d, %d>: %d VGPRs, k_dec_scaled: %d" % (key + (mine[key][0], model[key][0])))
    over = dict((key, (mine[key][0], model[key][0])) for key in mine if mine[key][0] > model[key][0])
    assert not over, over


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_program_under_asan_ubsan(tmp_path):
    """tests/cpp/test_sviews_plan.cpp, a stand-alone program: random lists against a restatement of every rule, the records, the
    per-byte model of an interior tile's loads, the walk, aliasing against marked bytes, every rule alone and in pairs, the
    judgement (see the file's head)."""
    CL.run_plan_program("sviews", tmp_path, flags=("-Werror",))


# ----------------------------------------------------------------------------------------------------------- Python
def test_scaled_view_plan_refuses_bad_layouts_before_any_device_call(S):
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import ScaledViewPlan, scaled_shape
    assert [scaled_shape(h, w, s) for h, w, s in ((200, 300, 1), (201, 301, 1), (1, 1, 5), (0, 9, 2), (64, 64, 0))] == [(100, 150), (101, 151), (1, 1), (0, 3), (64, 64)]
    t = torch.zeros((64, 160), dtype=torch.uint8)
    o = torch.zeros((32, 80), dtype=torch.uint8)
    for src, dst in ((t[:, ::2], o[:, :40]), (t, o[:, :79]), (t, o[:31]), (t.to(torch.float16), o), (t.reshape(-1), o.reshape(-1)), (np.zeros((4, 4), np.uint8), o[:2, :2]),
                     (t.t(), o.t()), (t, o.to(torch.float32)), (t, t), (t, o[:, ::2]), (t, np.zeros((32, 80), np.uint8))):
        with pytest.raises(ValueError, match="pair 0"):
            ScaledViewPlan([(src, dst)], 1)
    with pytest.raises(ValueError, match="pair 1"):
        ScaledViewPlan([(t, o), (t, o[:, :79])], 1)
    for shift in (-1, 32, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="shift"):
            ScaledViewPlan([(t, o)], shift)
    # a valid layout passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        ScaledViewPlan([(t, o)], 1)
    with pytest.raises(ValueError, match="GPU"):
        ScaledViewPlan([(t[:63, :159], o)], 1)
    for shift in (0, 1, 31):
        p = ScaledViewPlan([], shift)
        assert len(p) == 0 and p.fused and p.blob is None and p.info.count == 0 and p.shift == shift


def test_decode_scaled_views_serves_empty_plans_without_a_device(S):
    torch = pytest.importorskip("torch")
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    dec = H.Decoder(Crossed())
    assert dec.decode_scaled_views(H.ScaledViewPlan([], 2), 4) == []
    e = [(torch.zeros((0, 9), dtype=torch.uint8), torch.zeros((0, 3), dtype=torch.uint8)), (torch.zeros((5, 0), dtype=torch.uint8), torch.zeros((2, 0), dtype=torch.uint8))]

    class _Plan:      # what a plan of empty CUDA views looks like, without a device
        srcs, dsts, layouts, fused, blob, shift = [a for a, _ in e], [b for _, b in e], [(0, 0, 9, 0, 9, 3), (0, 0, 0, 5, 0, 0)], True, None, 2
        device = None

        def __len__(self):
            return 2

    outs = dec.decode_scaled_views(_Plan(), 4)
    assert [tuple(o.shape) for o in outs] == [(0, 3), (2, 0)]


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("sviews", after="qviews")
    import rustyhgi_amd
    assert {"sviews", "ScaledViewPlan", "scaled_shape"} <= set(rustyhgi_amd.__all__)
    assert hasattr(rustyhgi_amd.Decoder, "decode_scaled_views") and "decode_scaled_views" in rustyhgi_amd.__doc__
    from rustyhgi_amd import _ffi_sviews
    assert _ffi_sviews.LIB_PATH.endswith("libhgi_sviews.so")
