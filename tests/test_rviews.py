"""CPU suite of the recon view lists (libhgi_rviews.so, include/hgi_rviews.h, rustyhgi_amd.rviews): the companion library exports
its five entry points and nothing else, names no tuning switch, reads no environment and links nothing of the other libraries;
the ctypes table and the two structures match the header; the plan entry makes no HIP call and the launch entry decides its rules
-- one judgement function in a plain C++ header -- before the first one; the refusals recorded in
tests/golden/rviews_refusals.json repeat their status and text without a device; the kernel unit compiles for gfx950 without
spills, passes tools/check_isa.py and runs k_enc_recon's body call for call; the host plan and the judgement hold under
ASan / UBSan (tests/cpp/test_rviews_plan.cpp, a stand-alone program); ReconViewPlan and
Encoder.encode_views_with_reconstruction serve what needs no device without one."""
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

RVIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "rviews")
NAMES = ("hgi_rviews_plan_bytes", "hgi_rviews_plan", "hgi_rviews_encode_dev", "hgi_rviews_last_error", "hgi_rviews_version")
FILES = ["Makefile", "hgi_fused_rviews_enc.hip", "hgi_rviews.hip", "hgi_rviews.map", "hgi_rviews_kernels.h", "hgi_rviews_plan.h"]
UNIT = "hgi_fused_rviews_enc.hip"
# the calls of k_enc_recon's body, in its order: what every tile does, the interior path, the ragged path
BODY = ["pitched_buf", "tile_side", "pitched_issue<false>", "cone_issue<true>", "stage_commit<true>", "pitched_issue_odd",
        "cone_finish<INTERP, true, IDENT>", "enc_seed_commit<SEEDED>", "enc_tile_fast_recon<INTERP, IDENT>", "cone_issue<true>",
        "pitched_issue<true, true>", "stage_commit<true>", "cone_finish<INTERP, true, IDENT>", "enc_seed_commit<SEEDED>",
        "enc_tile_edge_recon<INTERP, IDENT, 1>", "enc_tile_edge_recon<INTERP, IDENT, 2>"]
MEDIUM = bytes((i // 4) * 4 for i in range(256))      # (a table that is not the identity: no replayed call reads more of it)


@pytest.fixture(scope="module")
def R():
    return CL.binding("rviews")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_five_entry_points(R):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", R.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(RVIEWS_DIR, "hgi_rviews.map")).read()
    assert re.search(r"global:\s*hgi_rviews_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", CL.header("rviews")))
    assert declared == set(NAMES) == set(s[0] for s in R.SYMBOLS)
    version = R.lib().hgi_rviews_version()
    assert version.startswith(b"hgi_rviews 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of the other libraries linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, R.LIB_PATH], text=True)) == []
    CL.check_sources(RVIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_" not in subprocess.check_output([readelf, "-d", R.LIB_PATH], text=True).replace("libhgi_rviews", "")
    # the Makefile: the fragment the sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(RVIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert len(code) == 4 and code[:2] == ["NAME := rviews", "FUSED := hgi_fused_enc.hip"] and code[3] == "include ../companion/companion.mk", code
    assert code[2].startswith("ALSO := ") and "CXXFLAGS" not in mk
    also = code[2].split()[2:]
    assert all(os.path.isfile(os.path.join(RVIEWS_DIR, f)) for f in also), also
    assert {"../recon/hgi_fused_recon_enc.hip", "../recon/hgi_recon_kernels.h", "../recon/hgi_recon_plan.h", "../views/hgi_views_tile.h",
            "../views/hgi_views_kernels.h", "../views/hgi_views_plan.h", "../csrc/hgi_framelist.h", "../../include/hgi_views.h"} <= set(also)
    # the other companions' directories hold what they held: this library adds no file to them
    for name, n in (("recon", 6), ("views", 8), ("companion", 4)):
        assert len(os.listdir(CL.unit_dir(name))) - sum(f.startswith("_obj") for f in os.listdir(CL.unit_dir(name))) == n, name


def test_unit_includes_the_two_units_as_they_stand_and_has_no_store_of_its_own():
    """The unit: the recon unit as it stands (which brings the encode direction's unit without its launchers, the pitched staging
    and the shared tile layer) and the view lists' frame search behind it, then this library's launch interface; one device
    function -- the context function -- and the kernel; no store; the launch through the launch layer."""
    src = open(os.path.join(RVIEWS_DIR, UNIT)).read()
    order = [src.index('#include "%s"' % f) for f in ("../recon/hgi_fused_recon_enc.hip", "../views/hgi_views_tile.h", "hgi_rviews_kernels.h")]
    assert order == sorted(order) and src.count("#include") == 3 and "#define" not in src
    recon = open(os.path.join(ROOT, "rustyhgi_amd", "recon", "hgi_fused_recon_enc.hip")).read()
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in recon and '#include "../csrc/hgi_fused_enc.hip"' in recon
    assert recon.index('#include "../csrc/hgi_fused_pitched.h"') < recon.index('#include "../companion/hgi_tile.h"')
    assert src.count("__device__") == 1 and src.count("__global__") == 1 and "RViewTileCtx rview_ctx(const RViewArgs &a)" in src
    assert "launch_tile_kernel<k_enc_recon_views<I, ID != 0, SE>>(t.blocks, enc_lds_bytes(t.nh), s, a, k, lut, t.sd)" in src
    assert "with_choices(" in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert "views_tile_launch(a.v, k, up)" in src
    assert "interp_choice(interp), OneOf<1, 0>{ident ? 1 : 0}, OneOf<2, 0>{t.cone ? 2 : 0}" in src
    # no store and no byte-checked path of its own: every store is enc_fine_recon's
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("buffer_store", "store_rows", "store_row_pair", "_generic", "global_store", "raw_buffer", "__builtin_nontemporal_store"):
        assert word not in code, word
    # the context function: view_ctx with the frame index kept -- the same calls in the same order, and one more 16-byte load
    tile = open(os.path.join(ROOT, "rustyhgi_amd", "views", "hgi_views_tile.h")).read()
    theirs = tile[tile.index("ViewTileCtx view_ctx("):tile.index("// What both launchers work out first")]
    mine = src[src.index("RViewTileCtx rview_ctx("):src.index("// One block (= one wave) per tile")]
    steps = r"\b(list_role|list_find|rview_find|view_tile|__builtin_memcpy|__builtin_amdgcn_readfirstlane)\s*\("
    assert re.findall(steps, theirs) == ["list_role", "list_find", "__builtin_memcpy", "view_tile", "__builtin_amdgcn_readfirstlane", "__builtin_amdgcn_readfirstlane"]
    # (the search is rview_find of the plan header: list_find's result by an unrolled descent, so that no cycle stands in front of
    # the tile body; tests/cpp/test_rviews_plan.cpp holds the two equal)
    assert re.findall(steps, mine) == ["list_role", "rview_find", "__builtin_memcpy", "__builtin_memcpy", "view_tile", "__builtin_amdgcn_readfirstlane", "__builtin_amdgcn_readfirstlane"]
    assert "view_cv4 *third = (view_cv4 *)a.recon + r.frame;" in mine and mine.count("view_cv4 *") == 4 and "view_cu32 *pre" in mine
    plan = open(os.path.join(RVIEWS_DIR, "hgi_rviews_plan.h")).read()
    assert '#include "../views/hgi_views_plan.h"' in plan and "struct ViewFrame" not in plan and not re.search(r"\bhip[A-Z_]\w*", plan)
    find = plan[plan.index("inline uint32_t rview_find("):plan.index("// ---- the blob")]
    assert "#pragma unroll" in find and "for (uint32_t step = 1u << 30; step; step >>= 1)" in find and "while" not in find
    assert "views_aliasing(rects)" in plan and "side_fits32(" in plan and "tail_in_page(t.src" in plan and "extra_side(true" in plan


def test_kernel_body_is_k_enc_recons_call_for_call():
    """k_enc_recon_views: rview_ctx(a), then the calls of k_enc_recon's body in its order, with its template arguments, and that
    kernel's wave budget expression."""
    calls = (r"\b(pitched_buf|tile_side|pitched_issue<[^>]*>|pitched_issue_odd|cone_issue<[^>]*>|cone_finish<[^>]*>|stage_commit<[^>]*>|enc_seed_commit<[^>]*>|"
             r"enc_tile_fast_recon<[^>]*>|enc_tile_edge_recon<[^>]*>)\s*\(")
    recon = open(os.path.join(ROOT, "rustyhgi_amd", "recon", "hgi_fused_recon_enc.hip")).read()
    model = recon[recon.index("void k_enc_recon("):recon.index("}  // namespace\n")]
    assert re.findall(calls, model) == BODY
    src = open(os.path.join(RVIEWS_DIR, UNIT)).read()
    body = src[src.index("void k_enc_recon_views("):src.index("}  // namespace\n")]
    assert re.findall(calls, body) == BODY
    assert body.index("rview_ctx(a)") < body.index("if (rc.v.idle) return;") < body.index("pitched_buf(")
    assert body.count("LDS_ORDER();") == model.count("LDS_ORDER();") == 2
    assert "pitched_buf(fr, out, p, tl, &rb)" in body and "tile_side(rc.x, rout, tl, 1)" in body and "c.x = ExtraSide{S.pitch32, S.rec, 0};" in src
    assert "if (tl.X0 + TW <= W && !(H & 1u))" in body and "if (tl.X0 + TW <= W && !(H & 1u))" in model
    assert "u8 *slut = smem;" in body and "u8 *buf = smem + 256 - HCOL;" in body and "u8 *rbuf = smem + 256 + buf_bytes(nh) - RCOL;" in body
    budget = re.search(r"amdgpu_waves_per_eu\(([^\n]*?)\)\)\)\s*void k_enc_recon\(", recon).group(1)
    assert re.search(r"amdgpu_waves_per_eu\(([^\n]*?)\)\)\)\s*void k_enc_recon_views\(", src).group(1) == budget


def test_ctypes_table_and_structures_match_the_header(R):
    head = CL.header("rviews")
    for name, fields in (("hgi_rview_triple", R.RViewTriple), ("hgi_rviews_info", R.RViewsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), head, flags=re.S).group(1)
        declared = []
        for stmt in body.split(";"):
            m = re.match(r"\s*(uint32_t|uint64_t)\s+(.*)$", stmt.strip(), flags=re.S)
            if m:
                declared += [(n.strip(), ctypes.c_uint32 if m.group(1) == "uint32_t" else ctypes.c_uint64) for n in m.group(2).split(",")]
        assert declared == [(n, t) for n, t in fields._fields_], (name, declared)
    assert ctypes.sizeof(R.RViewTriple) == 56 and ctypes.sizeof(R.RViewsInfo) == 64
    # hgi_views_info's layout, a magic of its own and one more field
    from rustyhgi_amd import _ffi_mviews, _ffi_sviews, _ffi_tviews, _ffi_views
    assert R.RViewsInfo._fields_ == _ffi_views.ViewsInfo._fields_ + [("recon_offset", ctypes.c_uint64)]
    assert [(n, getattr(R.RViewsInfo, n).offset) for n, _ in _ffi_views.ViewsInfo._fields_] == [(n, getattr(_ffi_views.ViewsInfo, n).offset) for n, _ in _ffi_views.ViewsInfo._fields_]
    magic = int(re.search(r"#define HGI_RVIEWS_MAGIC (0x[0-9a-fA-F]+)u", head).group(1), 16)
    assert magic == R.MAGIC == int.from_bytes(b"1GRV", "little") and magic not in (_ffi_views.MAGIC, _ffi_mviews.MAGIC, _ffi_tviews.MAGIC, _ffi_sviews.MAGIC)
    table = dict((s[0], s) for s in R.SYMBOLS)
    from rustyhgi_amd import _ffi
    want = {"hgi_rviews_plan_bytes": (_ffi._sz, [_ffi._sz]),
            "hgi_rviews_plan": (_ffi._int, [_ffi._vp, _ffi._sz, _ffi._vp, _ffi._sz, _ffi._vp]),
            "hgi_rviews_encode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int, _ffi._vp]),
            "hgi_rviews_last_error": (ctypes.c_char_p, []), "hgi_rviews_version": (ctypes.c_char_p, [])}
    assert set(want) == set(table)
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_rviews.h")).read()
    L = R.lib()
    assert [L.hgi_rviews_plan_bytes(n) for n in (0, 1, 4, 5)] == [0, 96 + 16, 288 + 64, 384 + 80]
    # include/hgi.h and the other headers are the parent's: this library's names appear in none of them
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn != "hgi_rviews.h":
            assert "rviews" not in open(os.path.join(ROOT, "include", fn)).read(), fn


def test_the_plan_makes_no_hip_call_and_the_launch_judges_first():
    """hgi_rviews.hip: nothing of HIP in the plan entry; in the launch entry the judgement -- one HIP-free function of the plan
    header, which holds every refusal, the HGI_EINVAL ones in front of the HGI_EUNSUPPORTED one -- stands in front of the launch,
    and no refusal but the HGI_EDEVICE one behind it."""
    CL.check_rule_order("rviews", "hgi_rviews_encode_dev", "launch_rviews_encode")
    src = open(os.path.join(RVIEWS_DIR, "hgi_rviews.hip")).read()
    hip = r"\bhip[A-Z]\w*\s*\(|launch_rviews_\w+\s*\("
    plan = src[src.index("hgi_status hgi_rviews_plan("):src.index("hgi_status hgi_rviews_encode_dev(")]
    assert not re.search(hip, plan)
    assert plan[plan.rindex("return fail("):].count('"unknown verdict"') == 1      # (the default of the verdict switch: never reached)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", plan[:plan.rindex("return fail(")])) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", plan))
    order = [plan.index(k) for k in ("NULL argument", "plan_bytes %zu <", "rviews_plan(triples")]
    assert order == sorted(order)
    assert '#include "../companion/hgi_entry.h"' in src and "g_err" in src and "thread_local" not in src      # the error slot is the shared host layer's
    body = src[src.index("hgi_status hgi_rviews_encode_dev("):src.index("const char *hgi_rviews_last_error")]
    assert body.index("rviews_judge(") < body.index("return HGI_OK;") < body.index("return fail(") < body.index("launch_rviews_encode(")
    assert body.count("fail(HGI_EDEVICE") == 1 and body.index("launch_rviews_encode(") < body.index("fail(HGI_EDEVICE")
    # the plan header: the rules of a list in the header's order, nothing allocated before the tile count fits; the judgement:
    # one function, no HIP call, the empty plan first, then the rules in the header's order
    head = open(os.path.join(RVIEWS_DIR, "hgi_rviews_plan.h")).read()
    body = head[head.index("inline RViewsJudged rviews_plan("):head.index("// ---- the launch's judgement")]
    order = [body.index(k) for k in ("return refuse(kRViewsNullEntry", "return refuse(kRViewsSrcPitch", "return refuse(kRViewsGridPitch", "return refuse(kRViewsReconPitch",
                                     "return refuse(kRViewsTiles", "views_aliasing(", "return refuse(kRViewsFits32", "return refuse(kRViewsTail", "memcpy(blob")]
    assert order == sorted(order)
    assert body.index("kRViewsTiles") < body.index("std::vector<ViewRect>") and body.count("std::vector") == 1
    judge = head[head.index("inline RViewsLaunchJudged rviews_judge("):]
    order = [judge.index(k) for k in ("info->count == 0 && rviews_info_consistent", '"info is NULL"', "!rviews_info_consistent(", '"d_plan is NULL"', "16-byte aligned",
                                      '"lut is NULL"', "levels > 31", "interpolator %d unknown", "levels == 0 || levels > 8", "split_levels(", "lut[i] == i")]
    assert order == sorted(order)
    assert max(m.start() for m in re.finditer(r"refuse\(HGI_EINVAL", judge)) < min(m.start() for m in re.finditer(r"refuse\(HGI_EUNSUPPORTED", judge))


# ---------------------------------------------------------------------------------------------------- argument rules
def _calls():
    with open(os.path.join(GOLDEN_DIR, "rviews_refusals.json")) as f:
        return json.load(f)["calls"]


def _plan(triples, keep):
    """hgi_rviews_plan of [[src, grid, recon, w, h, sp, gp, rp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_rviews as F
    n = len(triples)
    arr = (F.RViewTriple * max(n, 1))(*[F.RViewTriple(*t) for t in triples])
    size = F.lib().hgi_rviews_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.RViewsInfo()
    st = F.lib().hgi_rviews_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def replay(call):
    """One recorded call (tests/golden/make_rviews_refusals.py says what the fields mean): (status, error text)."""
    from rustyhgi_amd import _ffi_rviews as F
    L, keep = F.lib(), []
    if call["fn"] == "plan":
        triples = call["triples"]
        n = len(triples) if triples is not None else 1
        arr = (F.RViewTriple * max(n, 1))(*[F.RViewTriple(*t) for t in (triples or [])])
        size = L.hgi_rviews_plan_bytes(n)
        host = np.full(size + 16, 0xEE, np.uint8)
        info = F.RViewsInfo()
        st = L.hgi_rviews_plan(ctypes.addressof(arr) if triples is not None else None, n, host.ctypes.data if call["h_plan"] else None,
                               size if call["plan_bytes"] == "enough" else call["plan_bytes"], ctypes.addressof(info) if call["info"] else None)
        # a refused plan leaves the blob untouched and an info that no launch accepts: all zero
        assert (host == 0xEE).all() and bytes(info) == bytes(ctypes.sizeof(info)), "a refused plan wrote something"
    else:
        info = None
        if call["info"] is not None:
            st0, info, _ = _plan(call["info"], keep)
            assert st0 == 0, F.last_error()
            for k, v in call["damage"].items():
                setattr(info, k, v)
        lut = None if call["lut"] is None else (ctypes.c_uint8 * 256)(*(range(256) if call["lut"] == "identity" else MEDIUM))
        st = L.hgi_rviews_encode_dev(None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["levels"], call["interp"], lut)
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    calls = _calls()
    solo = [c["rule"] for c in calls if c["kind"] == "solo"]
    assert solo == ["null_argument", "plan_bytes", "null_entry", "src_pitch", "grid_pitch", "recon_pitch", "tiles", "out_out", "out_in", "fits32", "tail",
                    "info_null", "info_inconsistent", "d_plan_null", "d_plan_aligned", "lut_null", "levels_range", "interp", "levels"]
    assert sum(c["kind"] == "pair" for c in calls) >= 16
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in calls)      # refused before any device call
    assert set(c["call"]["fn"] for c in calls) == {"plan", "encode"}
    # HGI_EINVAL before HGI_EUNSUPPORTED: in every recorded pair that breaks one rule of each kind, the HGI_EINVAL text is recorded
    status = dict((c["rule"], c["status"]) for c in calls if c["kind"] == "solo")
    unsupported = set(r for r, s in status.items() if s == _ffi.EUNSUPPORTED)
    assert unsupported == {"fits32", "tail", "levels"}
    mixed = [c for c in calls if c["kind"] == "pair" and (c["rule"] in unsupported) != (c["also_breaks"] in unsupported)]
    assert len(mixed) >= 5 and all(c["status"] == _ffi.EINVAL for c in mixed)
    # every aliasing kind is on the list
    notes = set(c["note"] for c in calls if c["rule"] in ("out_out", "out_in"))
    assert {"grid against recon of the same entry", "grid against grid", "recon against recon", "a grid against an input", "in place",
            "the same windows at different pitches", "different pitches"} <= notes


def test_every_recorded_refusal_repeats_its_status_and_text(R):
    calls = _calls()
    for c in calls:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    # the texts name the offending list index, and for an aliasing pair the side of each view
    named = dict((c["rule"], c["error"]) for c in calls if c["kind"] == "solo")
    for rule in ("null_entry", "recon_pitch", "fits32", "tail"):
        assert named[rule].startswith("view 1:"), named[rule]
    for rule in ("src_pitch", "grid_pitch"):
        assert named[rule].startswith("view 0:"), named[rule]
    assert named["out_out"].startswith("the grid of view 0 and the reconstruction of view 1 share bytes")
    assert named["out_in"].startswith("the reconstruction of view 1 shares bytes with the input of view 0")
    extra = dict((c["note"], c["error"]) for c in calls if c["kind"] == "extra")
    assert extra["grid against recon of the same entry"].startswith("the grid of view 1 and the reconstruction of view 1 share")
    assert extra["grid against grid"].startswith("the grid of view 0 and the grid of view 1 share")
    assert extra["recon against recon"].startswith("the reconstruction of view 0 and the reconstruction of view 1 share")
    assert extra["recon of an earlier entry against grid of a later one"].startswith("the reconstruction of view 0 and the grid of view 1 share")
    assert extra["a grid against an input"].startswith("the grid of view 1 shares bytes with the input of view 0")
    assert extra["in place"].startswith("the reconstruction of view 0 shares bytes with the input of view 0")
    assert extra["the same windows at different pitches"].startswith("the grid of view 0 and the reconstruction of view 0: their byte spans meet and their pitches differ")
    assert extra["different pitches"].startswith("the grid of view 1 and the input of view 0: their byte spans meet and their pitches differ")


def test_served_and_empty_plans_without_a_device(R):
    """What is NOT refused, as far as no device is needed: grid and reconstruction windows side by side in one parent's rows,
    inputs overlapping inputs; the blob's first part is the view lists' blob of the (src, grid) pairs byte for byte and the third
    sides stand behind it; and the empty plans, which the launch accepts and does nothing for, whatever the other arguments.  The
    infos of the other view lists are not this library's, and the other way."""
    from rustyhgi_amd import _ffi, _ffi_views
    A, B, C, keep = 1 << 50, 2 << 50, 3 << 50, []
    side_by_side = [[A, B, B + 300, 300, 200, 320, 1536, 1536], [A + 7, B + 900, B + 600, 300, 200, 320, 1536, 1536], [A + (1 << 20), C, C + 64, 64, 1, 0, 0, 0]]
    st, info, host = _plan(side_by_side, keep)
    assert st == _ffi.OK, R.last_error()
    assert info.count == 3 and info.edge_tiles == 13 and info.interior_tiles == 12 and info.max_width == 300 and info.reserved == 0 and info.magic == R.MAGIC
    assert info.recon_offset == 3 * 64 + 2 * 16 and info.plan_bytes == info.recon_offset + 3 * 16 and (host[int(info.plan_bytes):] == 0xEE).all()
    # the first part: hgi_views_plan's blob of the (src, grid) pairs
    pairs = (_ffi_views.ViewPair * 3)(*[_ffi_views.ViewPair(t[0], t[1], t[3], t[4], t[5], t[6]) for t in side_by_side])
    theirs, vinfo = np.zeros(512, np.uint8), _ffi_views.ViewsInfo()
    assert _ffi_views.lib().hgi_views_plan(ctypes.addressof(pairs), 3, theirs.ctypes.data, 512, ctypes.addressof(vinfo)) == _ffi.OK
    assert vinfo.plan_bytes == info.recon_offset and (host[:int(vinfo.plan_bytes)] == theirs[:int(vinfo.plan_bytes)]).all()
    assert (vinfo.count, vinfo.edge_tiles, vinfo.interior_tiles, vinfo.max_width) == (info.count, info.edge_tiles, info.interior_tiles, info.max_width)
    # the third sides: {address, pitch, span}; a one-row frame's pitch counts as its width
    third = host[int(info.recon_offset):int(info.plan_bytes)]
    assert [int(v) for v in third.view(np.uint64)[0::2]] == [B + 300, B + 600, C + 64]      # addresses, no host pointer: the blob is position-independent
    assert [tuple(int(v) for v in third.view(np.uint32)[4 * i + 2:4 * i + 4]) for i in range(3)] == [(1536, 199 * 1536 + 300), (1536, 199 * 1536 + 300), (64, 64)]
    overlapping_inputs = [[A, B, C, 300, 200, 320, 304, 384], [A + 17 * 320 + 5, B + (1 << 30), C + (1 << 30), 300, 200, 320, 304, 384]]
    assert _plan(overlapping_inputs, keep)[0] == _ffi.OK, R.last_error()
    L = R.lib()
    for triples in ([], [[0, 0, 0, 0, 5, 0, 0, 0], [0, 0, 0, 7, 0, 1, 1, 1]]):
        st, info, _ = _plan(triples, keep)
        assert st == _ffi.OK and info.magic == R.MAGIC and info.count == 0 and info.plan_bytes == 0 and info.recon_offset == 0
        for levels, interp, d_plan in ((4, 1, None), (0, 7, 8), (99, -1, None)):
            assert L.hgi_rviews_encode_dev(None, d_plan, ctypes.addressof(info), levels, interp, None) == _ffi.OK
    assert L.hgi_rviews_plan(None, 0, None, 0, None) == _ffi.OK
    # foreign infos, both ways
    from rustyhgi_amd import _ffi_qviews
    lut = (ctypes.c_uint8 * 256)(*MEDIUM)
    st, mine, _ = _plan([[A, B, C, 300, 200, 320, 320, 320]], keep)
    assert st == _ffi.OK
    as_mine = R.RViewsInfo()
    ctypes.memmove(ctypes.addressof(as_mine), ctypes.addressof(vinfo), ctypes.sizeof(vinfo))
    as_mine.recon_offset = vinfo.plan_bytes
    assert L.hgi_rviews_encode_dev(None, 1 << 40, ctypes.addressof(as_mine), 4, 1, lut) == _ffi.EINVAL and "info is not" in R.last_error()
    assert _ffi_views.lib().hgi_views_decode_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1) == _ffi.EINVAL
    assert _ffi_views.lib().hgi_views_encode_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1, lut) == _ffi.EINVAL
    assert _ffi_qviews.lib().hgi_qviews_requant_dev(None, 1 << 40, ctypes.addressof(mine), 4, 1, lut) == _ffi.EINVAL


# ------------------------------------------------------------------------------------------------------ kernel unit
def _listing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    path = str(tmp_path / UNIT.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(RVIEWS_DIR, UNIT), "-o", path],
                          stderr=subprocess.DEVNULL)
    return path


def _metadata(text, kernel):
    """{template arguments: (VGPRs, spilled VGPRs, scratch bytes, static LDS bytes, SGPRs)} of the kernels named `kernel`, from
    the listing's metadata."""
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_count:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                         text, flags=re.S):
        k = re.search(r"\d+%sILi(\d)ELb(\d)ELi(\d)E" % kernel, m.group(2))
        if k:
            res[tuple(int(v) for v in k.groups())] = (int(m.group(5)), int(m.group(6)), int(m.group(3)), int(m.group(1)), int(m.group(4)))
    return res


def waves_by_registers(vgprs):
    """Waves per SIMD that a VGPR count allows: 512 VGPRs per SIMD, allocated in granules of 8."""
    return 512 // (-(-vgprs // 8) * 8)


@pytest.mark.timeout(900)
def test_unit_compiles_without_spills_and_passes_check_isa(tmp_path):
    """k_enc_recon_views<interp, ident, unseeded | cone>, eight kernels: the hazard rules of tools/check_isa.py, no scratch, no
    spills, no DPP, no traps, no static LDS.  The listing also holds the eight k_enc_recon of the included recon unit, which
    nothing launches.  The frame search is scalar: the prefix arrays, the record and the third side are read with s_load."""
    import check_isa
    path = _listing(tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == 16, r
    assert r["partial_writes"] > 1000, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_enc_recon_views\w*):", text))) == 8
    assert not re.search(r"k_(dec|enc)_(tiles|pitched|list|views)\b", text)
    mine, model = _metadata(text, "k_enc_recon_views"), _metadata(text, "k_enc_recon")
    assert len(mine) == len(model) == 8 and set(mine) == set(model) == set((i, d, s) for i in (0, 1) for d in (0, 1) for s in (0, 2))
    for key, (vgprs, spills, scratch, lds, _) in sorted(mine.items()):
        assert spills == 0 and scratch == 0 and lds == 0, (key, spills, scratch, lds)
        assert vgprs <= 512 // (4 if key[1] else 5) // 8 * 8, (key, vgprs)      # the budget of amdgpu_waves_per_eu: five waves, four for the identity
    bodies = re.findall(r"^_Z\w*k_enc_recon_views\w*:.*?^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(bodies) == 8
    for body in bodies:
        assert "s_load_dwordx4" in body and "v_mov_b32_dpp" not in body and "scratch_" not in body
        assert len(re.findall(r"\bbuffer_store_dwordx[24]\b", body)) > 0


@pytest.mark.timeout(900)
def test_unit_allows_k_enc_recons_waves_per_simd(tmp_path):
    """Every k_enc_recon_views instantiation has a VGPR count that allows the same waves per SIMD as the k_enc_recon instantiation
    of the same template arguments, both read from the metadata of one listing (512 VGPRs per SIMD, granule 8).

    Figures of this tree (-O3, gfx950), k_enc_recon_views / k_enc_recon, <INTERP, IDENT, SEEDED>, one for one:
    <0, 0, 0> 66 / 66, <0, 1, 0> 64 / 64, <1, 0, 0> 74 / 74, <1, 1, 0> 69 / 69, <0, 0, 2> 74 / 74, <0, 1, 2> 72 / 72, <1, 0, 2> 75 / 75,
    <1, 1, 2> 73 / 73.  With list_find's loop in the context function the four cone kernels took three more each (77, 75, 78, 76):
    any cycle in front of the tile body, even an empty one, keeps the ragged staging's four odd-row indices live down to the
    finest pass, where k_enc_recon's code forms three of them again; <0, 1, 2> at 75 then allowed 6 waves by count where 72 allow
    7.  rview_find is the same search without a cycle."""
    text = open(_listing(tmp_path)).read()
    mine, model = _metadata(text, "k_enc_recon_views"), _metadata(text, "k_enc_recon")
    assert len(mine) == len(model) == 8
    for key in sorted(mine):
        print("k_enc_recon_views<%d, %d, %d>: %d VGPRs %d SGPRs, k_enc_recon: %d VGPRs %d SGPRs" % (key + (mine[key][0], mine[key][4], model[key][0], model[key][4])))
    fewer = dict((key, (mine[key][0], model[key][0])) for key in mine if waves_by_registers(mine[key][0]) != waves_by_registers(model[key][0]))
    assert not fewer, fewer


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_program_under_asan_ubsan(tmp_path):
    """tests/cpp/test_rviews_plan.cpp, a stand-alone program: random lists whose blob starts with views_plan's blob and ends with
    extra_side's third sides, aliasing against marked bytes with the pair named by index and side, every aliasing kind by hand,
    every rule alone and in pairs, the judgement with the sibling magics refused (see the file's head)."""
    CL.run_plan_program("rviews", tmp_path, flags=("-Werror",))


# ----------------------------------------------------------------------------------------------------------- Python
def test_recon_view_plan_refuses_bad_layouts_before_any_device_call(R):
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import ReconViewPlan
    t = torch.zeros((64, 160), dtype=torch.uint8)
    g = torch.zeros((64, 160), dtype=torch.uint8)
    r = torch.zeros((64, 160), dtype=torch.uint8)
    bad = (t[:, ::2], t[:, :159], t[:63], t.to(torch.float16), t.reshape(-1), np.zeros((64, 160), np.uint8), t.t(), t.to(torch.float32))
    for side in range(3):
        for b in bad:
            triple = [t, g, r]
            triple[side] = b
            with pytest.raises(ValueError, match="triple 0"):
                ReconViewPlan([tuple(triple)])
    with pytest.raises(ValueError, match="triple 1: the reconstruction has shape"):
        ReconViewPlan([(t, g, r), (t, g, r[:, :159])])
    with pytest.raises(ValueError, match="triple 0: the grid has shape"):
        ReconViewPlan([(t, g[:63], r)])
    # a valid layout passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        ReconViewPlan([(t, g, r)])
    with pytest.raises(ValueError, match="GPU"):
        ReconViewPlan([(t[:63, :159], g[:63, :159], r[:63, :159])])
    p = ReconViewPlan([])
    assert len(p) == 0 and p.fused and p.reason == "" and p.blob is None and p.info.count == 0 and p.layouts == [] and p.info.magic == R.MAGIC


def test_encode_views_with_reconstruction_serves_empty_plans_without_a_device(R):
    torch = pytest.importorskip("torch")
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    assert enc.encode_views_with_reconstruction(H.ReconViewPlan([])) == ([], [])
    e = [tuple(torch.zeros(s, dtype=torch.uint8) for _ in range(3)) for s in ((0, 9), (5, 0))]

    class _Plan:      # what a plan of empty CUDA views looks like, without a device
        srcs, grids, recons, layouts, fused, blob = [a for a, _, _ in e], [b for _, b, _ in e], [c for _, _, c in e], [(0, 0, 0, 9, 0, 9, 9, 9), (0, 0, 0, 0, 5, 0, 0, 0)], True, None
        device = None

        def __len__(self):
            return 2

    grids, recons = enc.encode_views_with_reconstruction(_Plan())
    assert [tuple(o.shape) for o in grids] == [tuple(o.shape) for o in recons] == [(0, 9), (5, 0)]


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("rviews", after="sviews")
    import rustyhgi_amd
    assert {"rviews", "ReconViewPlan"} <= set(rustyhgi_amd.__all__)
    assert hasattr(rustyhgi_amd.Encoder, "encode_views_with_reconstruction") and "encode_views_with_reconstruction" in rustyhgi_amd.__doc__
    from rustyhgi_amd import _ffi_rviews
    assert _ffi_rviews.LIB_PATH.endswith("libhgi_rviews.so")
