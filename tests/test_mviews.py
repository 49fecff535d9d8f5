"""CPU suite of the mapped view lists (libhgi_mviews.so, include/hgi_mviews.h, rustyhgi_amd.mviews): the companion library exports
its five entry points and nothing else, names no tuning switch, reads no environment and links nothing of libhgi_hip.so; the
ctypes table and the two structures match the header; the plan entry makes no HIP call and the launch entry decides its rules
before the first one; the refusals recorded in tests/golden/mviews_refusals.json repeat their status and text without a device;
the kernel unit compiles for gfx950 within the mapped decoder's budgets and passes tools/check_isa.py; the host plan -- record
geometry with the written side in bytes, aliasing with E-byte elements, boundaries, the output interval -- holds under ASan /
UBSan (tests/cpp/test_mviews_plan.cpp, a stand-alone program); padded_batch and MappedViewPlan refuse bad layouts before any
device call."""
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

MVIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "mviews")
NAMES = ("hgi_mviews_plan_bytes", "hgi_mviews_plan", "hgi_mviews_decode_dev", "hgi_mviews_last_error", "hgi_mviews_version")
FILES = ["Makefile", "hgi_fused_mviews_dec.hip", "hgi_mviews.hip", "hgi_mviews.map", "hgi_mviews_kernels.h", "hgi_mviews_plan.h"]
UNIT = "hgi_fused_mviews_dec.hip"


@pytest.fixture(scope="module")
def M():
    return CL.binding("mviews")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_five_entry_points(M):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", M.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(MVIEWS_DIR, "hgi_mviews.map")).read()
    assert re.search(r"global:\s*hgi_mviews_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", CL.header("mviews")))
    assert declared == set(NAMES) == set(s[0] for s in M.SYMBOLS)
    version = M.lib().hgi_mviews_version()
    assert version.startswith(b"hgi_mviews 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, M.LIB_PATH], text=True)) == []
    CL.check_sources(MVIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", M.LIB_PATH], text=True)
    # the Makefile: the fragment the sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(MVIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert len(code) == 4 and code[:2] == ["NAME := mviews", "FUSED := hgi_fused_dec.hip"] and code[3] == "include ../companion/companion.mk", code
    assert code[2].startswith("ALSO := ") and "CXXFLAGS" not in mk
    also = code[2].split()[2:]
    assert all(os.path.isfile(os.path.join(MVIEWS_DIR, f)) for f in also), also
    # ... every file of the two sibling directories that the unit includes, directly or through them, is a dependency
    src = open(os.path.join(MVIEWS_DIR, UNIT)).read()
    assert {"../map/hgi_fused_map_dec.hip", "../map/hgi_map_kernels.h", "../map/hgi_map_plan.h", "../views/hgi_views_tile.h",
            "../views/hgi_views_kernels.h", "../views/hgi_views_plan.h", "../csrc/hgi_framelist.h"} <= set(also)
    # the unit: the mapped unit as it stands (which brings the decode direction's unit without its launchers, the pitched
    # staging and the shared tile layer, in that order), the view lists' frame search behind it, the launch through the launch layer
    assert src.index('#include "../map/hgi_fused_map_dec.hip"') < src.index('#include "../views/hgi_views_tile.h"') < src.index('#include "hgi_mviews_kernels.h"')
    assert "#define" not in src
    mapped = open(os.path.join(ROOT, "rustyhgi_amd", "map", "hgi_fused_map_dec.hip")).read()
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in mapped and '#include "../csrc/hgi_fused_dec.hip"' in mapped
    assert mapped.index('"../csrc/hgi_fused_pitched.h"') < mapped.index('"../companion/hgi_tile.h"')
    assert "launch_tile_kernel<k_dec_mviews<" in src and "with_choices(" in src and "hipLaunchKernelGGL" not in src
    assert "view_ctx(a)" in src and "map_waves_per_eu(SEEDED, E)" in src and "kMapStageBytes" in src and "dec_resident_tiles(" in src
    assert src.count("dec_tile_map<INTERP, E, ") == 3
    # every store of the unit is the mapped finest pass's: none of its own
    assert "buffer_store" not in src and "store_rows" not in src and "store_row_pair" not in src
    plan = open(os.path.join(MVIEWS_DIR, "hgi_mviews_plan.h")).read()
    assert '#include "../views/hgi_views_plan.h"' in plan and "struct ViewFrame" not in plan and not re.search(r"\bhip[A-Z_]\w*", plan)


def test_ctypes_table_and_structures_match_the_header(M):
    head = CL.header("mviews")
    for name, fields in (("hgi_mview_pair", M.MViewPair), ("hgi_mviews_info", M.MViewsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), head, flags=re.S).group(1)
        declared = []
        for stmt in body.split(";"):
            m = re.match(r"\s*(uint32_t|uint64_t)\s+(.*)$", stmt.strip(), flags=re.S)
            if m:
                declared += [(n.strip(), ctypes.c_uint32 if m.group(1) == "uint32_t" else ctypes.c_uint64) for n in m.group(2).split(",")]
        assert declared == [(n, t) for n, t in fields._fields_], (name, declared)
    assert ctypes.sizeof(M.MViewPair) == 40 and ctypes.sizeof(M.MViewsInfo) == 72
    # hgi_views_info's layout with the element size in its reserved slot and the output interval behind it
    from rustyhgi_amd import _ffi_views
    theirs, mine = _ffi_views.ViewsInfo._fields_, M.MViewsInfo._fields_
    assert [(n if n != "reserved" else "elem_size", t) for n, t in theirs] == mine[:len(theirs)] and [n for n, _ in mine[len(theirs):]] == ["dst_lo", "dst_hi"]
    assert [(n, getattr(M.MViewPair, n).offset) for n, _ in M.MViewPair._fields_] == [(n, getattr(_ffi_views.ViewPair, n).offset) for n, _ in _ffi_views.ViewPair._fields_]
    magic = int(re.search(r"#define HGI_MVIEWS_MAGIC (0x[0-9a-fA-F]+)u", head).group(1), 16)
    assert magic == M.MAGIC and magic != _ffi_views.MAGIC
    table = dict((s[0], s) for s in M.SYMBOLS)
    from rustyhgi_amd import _ffi
    want = {"hgi_mviews_plan_bytes": (_ffi._sz, [_ffi._sz]),
            "hgi_mviews_plan": (_ffi._int, [_ffi._vp, _ffi._sz, _ffi._u32, _ffi._vp, _ffi._sz, _ffi._vp]),
            "hgi_mviews_decode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int, _ffi._vp]),
            "hgi_mviews_last_error": (ctypes.c_char_p, []), "hgi_mviews_version": (ctypes.c_char_p, [])}
    assert set(want) == set(table)
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_mviews.h")).read()
    L = M.lib()
    assert [L.hgi_mviews_plan_bytes(n) for n in (0, 1, 4, 5)] == [0, 96, 288, 384]


def test_the_plan_makes_no_hip_call_and_the_launch_judges_first():
    """hgi_mviews.hip: nothing of HIP in the plan entry; in the launch entry the judge -- which holds every refusal, the
    HGI_EINVAL ones in front of the HGI_EUNSUPPORTED one, and no HIP call -- stands in front of the launch, and no refusal but the
    HGI_EDEVICE one behind it."""
    src = open(os.path.join(MVIEWS_DIR, "hgi_mviews.hip")).read()
    hip = r"\bhip[A-Z]\w*\s*\(|launch_mviews_\w+\s*\("
    plan = src[src.index("hgi_status hgi_mviews_plan("):src.index("hgi_status hgi_mviews_decode_dev(")]
    assert not re.search(hip, plan)
    assert plan[plan.rindex("return fail("):].count('"unknown verdict"') == 1      # (the default of the verdict switch: never reached)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", plan[:plan.rindex("return fail(")])) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", plan))
    judge = src[src.index("hgi_status judge_launch("):src.index("bool empty_plan(")]
    assert not re.search(hip, judge)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", judge)) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", judge))
    order = [judge.index(k) for k in ('"info is NULL"', "mviews_info_consistent(", '"d_plan is NULL"', "16-byte aligned", '"d_table is NULL"', "meet(ti, oi)",
                                      "levels > 31", "interpolator %d unknown", "levels == 0 || levels > 8")]
    assert order == sorted(order)
    body = src[src.index("hgi_status hgi_mviews_decode_dev("):src.index("const char *hgi_mviews_last_error")]
    first = min(m.start() for m in re.finditer(hip, body))
    assert body[first:].startswith("launch_mviews_decode(") and body.index("judge_launch(") < first
    assert "fail(HGI_EINVAL" not in body and "fail(HGI_EUNSUPPORTED" not in body and body.count("fail(HGI_EDEVICE") == 1
    assert body.index("return HGI_OK;") < body.index("judge_launch(")      # the empty plan is decided first
    # the entry judges its own arguments in front of the list; the plan header judges in the header's order: per entry the NULL
    # side, the grid pitch, the three element rules; then tiles, aliasing; then the 32-bit bound and the page rule
    order = [plan.index(k) for k in ("NULL argument", "plan_bytes %zu <", "elem_size %u: table elements", "mviews_plan(views")]
    assert order == sorted(order)
    head = open(os.path.join(MVIEWS_DIR, "hgi_mviews_plan.h")).read()
    body = head[head.index("inline MViewsJudged mviews_plan("):]
    order = [body.index(k) for k in ("kMViewsNullEntry", "kMViewsSrcPitch", "kMViewsDstAlign", "kMViewsDstPitchAlign", "kMViewsDstPitch", "kMViewsTiles",
                                     "mviews_aliasing(", "kMViewsFits32", "kMViewsTail", "memcpy(blob")]
    assert order == sorted(order)
    assert body.index("kMViewsTiles") < body.index("std::vector<MViewRect>")      # nothing is allocated before the tile count fits


# ---------------------------------------------------------------------------------------------------- argument rules
def _calls():
    with open(os.path.join(GOLDEN_DIR, "mviews_refusals.json")) as f:
        return json.load(f)["calls"]


def _plan(views, elem, keep):
    """hgi_mviews_plan of [[src, dst, w, h, sp, dp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_mviews as F
    n = len(views)
    arr = (F.MViewPair * max(n, 1))(*[F.MViewPair(*v) for v in views])
    size = F.lib().hgi_mviews_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.MViewsInfo()
    st = F.lib().hgi_mviews_plan(ctypes.addressof(arr), n, elem, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def replay(call):
    """One recorded call (tests/golden/make_mviews_refusals.py says what the fields mean): (status, error text)."""
    from rustyhgi_amd import _ffi_mviews as F
    L, keep = F.lib(), []
    if call["fn"] == "plan":
        views = call["views"]
        n = len(views) if views is not None else 1
        arr = (F.MViewPair * max(n, 1))(*[F.MViewPair(*v) for v in (views or [])])
        size = L.hgi_mviews_plan_bytes(n)
        host = np.full(size + 16, 0xEE, np.uint8)
        info = F.MViewsInfo()
        st = L.hgi_mviews_plan(ctypes.addressof(arr) if views is not None else None, n, call["elem"], host.ctypes.data if call["h_plan"] else None,
                               size if call["plan_bytes"] == "enough" else call["plan_bytes"], ctypes.addressof(info) if call["info"] else None)
        # a refused plan leaves the blob untouched and an info that no launch accepts: as it was handed in, all zero
        assert (host == 0xEE).all() and bytes(info) == bytes(ctypes.sizeof(info)), "a refused plan wrote something"
    else:
        info = None
        if call["info"] is not None:
            st0, info, _ = _plan(call["info"], call["elem"], keep)
            assert st0 == 0, F.last_error()
            for k, v in call["damage"].items():
                setattr(info, k, v)
        st = L.hgi_mviews_decode_dev(None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["levels"], call["interp"], call["table"])
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    calls = _calls()
    solo = [c["rule"] for c in calls if c["kind"] == "solo"]
    assert solo == ["null_argument", "plan_bytes", "elem_size", "null_entry", "src_pitch", "dst_align", "dst_pitch_align", "dst_pitch", "tiles", "out_out",
                    "out_in", "fits32", "tail", "info_null", "info_inconsistent", "d_plan_null", "d_plan_aligned", "table_null", "table_alias",
                    "levels_range", "interp", "levels_launch"]
    assert sum(c["kind"] == "pair" for c in calls) >= 17
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in calls)      # refused before any device call
    assert set(c["call"]["fn"] for c in calls) == {"plan", "decode"}
    # HGI_EINVAL before HGI_EUNSUPPORTED: in every recorded pair that breaks one rule of each kind, the HGI_EINVAL text is recorded
    status = dict((c["rule"], c["status"]) for c in calls if c["kind"] == "solo")
    unsupported = set(r for r, s in status.items() if s == _ffi.EUNSUPPORTED)
    assert unsupported == {"fits32", "tail", "levels_launch"}
    mixed = [c for c in calls if c["kind"] == "pair" and (c["rule"] in unsupported) != (c["also_breaks"] in unsupported)]
    assert len(mixed) >= 2 and all(c["status"] == _ffi.EINVAL for c in mixed)


def test_every_recorded_refusal_repeats_its_status_and_text(M):
    calls = _calls()
    for c in calls:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    # the texts name the offending list index
    named = dict((c["rule"], c["error"]) for c in calls if c["kind"] == "solo")
    for rule in ("null_entry", "dst_align", "tail"):
        assert named[rule].startswith("view 1:"), named[rule]
    for rule in ("src_pitch", "dst_pitch_align", "dst_pitch", "fits32"):
        assert named[rule].startswith("view 0:"), named[rule]
    assert "views 0 and 1" in named["out_out"] and "output of view 1" in named["out_in"] and "input of view 0" in named["out_in"]


def test_served_and_empty_plans_without_a_device(M):
    """What is NOT refused, as far as no device is needed: float windows side by side in one parent's rows, grids overlapping
    grids, a one-row view beside a window, a grid in the gap of an output's pitch; the record's written side in bytes and the
    output interval; and the empty plans, which the launch accepts and does nothing for, whatever the other arguments."""
    from rustyhgi_amd import _ffi
    A, B, keep = 1 << 50, 2 << 50, []
    for E in (2, 4):
        side_by_side = [[A, B, 32, 8, 40, 64 * E], [A + 4096, B + 32 * E, 32, 8, 40, 64 * E], [A + 8192, B + 8 * 64 * E, 64, 1, 0, 0]]
        st, info, host = _plan(side_by_side, E, keep)
        assert st == _ffi.OK, M.last_error()
        assert info.count == 3 and info.edge_tiles == 3 and info.interior_tiles == 0 and info.max_width == 64 and info.elem_size == E
        assert info.plan_bytes == 3 * 64 + 2 * 16 and (host[int(info.plan_bytes):] == 0xEE).all()
        assert (info.dst_lo, info.dst_hi) == (B, B + 8 * 64 * E + 64 * E)
        rec = host[:64].view(np.uint64)
        assert int(rec[0]) == A and int(rec[1]) == B      # addresses and sizes, no host pointer: the blob is position-independent
        words = host[:64].view(np.uint32)
        assert list(words[4:6]) == [32, 8] and list(words[8:12]) == [40, 64 * E, 7 * 40 + 32, 7 * 64 * E + 32 * E]      # sp32, dp32, srec, drec
        one_row = host[128:192].view(np.uint32)
        assert list(one_row[8:12]) == [64, 64 * E, 64, 64 * E]      # a one-row frame's pitch counts as its row, in bytes on the written side
        crops = [[A, B, 32, 8, 40, 32 * E], [A + 5, B + 4096, 32, 8, 40, 32 * E], [A, B + 8192, 32, 8, 40, 32 * E]]
        assert _plan(crops, E, keep)[0] == _ffi.OK
        in_the_gap = [[A, B, 32, 8, 40, 64 * E], [B + 32 * E, A + 4096, 8, 8, 64 * E, 8 * E]]
        assert _plan(in_the_gap, E, keep)[0] == _ffi.OK, M.last_error()
    L = M.lib()
    for views in ([], [[0, 0, 0, 5, 0, 0], [0, 0, 7, 0, 1, 1]]):
        st, info, _ = _plan(views, 4, keep)
        assert st == _ffi.OK and info.magic == M.MAGIC and info.count == 0 and info.plan_bytes == 0 and (info.dst_lo, info.dst_hi) == (0, 0)
        for levels, interp, d_plan, table in ((4, 1, None, None), (0, 7, 8, 1), (99, -1, None, None)):
            assert L.hgi_mviews_decode_dev(None, d_plan, ctypes.addressof(info), levels, interp, table) == _ffi.OK
    assert L.hgi_mviews_plan(None, 0, 0, None, 0, None) == _ffi.OK
    # the view lists' info is not this library's
    from rustyhgi_amd import _ffi_views
    theirs = _ffi_views.ViewsInfo()
    assert _ffi_views.lib().hgi_views_plan(None, 0, None, 0, ctypes.addressof(theirs)) == _ffi.OK
    mine = M.MViewsInfo()
    ctypes.memmove(ctypes.addressof(mine), ctypes.addressof(theirs), ctypes.sizeof(theirs))
    assert L.hgi_mviews_decode_dev(None, None, ctypes.addressof(mine), 4, 1, None) == _ffi.EINVAL


# ------------------------------------------------------------------------------------------------------ kernel unit
@pytest.mark.timeout(900)
def test_unit_is_within_the_mapped_decoders_budgets(tmp_path):
    """k_dec_mviews<interp, unseeded | cone, E = 2 | 4>, eight kernels: the hazard rules of tools/check_isa.py (rule 4 covers the
    row stores: they go through store_map_rows), no scratch, no spills, no DPP, no traps, no static LDS, and k_dec_map's
    occupancy: E = 4 within 64 VGPRs (eight waves per SIMD), E = 2 within 72 (seven), the cone within 68 / 72.  The frame search
    is scalar: the prefix arrays and the record are read with s_load; whole 16-byte pieces are stored non-temporally.  The
    listing also holds the eight k_dec_map kernels of the included mapped unit, which nothing launches: within the same budgets."""
    import check_isa
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    path = str(tmp_path / UNIT.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(MVIEWS_DIR, UNIT), "-o", path],
                          stderr=subprocess.DEVNULL)
    r = check_isa.check(path)
    assert r["kernels"] == 16, r
    assert r["partial_writes"] > 100, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*k_dec_mviews\w*):", text))) == 8
    assert not re.search(r"k_(dec|enc)_(tiles|pitched|list|views)", text)
    for name in ("k_dec_mviews", "k_dec_map"):
        res = CL.resources(text, name)
        assert len(res) == 8, res
        for k, (vgprs, lds, scratch) in res.items():
            assert lds == 0 and scratch == 0, (k, lds, scratch)
            e2, cone = "ELi2EEE" in k, "ELi2ELi" in k
            assert ("ELi4EEE" in k) != e2 and ("ELi0ELi" in k) != cone, k
            assert vgprs <= (72 if e2 else 68 if cone else 64), (k, vgprs)
    # the kernels of this unit alone: scalar loads of the record, non-temporal 16-byte stores
    bodies = re.findall(r"^_Z\w*k_dec_mviews\w*:.*?^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(bodies) == 8
    for body in bodies:
        assert "k_dec_map" not in body and "s_load_dwordx4" in body and re.search(r"buffer_store_dwordx4 .* nt", body)


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_program_under_asan_ubsan(tmp_path):
    """tests/cpp/test_mviews_plan.cpp, a stand-alone program: the records of 100 000 random small lists against pitched_plan with
    the byte-wide write side, the aliasing test against bytes, the boundary rules on both sides, the output interval (see the
    file's head)."""
    exe = str(tmp_path / "test_mviews_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_mviews_plan.cpp"), "-o", exe])
    p = subprocess.run([exe, "100000", "0x48474941"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "100000 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ----------------------------------------------------------------------------------------------------------- Python
def test_padded_batch_refuses_before_any_device_call():
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import padded_batch
    for dtype in (torch.uint8, torch.float64, np.float16, "float16"):
        with pytest.raises(ValueError, match="dtype"):
            padded_batch([(2, 2)], dtype)
    for bad in (0, 3, 100, -128, 1):
        with pytest.raises(ValueError, match="align"):
            padded_batch([(2, 2)], torch.float16, bad)
    with pytest.raises(ValueError, match="align"):
        padded_batch([(2, 2)], torch.float32, 2)
    for shapes in ([(-1, 2)], [(2, 2, 2)], [(3,)]):
        with pytest.raises(ValueError, match="shape"):
            padded_batch(shapes, torch.float32)
    # the layout, on the host: [N, Hmax, Wp] with Wp * E a multiple of `align`; empty frames take a slot and give an empty view
    shapes = [(65, 129), (0, 900), (3, 130), (1, 1), (700, 0)]
    for dtype, e in ((torch.float16, 2), (torch.bfloat16, 2), (torch.float32, 4)):
        for align in (128, 16, 4, 512):
            batch, views = padded_batch(shapes, dtype, align, device="cpu", fill=-1.0)
            wp = batch.shape[2]
            assert tuple(batch.shape[:2]) == (5, 65) and wp * e % align == 0 and 130 <= wp < 130 + max(align // e, 1) and batch.dtype == dtype
            assert [tuple(v.shape) for v in views] == shapes and all(v.dtype == dtype for v in views)
            for i, (v, (h, w)) in enumerate(zip(views, shapes)):
                if h and w:
                    assert v.data_ptr() == batch[i].data_ptr() and v.stride() == (wp, 1) and (v.data_ptr() - batch.data_ptr()) % align == 0
            assert (batch == -1.0).all()
    batch, views = padded_batch([], torch.float32, device="cpu")
    assert tuple(batch.shape) == (0, 0, 0) and views == []


def test_mapped_view_plan_refuses_bad_layouts_before_any_device_call(M):
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import MappedViewPlan
    t = torch.zeros((64, 160), dtype=torch.uint8)
    o = torch.zeros((64, 160), dtype=torch.float16)
    v = t[8:40, 16:100]
    for src, dst in ((t[:, ::2], o[:, :80]), (v, o[8:40, 16:99]), (t.to(torch.float16), o), (t.reshape(-1), o.reshape(-1)), (np.zeros((4, 4), np.uint8), o[:4, :4]),
                     (t.t(), o.t()), (t, o.to(torch.float32)), (t, o.to(torch.bfloat16)), (t, t), (t[:, :80], o[:, ::2]), (t, np.zeros((64, 160), np.float16))):
        with pytest.raises(ValueError, match="pair 0"):
            MappedViewPlan([(src, dst)], torch.float16)
    with pytest.raises(ValueError, match="pair 1"):
        MappedViewPlan([(v, o[8:40, 16:100]), (t[:, ::2], o[:, :80])], torch.float16)
    for dtype in (torch.uint8, torch.float64, np.float32):
        with pytest.raises(ValueError, match="dtype"):
            MappedViewPlan([(v, o[8:40, 16:100])], dtype)
    # a valid layout passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        MappedViewPlan([(v, o[8:40, 16:100])], torch.float16)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        p = MappedViewPlan([], dtype)
        assert len(p) == 0 and p.fused and p.blob is None and p.info.count == 0 and p.elem_size == (4 if dtype == torch.float32 else 2)


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("mviews", after="views")
    import rustyhgi_amd
    assert {"mviews", "MappedViewPlan", "padded_batch"} <= set(rustyhgi_amd.__all__)
    assert hasattr(rustyhgi_amd.Decoder, "decode_mapped_views")
