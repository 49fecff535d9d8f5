"""CPU suite of the view lists (libhgi_views.so, include/hgi_views.h, rustyhgi_amd.views): the companion library exports its six
entry points and nothing else, names no tuning switch, reads no environment and links nothing of libhgi_hip.so; the ctypes table
and the two structures match the header; the plan entry makes no HIP call and the launch entries decide their rules before the
first one; the refusals recorded in tests/golden/views_refusals.json repeat their status and text without a device; the two kernel
units compile for gfx950 within the pitched kernels' budgets and pass tools/check_isa.py; the host plan -- block map, geometry,
aliasing, boundaries -- holds under ASan / UBSan (tests/cpp/test_views_plan.cpp, a stand-alone program); aligned_arena places
frames disjoint and aligned; ViewPlan refuses bad layouts before any device call."""
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

VIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "views")
NAMES = ("hgi_views_plan_bytes", "hgi_views_plan", "hgi_views_encode_dev", "hgi_views_decode_dev", "hgi_views_last_error", "hgi_views_version")
FILES = ["Makefile", "hgi_fused_views_dec.hip", "hgi_fused_views_enc.hip", "hgi_views.hip", "hgi_views.map", "hgi_views_kernels.h",
         "hgi_views_plan.h", "hgi_views_tile.h"]


@pytest.fixture(scope="module")
def V():
    return CL.binding("views")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_six_entry_points(V):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(VIEWS_DIR, "hgi_views.map")).read()
    assert re.search(r"global:\s*hgi_views_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_\w+)\s*\(", CL.header("views")))
    assert declared == set(NAMES) == set(s[0] for s in V.SYMBOLS)
    version = V.lib().hgi_views_version()
    assert version.startswith(b"hgi_views 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, V.LIB_PATH], text=True)) == []
    CL.check_sources(VIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    assert "libhgi_hip" not in subprocess.check_output([readelf, "-d", V.LIB_PATH], text=True)
    # the Makefile: the fragment the four sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(VIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert code == ["NAME := views", "FUSED := hgi_fused_dec.hip", "ALSO := ../csrc/hgi_fused_enc.hip ../csrc/hgi_framelist.h hgi_views_tile.h",
                    "include ../companion/companion.mk"], code
    shared = open(os.path.join(CL.COMPANION_DIR, "companion.mk")).read()
    assert "CXXFLAGS" not in mk and "$(ALSO)" in shared and re.search(r"^ALSO \?=\s*$", shared, flags=re.M)
    rule = [l for l in shared.splitlines() if l.startswith("$(OBJ)/%.o:")]
    assert len(rule) == 1 and rule[0].endswith("$(ALSO)") and "$(ALSO)" not in shared.replace(rule[0], "").replace("ALSO ?=", "")
    for unit, fused in (("hgi_fused_views_dec.hip", "hgi_fused_dec.hip"), ("hgi_fused_views_enc.hip", "hgi_fused_enc.hip")):
        src = open(os.path.join(VIEWS_DIR, unit)).read()
        assert "#define HGI_FUSED_NO_LAUNCHERS 1" in src and '#include "../csrc/%s"' % fused in src
        assert src.index('"../csrc/hgi_fused_pitched.h"') < src.index('"../companion/hgi_tile.h"') < src.index('"hgi_views_tile.h"')
        assert "launch_tile_kernel<" in src and "with_choices(" in src and "hipLaunchKernelGGL" not in src
    assert "enc_lds_bytes(t.nh)" in open(os.path.join(VIEWS_DIR, "hgi_fused_views_enc.hip")).read()
    plan = open(os.path.join(VIEWS_DIR, "hgi_views_plan.h")).read()
    assert "static_assert(sizeof(ViewFrame) == 64" in plan and not re.search(r"\bhip[A-Z_]\w*", plan)


def test_ctypes_table_and_structures_match_the_header(V):
    head = CL.header("views")
    for name, fields in (("hgi_view_pair", V.ViewPair), ("hgi_views_info", V.ViewsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), head, flags=re.S).group(1)
        declared = []
        for stmt in body.split(";"):
            m = re.match(r"\s*(uint32_t|uint64_t)\s+(.*)$", stmt.strip(), flags=re.S)
            if m:
                declared += [(n.strip(), ctypes.c_uint32 if m.group(1) == "uint32_t" else ctypes.c_uint64) for n in m.group(2).split(",")]
        assert declared == [(n, t) for n, t in fields._fields_], (name, declared)
    assert ctypes.sizeof(V.ViewPair) == 40 and ctypes.sizeof(V.ViewsInfo) == 56
    assert int(re.search(r"#define HGI_VIEWS_MAGIC (0x[0-9a-fA-F]+)u", head).group(1), 16) == V.MAGIC
    table = dict((s[0], s) for s in V.SYMBOLS)
    from rustyhgi_amd import _ffi
    want = {"hgi_views_plan_bytes": (_ffi._sz, [_ffi._sz]),
            "hgi_views_plan": (_ffi._int, [_ffi._vp, _ffi._sz, _ffi._vp, _ffi._sz, _ffi._vp]),
            "hgi_views_encode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int, _ffi._vp]),
            "hgi_views_decode_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int]),
            "hgi_views_last_error": (ctypes.c_char_p, []), "hgi_views_version": (ctypes.c_char_p, [])}
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    assert '#include "hgi.h"' in open(os.path.join(ROOT, "include", "hgi_views.h")).read()
    L = V.lib()
    assert [L.hgi_views_plan_bytes(n) for n in (0, 1, 4, 5)] == [0, 96, 288, 384]


def test_the_plan_makes_no_hip_call_and_the_launches_judge_first():
    """hgi_views.hip: nothing of HIP in the plan entry; in each launch entry the shared judge -- which holds every refusal, the
    HGI_EINVAL ones in front of the HGI_EUNSUPPORTED one, and no HIP call -- stands in front of the launch, and no refusal but
    the HGI_EDEVICE one behind it."""
    src = open(os.path.join(VIEWS_DIR, "hgi_views.hip")).read()
    hip = r"\bhip[A-Z]\w*\s*\(|launch_views_\w+\s*\("
    plan = src[src.index("hgi_status hgi_views_plan("):src.index("hgi_status hgi_views_encode_dev(")]
    assert not re.search(hip, plan)
    assert plan[plan.rindex("return fail("):].count('"unknown verdict"') == 1      # (the default of the verdict switch: never reached)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", plan[:plan.rindex("return fail(")])) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", plan))
    judge = src[src.index("hgi_status judge_launch("):src.index("bool empty_plan(")]
    assert not re.search(hip, judge)
    assert max(m.start() for m in re.finditer(r"fail\(HGI_EINVAL", judge)) < min(m.start() for m in re.finditer(r"fail\(HGI_EUNSUPPORTED", judge))
    for entry, launcher, end in (("hgi_views_encode_dev", "launch_views_encode", "hgi_status hgi_views_decode_dev("),
                                 ("hgi_views_decode_dev", "launch_views_decode", "const char *hgi_views_last_error")):
        body = src[src.index("hgi_status %s(" % entry):src.index(end)]
        first = min(m.start() for m in re.finditer(hip, body))
        assert body[first:].startswith(launcher + "(") and body.index("judge_launch(") < first
        assert "fail(HGI_EINVAL" not in body and "fail(HGI_EUNSUPPORTED" not in body and body.count("fail(HGI_EDEVICE") == 1
        assert body.index("return HGI_OK;") < body.index("judge_launch(")      # the empty plan is decided first
    # the plan header judges in the header's order: NULL entry, pitches, tiles, aliasing; then the 32-bit bound and the page rule
    head = open(os.path.join(VIEWS_DIR, "hgi_views_plan.h")).read()
    body = head[head.index("inline ViewsJudged views_plan("):]
    order = [body.index(k) for k in ("kViewsNullEntry", "kViewsSrcPitch", "kViewsDstPitch", "kViewsTiles", "views_aliasing(", "kViewsFits32", "kViewsTail",
                                     "memcpy(blob")]
    assert order == sorted(order)
    assert body.index("kViewsTiles") < body.index("std::vector<ViewRect>")      # nothing is allocated before the tile count fits


# ---------------------------------------------------------------------------------------------------- argument rules
with open(os.path.join(GOLDEN_DIR, "views_refusals.json")) as _f:
    CALLS = json.load(_f)["calls"]


def _plan(views, keep):
    """hgi_views_plan of [[src, dst, w, h, sp, dp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_views as F
    n = len(views)
    arr = (F.ViewPair * max(n, 1))(*[F.ViewPair(*v) for v in views])
    size = F.lib().hgi_views_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.ViewsInfo()
    st = F.lib().hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def replay(call):
    """One recorded call (tests/golden/make_views_refusals.py says what the fields mean): (status, error text)."""
    from rustyhgi_amd import _ffi_views as F
    L, keep = F.lib(), []
    ramp = np.arange(256, dtype=np.uint8)
    if call["fn"] == "plan":
        views = call["views"]
        n = len(views) if views is not None else 1
        arr = (F.ViewPair * max(n, 1))(*[F.ViewPair(*v) for v in (views or [])])
        size = L.hgi_views_plan_bytes(n)
        host = np.full(size + 16, 0xEE, np.uint8)
        info = F.ViewsInfo()
        st = L.hgi_views_plan(ctypes.addressof(arr) if views is not None else None, n, host.ctypes.data if call["h_plan"] else None,
                              size if call["plan_bytes"] == "enough" else call["plan_bytes"], ctypes.addressof(info) if call["info"] else None)
        assert (host == 0xEE).all() and info.magic == 0, "a refused plan wrote something"
    else:
        info = None
        if call["info"] is not None:
            st0, info, _ = _plan(call["info"], keep)
            assert st0 == 0, F.last_error()
            for k, v in call["damage"].items():
                setattr(info, k, v)
        args = [None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["levels"], call["interp"]]
        if call["fn"] == "encode":
            st = L.hgi_views_encode_dev(*args, ramp.ctypes.data if call["lut"] else None)
        else:
            st = L.hgi_views_decode_dev(*args)
    assert (ramp == np.arange(256)).all()
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    assert sum(c["kind"] == "solo" for c in CALLS) == 18 and sum(c["kind"] == "pair" for c in CALLS) >= 14
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in CALLS)      # refused before any device call
    assert set(c["call"]["fn"] for c in CALLS) == {"plan", "encode", "decode"}


def test_every_recorded_refusal_repeats_its_status_and_text(V):
    for c in CALLS:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    # the texts name the offending list index
    named = dict((c["rule"], c["error"]) for c in CALLS if c["kind"] == "solo")
    assert named["null_entry"].startswith("view 1:") and named["tail"].startswith("view 1:") and "views 0 and 1" in named["out_out"]
    assert "output of view 1" in named["out_in"] and "input of view 0" in named["out_in"]


def test_served_and_empty_plans_without_a_device(V):
    """What is NOT refused, as far as no device is needed: windows side by side in one parent's rows, inputs overlapping inputs, a
    one-row view beside a window; and the empty plans, which the launches accept and do nothing for, whatever the other arguments."""
    from rustyhgi_amd import _ffi
    A, B, keep = 1 << 50, 2 << 50, []
    side_by_side = [[A, B, 32, 8, 40, 64], [A + 4096, B + 32, 32, 8, 40, 64], [A + 8192, B + 8 * 64, 64, 1, 0, 0]]
    st, info, host = _plan(side_by_side, keep)
    assert st == _ffi.OK and info.count == 3 and info.edge_tiles == 3 and info.interior_tiles == 0 and info.max_width == 64
    assert info.plan_bytes == 3 * 64 + 2 * 16 and (host[int(info.plan_bytes):] == 0xEE).all()
    rec = host[:64].view(np.uint64)
    assert int(rec[0]) == A and int(rec[1]) == B      # addresses and sizes, no host pointer: the blob is position-independent
    crops = [[A, B, 32, 8, 40, 32], [A + 5, B + 4096, 32, 8, 40, 32], [A, B + 8192, 32, 8, 40, 32]]
    assert _plan(crops, keep)[0] == _ffi.OK
    L = V.lib()
    for views in ([], [[0, 0, 0, 5, 0, 0], [0, 0, 7, 0, 1, 1]]):
        st, info, _ = _plan(views, keep)
        assert st == _ffi.OK and info.magic == V.MAGIC and info.count == 0 and info.plan_bytes == 0
        for levels, interp, d_plan in ((4, 1, None), (0, 7, 8), (99, -1, None)):
            assert L.hgi_views_encode_dev(None, d_plan, ctypes.addressof(info), levels, interp, None) == _ffi.OK
            assert L.hgi_views_decode_dev(None, d_plan, ctypes.addressof(info), levels, interp) == _ffi.OK
    assert L.hgi_views_plan(None, 0, None, 0, None) == _ffi.OK


# ------------------------------------------------------------------------------------------------------ kernel units
def _isa(unit, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / unit.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(VIEWS_DIR, unit), "-o", out],
                          stderr=subprocess.DEVNULL)
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("unit,name,kernels,sdwa", [("hgi_fused_views_dec.hip", "k_dec_views", 4, 100), ("hgi_fused_views_enc.hip", "k_enc_views", 8, 400)])
def test_view_units_are_within_the_pitched_kernels_budgets(tmp_path, unit, name, kernels, sdwa):
    """k_dec_views<interp, unseeded | cone> and k_enc_views<interp, ident, unseeded | cone>: the SDWA paths really there, the hazard
    rules of tools/check_isa.py (rule 4 covers the row stores: they go through store_row_pair / store_rows_edge), no scratch, no
    spills, no DPP, no traps, no static LDS (the encoder's table sits at LDS offset 0), and the occupancy of the pitched kernels:
    a plain decode tile within 64 VGPRs (eight waves per SIMD), a cone decode within 80 (six), every encode within 94 (five).
    The frame search is scalar: the prefix arrays and the record are read with s_load."""
    import check_isa
    path = _isa(unit, tmp_path)
    r = check_isa.check(path)
    assert r["kernels"] == kernels, r
    assert r["partial_writes"] > sdwa, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert len(set(re.findall(r"\b(_Z\w*%s\w*):" % name, text))) == kernels
    assert not re.search(r"k_(dec|enc)_(tiles|pitched|list)", text)
    assert re.search(r"buffer_store_dwordx4 .* nt", text) and "s_load_dwordx4" in text
    res = CL.resources(text, name)
    assert len(res) == kernels, res
    for k, (vgprs, lds, scratch) in res.items():
        assert lds == 0 and scratch == 0, (k, lds, scratch)
        if name == "k_enc_views":
            assert vgprs <= 94, (k, vgprs)
        else:
            assert vgprs <= (80 if "ELi2EEE" in k else 64), (k, vgprs)


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_walker_under_asan_ubsan(tmp_path):
    """tests/cpp/test_views_plan.cpp, a stand-alone program: every block of 100 000 random small lists walked through the map the
    kernels run, the per-frame geometry against pitched_plan, the aliasing test against bytes, the boundary rules on both sides
    (see the file's head)."""
    exe = str(tmp_path / "test_views_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_views_plan.cpp"), "-o", exe])
    p = subprocess.run([exe, "100000", "0x48474941"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "100000 cases, 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ----------------------------------------------------------------------------------------------------------- Python
def test_aligned_arena_places_frames_disjoint_and_aligned():
    from rustyhgi_amd import aligned_arena
    rng = np.random.default_rng(0x48474941)
    for align in (128, 16, 256, 1):
        shapes = [(int(rng.integers(0, 90)), int(rng.integers(0, 700))) for _ in range(60)] + [(1, 1), (0, 0), (64, 128), (3, 129)]
        total, places = aligned_arena(shapes, align)
        assert len(places) == len(shapes)
        end = 0
        for (h, w), (off, pitch) in zip(shapes, places):
            assert off % align == 0 and pitch % align == 0 and w <= pitch < w + align, (h, w, off, pitch)
            assert off >= end      # list order, nothing shared
            assert not (h and w % 4) or (off + (h - 1) * pitch + w - 1) % 4096 <= 4092      # the page rule, on a page-aligned base
            end = off + (h * pitch if h and w else 0)
        assert total == end
        assert total <= sum(h * (w + align) + 4 * align for h, w in shapes)
    total, places = aligned_arena([(1, 4095), (3, 5)], 1)      # the first frame would end on the last but one byte of a page
    assert places == [(2, 4095), (4097, 5)] and total == 4112
    assert aligned_arena([]) == (0, [])
    assert aligned_arena([(2, 130)]) == (512, [(0, 256)])
    for bad in (0, 3, 100, -128):
        with pytest.raises(ValueError):
            aligned_arena([(2, 2)], bad)
    with pytest.raises(ValueError):
        aligned_arena([(-1, 2)])


def test_view_plan_refuses_bad_layouts_before_any_device_call(V):
    torch = pytest.importorskip("torch")
    from rustyhgi_amd import ViewPlan
    t = torch.zeros((64, 160), dtype=torch.uint8)
    o = torch.zeros((64, 160), dtype=torch.uint8)
    v = t[8:40, 16:100]
    for src, dst in ((t[:, ::2], o[:, :80]), (v, o[8:40, 16:99]), (t.to(torch.float16), o), (t.reshape(-1), o.reshape(-1)), (np.zeros((4, 4), np.uint8), o[:4, :4]),
                     (t.t(), o.t())):
        with pytest.raises(ValueError, match="pair 0"):
            ViewPlan([(src, dst)])
    with pytest.raises(ValueError, match="pair 1"):
        ViewPlan([(v, v), (t[:, ::2], o[:, :80])])
    # a valid layout passes the layout checks and only then meets the CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        ViewPlan([(v, o[8:40, 16:100])])
    p = ViewPlan([])
    assert len(p) == 0 and p.fused and p.blob is None and p.info.count == 0


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("views", after="requant")
