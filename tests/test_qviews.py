"""CPU suite of the requantize view lists (libhgi_qviews.so, include/hgi_qviews.h, Encoder.requantize_views): the companion
library exports its three entry points and nothing else, names no tuning switch, reads no environment and links nothing of
libhgi_hip.so or libhgi_views.so; the ctypes table matches the header, and the plan it takes is the view lists' own; the entry
point decides its rules -- one judgement function in a plain C++ header -- before the first HIP call; the refusals recorded in
tests/golden/qviews_refusals.json repeat their status and text without a device; the kernel unit compiles for gfx950 within
k_requant's budget and passes tools/check_isa.py; the judgement holds under ASan / UBSan (tests/cpp/test_qviews_plan.cpp, a
stand-alone program); Encoder.requantize_views serves what needs no device without one."""
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

QVIEWS_DIR = os.path.join(ROOT, "rustyhgi_amd", "qviews")
NAMES = ("hgi_qviews_requant_dev", "hgi_qviews_last_error", "hgi_qviews_version")
FILES = ["Makefile", "hgi_fused_qviews.hip", "hgi_qviews.hip", "hgi_qviews.map", "hgi_qviews_kernels.h", "hgi_qviews_plan.h"]
UNIT = "hgi_fused_qviews.hip"
WAVES, VGPR_BUDGET = 5, 96      # HGI_ENC_WAVES_PER_EU: 512 VGPRs per SIMD lane, allocated in eights


@pytest.fixture(scope="module")
def Q():
    CL.binding("views")      # the plan of this library is hgi_views_plan's
    return CL.binding("qviews")


# ------------------------------------------------------------------------------------------------- exports and build
def test_library_exports_exactly_the_three_entry_points(Q):
    nm = shutil.which("nm")
    assert nm, "binutils nm is needed to list the exports"
    out = subprocess.check_output([nm, "-D", "--defined-only", Q.LIB_PATH], text=True)
    exported = sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip())
    assert exported == sorted(NAMES), exported
    script = open(os.path.join(QVIEWS_DIR, "hgi_qviews.map")).read()
    assert re.search(r"global:\s*hgi_qviews_\*;", script) and re.search(r"local:\s*\*;", script)
    declared = set(re.findall(r"HGI_API\s+[\w\s\*]+?\b(hgi_qviews_\w+)\s*\(", CL.header("qviews")))
    assert declared == set(NAMES) == set(s[0] for s in Q.SYMBOLS)
    version = Q.lib().hgi_qviews_version()
    assert version.startswith(b"hgi_qviews 1.0") and b"gfx950" in version
    # stateless and switch-free: no tuning-constant or switch name in the object, no environment read in the sources, nothing
    # of libhgi_hip.so or of libhgi_views.so linked
    strings = shutil.which("strings")
    assert strings, "binutils strings is needed to search the object for switch names"
    assert re.findall(r"HGI_[A-Z0-9_]+", subprocess.check_output([strings, Q.LIB_PATH], text=True)) == []
    CL.check_sources(QVIEWS_DIR, FILES)
    readelf = shutil.which("readelf")
    assert readelf, "binutils readelf is needed to list what the library links"
    linked = subprocess.check_output([readelf, "-d", Q.LIB_PATH], text=True)
    assert "libhgi_hip" not in linked and "libhgi_views" not in linked and "libhgi_requant" not in linked
    # the Makefile: the fragment the sibling libraries build with, their flags, and the files only this library includes
    mk = open(os.path.join(QVIEWS_DIR, "Makefile")).read()
    code = [l.strip() for l in mk.splitlines() if l.strip() and not l.startswith("#")]
    assert len(code) == 4 and code[:2] == ["NAME := qviews", "FUSED := hgi_fused_enc.hip"] and code[3] == "include ../companion/companion.mk", code
    assert code[2].startswith("ALSO := ") and "CXXFLAGS" not in mk and "EXTRA" not in mk
    also = code[2].split()[2:]
    assert all(os.path.isfile(os.path.join(QVIEWS_DIR, f)) for f in also), also
    # ... every file of the sibling directories that the units include, directly or through them, is a dependency
    assert {"../requant/hgi_fused_requant.hip", "../requant/hgi_requant_kernels.h", "../requant/hgi_requant_plan.h", "../views/hgi_views_tile.h",
            "../views/hgi_views_kernels.h", "../views/hgi_views_plan.h", "../csrc/hgi_framelist.h", "../../include/hgi_views.h"} <= set(also)
    included = set()
    for fn in FILES[1:3] + FILES[4:]:
        included |= set(re.findall(r'#include "(\.\./(?:requant|views)/[^"]+)"', open(os.path.join(QVIEWS_DIR, fn)).read()))
    assert included == {"../requant/hgi_fused_requant.hip", "../views/hgi_views_tile.h", "../views/hgi_views_plan.h"} and included <= set(also)


def test_the_unit_is_the_frame_search_in_front_of_k_requants_body():
    """hgi_fused_qviews.hip: the requantize unit and the view lists' tile header included as they stand, no device function and
    no store of its own, k_requant's body call for call, the launch through the launch layer."""
    src = open(os.path.join(QVIEWS_DIR, UNIT)).read()
    assert src.index('#include "../requant/hgi_fused_requant.hip"') < src.index('#include "../views/hgi_views_tile.h"') < src.index('#include "hgi_qviews_kernels.h"')
    assert "#define" not in src and len(re.findall(r"^#include", src, flags=re.M)) == 3
    # what the requantize unit brings: the encode direction's unit without its launchers, the pitched staging, the tile layer
    requant = open(os.path.join(ROOT, "rustyhgi_amd", "requant", "hgi_fused_requant.hip")).read()
    assert "#define HGI_FUSED_NO_LAUNCHERS 1" in requant and '#include "../csrc/hgi_fused_enc.hip"' in requant
    assert requant.index('"../csrc/hgi_fused_pitched.h"') < requant.index('"../companion/hgi_tile.h"')
    assert "launch_tile_kernel<k_requant_views<I, SE>>" in src and "with_choices(" in src and "hipLaunchKernelGGL" not in src
    assert "views_tile_launch(a, k, up)" in src and "enc_lds_bytes(t.nh)" in src and "OneOf<2, 0>{t.cone ? 2 : 0}" in src
    assert src.count("view_ctx(a)") == 1 and src.count("amdgpu_waves_per_eu(HGI_ENC_WAVES_PER_EU)") == 1
    assert "__device__" not in src and src.count("__global__") == 1      # no device function of its own
    assert "buffer_store" not in src and "store_rows" not in src and "store_row_pair" not in src      # every store is the encoder tile's
    # k_requant's body: the same calls, as many times, in the same order
    calls = r"\b(pitched_buf|pitched_issue(?:_odd)?|stage_commit|cone_issue|cone_finish|dec_seed_commit|dec_chain|lattice_fast|dec_fine_keep|cone_recode|enc_seed_commit|enc_tile_fast|enc_tile_edge)(<[^>(]*>)?\("

    def body(text, kernel):
        b = text[text.index("void %s(" % kernel):]
        return [m.group(1) + (m.group(2) or "") for m in re.finditer(calls, b[:b.index("\n}\n")])]
    mine, theirs = body(src, "k_requant_views"), body(requant, "k_requant")
    assert mine == theirs and len(mine) == 30, (mine, theirs)
    for piece, times in (("pitched_buf(fr, out, p, tl, &rb)", 1), ("stage_commit<false>(", 2), ("cone_issue<false>(", 2), ("cone_finish<INTERP, false, true>(", 2),
                         ("dec_fine_keep<INTERP>(", 1), ("dec_fine_keep<INTERP, 1>(", 1), ("dec_fine_keep<INTERP, 2>(", 1), ("cone_recode<INTERP>(", 3),
                         ("enc_tile_fast<INTERP, false>(", 1), ("enc_tile_edge<INTERP, false, 1>(", 1), ("enc_tile_edge<INTERP, false, 2>(", 1)):
        assert src.count(piece) == times, piece
    # the plan header: plain C++, the view lists' plan by inclusion, nothing of a blob of its own
    plan = open(os.path.join(QVIEWS_DIR, "hgi_qviews_plan.h")).read()
    assert '#include "../views/hgi_views_plan.h"' in plan and '#include "../../include/hgi_qviews.h"' in plan
    assert not re.search(r"\bhip[A-Z_]\w*", plan) and "struct ViewFrame" not in plan and "MAGIC 0x" not in plan and "ViewRect" not in plan
    assert "views_info_consistent(" in plan and "view_args(" in open(os.path.join(QVIEWS_DIR, "hgi_qviews.hip")).read()
    assert '#include "hgi_views.h"' in open(os.path.join(ROOT, "include", "hgi_qviews.h")).read()


def test_ctypes_table_matches_the_header(Q):
    from rustyhgi_amd import _ffi
    head = CL.header("qviews")
    table = dict((s[0], s) for s in Q.SYMBOLS)
    want = {"hgi_qviews_requant_dev": (_ffi._int, [_ffi._vp, _ffi._vp, _ffi._vp, _ffi._u32, _ffi._int, _ffi._vp]),
            "hgi_qviews_last_error": (ctypes.c_char_p, []), "hgi_qviews_version": (ctypes.c_char_p, [])}
    assert set(want) == set(table)
    for n, (res, args) in want.items():
        m = re.search(r"HGI_API\s+[\w\s\*]+?\b%s\s*\(([^)]*)\)" % n, head)
        assert m and (m.group(1).strip() == "void") == (not args) and (not args or len(m.group(1).split(",")) == len(args)), n
        assert table[n][1] is res and table[n][2] == args, n
    # the launch takes hgi_views_info: no structure, no magic and no plan entry of this library's own
    assert "const hgi_views_info *info" in head and "typedef struct" not in head and "MAGIC" not in head and "_plan(" not in head
    assert not hasattr(Q, "MAGIC") and not [n for n in dir(Q) if n.endswith("Info") or n.endswith("Pair")]


def test_the_entry_judges_first_and_in_the_headers_order():
    CL.check_rule_order("qviews", "hgi_qviews_requant_dev", "launch_qviews_requant")
    src = open(os.path.join(QVIEWS_DIR, "hgi_qviews.hip")).read()
    body = src[src.index("hgi_status hgi_qviews_requant_dev("):src.index("const char *hgi_qviews_last_error")]
    assert body.index("qviews_judge(") < body.index("return HGI_OK;") < body.index("return fail(") < body.index("launch_qviews_requant(")
    assert body.count("fail(HGI_EDEVICE") == 1 and body.index("launch_qviews_requant(") < body.index("fail(HGI_EDEVICE")
    # the judgement: one function, no HIP call, the empty plan first, then the rules in the header's order
    plan = open(os.path.join(QVIEWS_DIR, "hgi_qviews_plan.h")).read()
    judge = plan[plan.index("inline QViewsJudged qviews_judge("):]
    assert not re.search(r"\bhip[A-Z]\w*\s*\(|launch_\w+\s*\(", judge)
    order = [judge.index(k) for k in ("info->count == 0 && views_info_consistent(*info)) return j;", "kQViewsInfoNull)", "kQViewsInfo)", "kQViewsPlanNull)",
                                      "kQViewsPlanAlign)", "kQViewsLutNull)", "kQViewsLevelsRange)", "kQViewsInterp)", "kQViewsLevels)", "qviews_identity(lut)",
                                      "kQViewsIdentity)", "split_levels(")]
    assert order == sorted(order)
    statuses = re.findall(r"return refuse\((HGI_\w+), kQViews\w+\);", judge)
    assert statuses == ["HGI_EINVAL"] * 7 + ["HGI_EUNSUPPORTED"] * 2
    assert "copy the source" in judge


# ---------------------------------------------------------------------------------------------------- argument rules
def _calls():
    with open(os.path.join(GOLDEN_DIR, "qviews_refusals.json")) as f:
        return json.load(f)["calls"]


def _plan(views, keep):
    """hgi_views_plan (libhgi_views.so) of [[src, dst, w, h, sp, dp], ...] into memory of our own: (status, info, host blob)."""
    from rustyhgi_amd import _ffi_views as F
    n = len(views)
    arr = (F.ViewPair * max(n, 1))(*[F.ViewPair(*v) for v in views])
    size = F.lib().hgi_views_plan_bytes(n)
    host = np.full(size + 16, 0xEE, np.uint8)
    info = F.ViewsInfo()
    st = F.lib().hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
    keep += [arr, host, info]
    return st, info, host


def table(name):
    """The tables a recorded call names (tests/golden/make_qviews_refusals.py)."""
    if name is None:
        return None
    if name == "coarse":
        return np.minimum(np.arange(256) // 8 * 8 + 4, 255).astype(np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    if name.startswith("identity^"):
        lut[int(name[9:])] ^= 1
    else:
        assert name == "identity", name
    return lut


def replay(call):
    """One recorded call: (status, error text)."""
    from rustyhgi_amd import _ffi_qviews as F
    from rustyhgi_amd import _ffi_views
    keep, info = [], None
    if call["info"] is not None:
        st0, info, _ = _plan(call["info"], keep)
        assert st0 == 0, _ffi_views.last_error()
        for k, v in call["damage"].items():
            setattr(info, k, v)
    lut = table(call["lut"])
    st = F.lib().hgi_qviews_requant_dev(None, call["d_plan"], ctypes.addressof(info) if info is not None else None, call["levels"], call["interp"],
                                        lut.ctypes.data if lut is not None else None)
    return st, F.last_error()


def test_the_list_covers_every_rule():
    from rustyhgi_amd import _ffi
    calls = _calls()
    solo = [c["rule"] for c in calls if c["kind"] == "solo"]
    assert solo == ["info_null", "info_inconsistent", "d_plan_null", "d_plan_aligned", "lut_null", "levels_range", "interp", "levels_launch", "identity"]
    assert all(c["status"] in (_ffi.EINVAL, _ffi.EUNSUPPORTED) for c in calls)      # refused before any device call
    status = dict((c["rule"], c["status"]) for c in calls if c["kind"] == "solo")
    unsupported = [r for r in solo if status[r] == _ffi.EUNSUPPORTED]
    assert unsupported == ["levels_launch", "identity"]      # ... behind every HGI_EINVAL rule
    pairs = [(c["rule"], c["also_breaks"]) for c in calls if c["kind"] == "pair"]
    # adjacent rules in pairs (but the two that cannot be broken together), the earlier one recorded
    for a, b in zip(solo, solo[1:]):
        assert (a, b) in pairs or (a, b) in (("info_null", "info_inconsistent"), ("d_plan_null", "d_plan_aligned")), (a, b)
    assert all(solo.index(a) < solo.index(b) for a, b in pairs)
    # the identity table is refused only behind every HGI_EINVAL rule and behind the depth rule
    assert set(a for a, b in pairs if b == "identity") == set(solo[:-1]) - {"lut_null"}
    extras = dict((c["note"], c) for c in calls if c["kind"] == "extra")
    assert extras["the mapped view lists' magic"]["status"] == extras["the typed view lists' magic"]["status"] == _ffi.EINVAL


def test_every_recorded_refusal_repeats_its_status_and_text(Q):
    calls = _calls()
    for c in calls:
        st, text = replay(c["call"])
        where = "%s %s %s %s" % (c["kind"], c["rule"], c["also_breaks"] or "", c["note"])
        assert st == c["status"], (where, st, text)
        assert text == c["error"], (where, text)
    named = dict((c["rule"], c["error"]) for c in calls if c["kind"] == "solo")
    assert "copy the source" in named["identity"] and "hgi_views_plan" in named["info_inconsistent"]


def test_served_judgements_and_empty_plans_without_a_device(Q):
    """What needs no device: the empty plans, which the launch accepts and does nothing for, whatever the other arguments; the
    infos of the sibling lists, which are not this library's; a refused plan's zeroed info."""
    from rustyhgi_amd import _ffi, _ffi_mviews, _ffi_tviews, _ffi_views
    L, keep = Q.lib(), []
    ident, medium = table("identity"), table("coarse")
    for views in ([], [[0, 0, 0, 5, 0, 0], [0, 0, 7, 0, 1, 1]]):
        st, info, _ = _plan(views, keep)
        assert st == _ffi.OK and info.magic == _ffi_views.MAGIC and info.count == 0 and info.plan_bytes == 0
        for levels, interp, d_plan, lut in ((4, 1, None, None), (0, 7, 8, ident.ctypes.data), (99, -1, None, medium.ctypes.data), (4, 1, 16, ident.ctypes.data)):
            assert L.hgi_qviews_requant_dev(None, d_plan, ctypes.addressof(info), levels, interp, lut) == _ffi.OK
    for other, plan in ((_ffi_mviews.MViewsInfo(), lambda i: _ffi_mviews.lib().hgi_mviews_plan(None, 0, 4, None, 0, i)),
                        (_ffi_tviews.TViewsInfo(), lambda i: _ffi_tviews.lib().hgi_tviews_plan(None, 0, 4, None, 0, i))):
        assert plan(ctypes.addressof(other)) == _ffi.OK and ctypes.sizeof(other) >= ctypes.sizeof(_ffi_views.ViewsInfo)
        assert L.hgi_qviews_requant_dev(None, None, ctypes.addressof(other), 4, 1, medium.ctypes.data) == _ffi.EINVAL
        assert "hgi_views_plan" in Q.last_error()
    st, info, host = _plan([[1 << 50, 1 << 50, 32, 8, 32, 32]], keep)      # in place: the plan refuses it, as requantize does
    assert st == _ffi.EINVAL and bytes(info) == bytes(ctypes.sizeof(info)) and (host == 0xEE).all()
    assert L.hgi_qviews_requant_dev(None, 1 << 40, ctypes.addressof(info), 4, 1, medium.ctypes.data) == _ffi.EINVAL


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
def test_unit_is_within_k_requants_budget(tmp_path):
    """k_requant_views<interp, unseeded | cone>, four kernels: the hazard rules of tools/check_isa.py as the requantize unit
    passes them, no scratch, no spills, no DPP, no traps, no static LDS (the table sits at LDS offset 0), and k_requant's
    occupancy: five waves per SIMD, at most 96 VGPRs, read from the listing's metadata.  The listing also holds the four
    k_requant of the included requantize unit, which nothing launches: within the same budget.  Nothing here searches the
    instructions: that is check_isa's."""
    import check_isa
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    path = str(tmp_path / UNIT.replace(".hip", ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(QVIEWS_DIR, UNIT), "-o", path],
                          stderr=subprocess.DEVNULL)
    r = check_isa.check(path)
    assert r["kernels"] == 8, r
    assert r["partial_writes"] > 800, r
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["adjacent_dependent"] == 0 and r["store_data_overwritten"] == 0 and r["dpp"] == 0 and r["traps"] == 0, r
    text = open(path).read()
    assert VGPR_BUDGET == 512 // WAVES // 8 * 8
    for name in ("k_requant_views", "k_requantI"):
        res = _metadata(text, name)
        assert len(res) == 4, res
        for k, (vgprs, vspill, sspill, scratch, lds) in res.items():
            assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0, (k, vspill, sspill, scratch, lds)
            assert vgprs <= VGPR_BUDGET, (k, vgprs)
        assert set(CL.resources(text, name)) == set(res)
    # <INTERP, SEEDED>: both interpolators, unseeded and the cone, and no kernel for the identity table
    assert sorted(re.search(r"k_requant_viewsILi(\d)ELi(\d)EE", k).groups() for k in _metadata(text, "k_requant_views")) == [("0", "0"), ("0", "2"), ("1", "0"), ("1", "2")]
    assert "k_enc_views" not in text and "k_enc_pitched" not in text and "k_dec_views" not in text


# -------------------------------------------------------------------------------------------------------- host plan
def test_plan_program_under_asan_ubsan(tmp_path):
    """tests/cpp/test_qviews_plan.cpp, a stand-alone program: random lists through views_plan and then through qviews_judge, every
    rule alone and in pairs, the sibling magics, the identity table and its one-entry neighbours, the block count (see the file's
    head)."""
    CL.run_plan_program("qviews", tmp_path, flags=("-Werror",))


# ----------------------------------------------------------------------------------------------------------- Python
class _Plan:
    """What _views_launch reads of a ViewPlan, for the cases that need no device."""

    def __init__(self, srcs, dsts, device=None, fused=True):
        self.srcs, self.dsts, self.device, self.fused, self.blob = list(srcs), list(dsts), device, fused, None
        self.layouts = [(0, 0, int(s.shape[1]), int(s.shape[0]), int(s.shape[1]), int(s.shape[1])) for s in self.srcs]

    def __len__(self):
        return len(self.srcs)


def test_requantize_views_without_a_device(Q):
    torch = pytest.importorskip("torch")
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    assert hasattr(H.Encoder, "requantize_views")
    medium = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    ident = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Lossless), 4)
    assert bool((ident._lut == np.arange(256)).all()) and not bool((medium._lut == np.arange(256)).all())
    # empty plans need no device: the view lists' own plan object, and lists of empty views
    p = H.ViewPlan([])
    assert len(p) == 0 and p.fused and p.blob is None and p.info.count == 0
    for enc in (medium, ident):
        assert enc.requantize_views(p) == []
        assert H.Encoder(Crossed(), enc.quantizator, 9).requantize_views(p) == []
    g = torch.zeros((0, 5), dtype=torch.uint8)
    out = medium.requantize_views(_Plan([g], [g]))
    assert len(out) == 1 and out[0] is g
    # CPU tensors are refused where the plan is made, as `requantize` refuses them: before any table is looked at
    a, b = torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 32), dtype=torch.uint8)
    for enc in (medium, ident):
        with pytest.raises(ValueError, match="GPU"):
            H.ViewPlan([(a, b)])
        with pytest.raises(ValueError, match="GPU"):
            enc.requantize(a, out=b)
    # a context of another device: judged in front of both routes and of the identity copy
    class Ctx:
        device = 1
    for quant in (QuantizationLevel.Medium, QuantizationLevel.Lossless):
        enc = H.Encoder(Crossed(), Linear.from_level(quant), 4)
        enc._ctx = Ctx()
        for fused in (True, False):
            with pytest.raises(ValueError, match="context was created for cuda:1"):
                enc.requantize_views(_Plan([a], [b], device=torch.device("cuda", 0), fused=fused))
    assert (b == 0).all()


def test_build_entry_builds_the_companion_library():
    CL.check_build_entry("qviews", after="tviews")
    import rustyhgi_amd
    assert hasattr(rustyhgi_amd.Encoder, "requantize_views") and "requantize_views" in rustyhgi_amd.__doc__
    from rustyhgi_amd import _ffi_qviews
    assert _ffi_qviews.LIB_PATH.endswith("libhgi_qviews.so")
