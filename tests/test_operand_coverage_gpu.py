"""GPU suite of the operand-coverage designs (tests/operand_designs.py; what they cover is asserted on the CPU in
tests/test_operand_coverage.py): every design goes through every entry point that has a kernel of its own and is compared with
the oracle bit for bit.  The quantizer designs put every (prediction, pixel) pair in front of every byte lane of the hand-written
quantizer step, the predictor designs every corner quadruple over the edge values in front of the packed averages; a mistake
confined to one lane at p = 255 or to one carry fails here and nowhere else in the suite.

One test case is (design, interpolator, part): `uniform` runs the *_dev calls on a fused and on a level-wise context (and is
what the forced-path children re-run on the knobs build), `variants` the pitched, list, reconstruction, region, scaled,
mapped and typed kernels (typed encode takes the design lifted to float16 / bfloat16 / float32 elements whose conversion is
exactly the design: tests/typed_reference.py:preimages).  The oracle's grid and decode are computed once per (design, table, interpolator) and shared by both parts.
Outputs with a pitch are written into sentinel-filled parents that are checked whole; inputs with a pitch are read out of
parents of random bytes.  Expected bytes: the oracle.  Never the library under test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import operand_designs as D
from kernel_calls import (SENT, H, Plane, assert_same, call_list, ctxs, dev, injective_table, lift_dev, run_list, run_mapped,  # noqa: F401
                          run_narrowed, run_pitched, run_recon, run_region, run_scaled, run_typed, run_uniform, same_dev, typed_choice)

pytestmark = pytest.mark.gpu
TABLES = D.tables()
TABLES_PLUS = dict(TABLES, nonzero_origin=D.table_nonzero_origin())


def _designs():
    """name -> (frame name, levels, table names, targeted subs)."""
    out = {}
    for name, frame, lv, req in D.quant_designs():
        big = D.quant_frame(frame).size > 12e6
        out[name] = (frame, lv, ("linear2", "identity", "identity_but_255", "random0") if big else tuple(TABLES_PLUS), [s for s, _ in req])
    for frame, (lv, _) in D.PRED_FRAMES.items():
        out["%s_L%d" % (frame, lv)] = (frame, lv, ("identity", "linear2"), [1 << k for k in range(lv)])
    # the lattice kernel (nine levels and more): one design each at 9 and 12 levels
    out["q8_16_L9"] = ("q8_16", 9, ("linear2", "identity"), [8, 16])
    out["pred5_L12"] = ("pred5", 12, ("identity", "linear2"), [1 << k for k in range(5)])
    return out


DESIGNS = _designs()
CASES = [(d, i, part) for d in DESIGNS for i in (1, 0) for part in ("uniform", "variants")]


def narrowed(design, tname):
    return design.startswith(("q1_", "q2_")) and tname in ("linear2", "identity")


def typed_calls(design, interp):
    """The typed calls of a design's `variants` part: [(table name, E, kind, (scale, bias), also narrowed)].  Typed encode takes
    up to eight levels (its contract).  Kind and pair go by the design's place in DESIGNS and the interpolator, not by the
    table, so that the design is lifted once per element size.  tests/test_typed_coverage.py counts the kernel instantiations
    these calls reach."""
    _, levels, tnames, _ = DESIGNS[design]
    if levels > 8:
        return []
    n = list(DESIGNS).index(design) + interp
    return [(tname, E) + typed_choice(E, n) + (narrowed(design, tname),) for tname in tnames for E in (2, 4)]


def frame_of(design):
    f = DESIGNS[design][0]
    return D.pred_frame(f) if f in D.PRED_FRAMES else D.quant_frame(f)


@functools.lru_cache(maxsize=8)
def expected(design, tname, interp):
    """(grid, decode) of the oracle, once per (design, table, interpolator): the two parts of a design run back to back."""
    from oracle import hgi_oracle as O
    O.build()
    _, levels, _, _ = DESIGNS[design]
    grid = O.encode(frame_of(design), levels, TABLES_PLUS[tname], interp)
    return grid, O.decode(grid, levels, interp)


@pytest.mark.parametrize("design,interp,part", CASES, ids=["%s-i%d-%s" % c for c in CASES])
def test_design_through_every_entry_point(H, ctxs, oracle, design, interp, part):
    """Every table of the design, one interpolator: `uniform` -- hgi_encode_u8_dev / hgi_decode_u8_dev on a fused and on a
    level-wise context; `variants` -- pitched, frame list, encode with reconstruction (grid and reconstruction), region (two
    windows at odd offsets), scaled at s = 1 and 2 where a targeted level survives the shift, mapped decode with E = 2 and 4
    and an injective table, typed encode with E = 2 and 4 (reconstruction, mapping and typed encode up to eight levels: their
    contract); the sub 1 and sub 2 designs also at width - 1 and width - 2 under two tables.  All against the oracle, bit for bit."""
    _, levels, tnames, subs = DESIGNS[design]
    img = frame_of(design)
    d_img = dev(img)
    fused = ctxs["fused"]
    typed = {}
    if part == "variants":
        calls = typed_calls(design, interp)
        # lifted once per (design, E): the frame does not depend on the table
        typed = {E: (kind, pair, lift_dev(d_img, kind, pair, salt=levels)) for _, E, kind, pair, _ in calls[:2]}
        assert all(typed[E][:2] == (kind, pair) for _, E, kind, pair, _ in calls)
    for tname in tnames:
        lut = np.ascontiguousarray(TABLES_PLUS[tname])
        grid, dec = expected(design, tname, interp)
        d_grid, d_dec = dev(grid), dev(dec)
        what = "%s %s interp %d" % (design, tname, interp)
        if part == "uniform":
            run_uniform(ctxs, d_img, d_grid, d_dec, levels, interp, lut, what)
            continue
        run_pitched(fused, d_img, d_grid, d_dec, levels, interp, lut, what)
        run_list(fused, oracle, img, d_img, d_grid, d_dec, levels, interp, lut, what)
        run_region(fused, d_grid, d_dec, levels, interp, what)
        for shift in (1, 2):
            if max(subs) >= 1 << shift:
                run_scaled(fused, d_grid, d_dec, levels, interp, shift, what)
        if levels <= 8:
            run_recon(d_img, d_grid, d_dec, levels, interp, lut, what)
            for E in (2, 4):
                run_mapped(d_grid, d_dec, levels, interp, E, what)
            for E, (kind, pair, lifted) in sorted(typed.items()):
                run_typed(d_img, d_grid, levels, interp, lut, E, kind, pair, what, lifted=lifted)
        if narrowed(design, tname):
            run_narrowed(fused, oracle, img, d_img, levels, interp, lut, what, typed=typed)


# ------------------------------------------------------------------------------------ forced paths, knobs build
CHILD_MODES = ["HGI_FORCE_CHECKED=1", "HGI_TILE_H=64", "HGI_TILE_H=32", "HGI_TILE_H=16"]
_child_lost = []


@pytest.mark.parametrize("mode", CHILD_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """A child process on the KNOBS build re-runs this file's uniform cases with the checked path or one tile height forced (as
    tests/test_parity_gpu.py does for its shapes): the bytes must not depend on it.  Each child has its own timeout; once a
    child has ended by signal or timeout this test fails at once and starts no other."""
    from rustyhgi_amd import _ffi
    assert not _child_lost, "not started: the child under %s ended by signal or timeout" % _child_lost[0]
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs), "libhgi_hip_knobs.so is missing: __graft_entry__.build() / `make -C rustyhgi_amd/csrc knobs` builds it"
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
           "-k", "uniform"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _child_lost.append(mode)
        pytest.fail(mode + ": the child did not finish in 600 s")
    if r.returncode < 0:
        _child_lost.append(mode)
        pytest.fail("%s: the child ended by signal %d\n%s" % (mode, -r.returncode, r.stdout[-2000:] + r.stderr[-1000:]))
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]
    assert "%d passed" % (len(CASES) // 2) in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------- graph capture, companion libraries
def test_companion_calls_replay_from_a_graph(H, oracle):
    """include/hgi_recon.h and include/hgi_map.h: "capturable into a graph".  One hgi_recon_encode_u8_dev and one
    hgi_map_decode_dev call (384 x 127, three levels, batch 2, a pitch on every side), each a single kernel, captured on a side
    stream into one graph -- a linear chain -- and replayed twice on pixels, grids and table contents written in place; every
    replay against the oracle, the sentinels around every output row intact."""
    import torch
    from rustyhgi_amd import _ffi_map as M, _ffi_recon as R
    w, h, levels, B, E = 384, 127, 3, 2, 4
    lut = np.ascontiguousarray(TABLES["linear2"])
    sp, gp, rp, mp, op = w + 16, w + 61, w + 128, w + 3, (w + 5) * E
    img = torch.zeros((B, h, sp), dtype=torch.uint8, device="cuda")
    grid = torch.full((B, h, gp), SENT, dtype=torch.uint8, device="cuda")
    rec = torch.full((B, h, rp), SENT, dtype=torch.uint8, device="cuda")
    mgrid = torch.zeros((B, h, mp), dtype=torch.uint8, device="cuda")
    out = torch.full((B, h, op), SENT, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros((256,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()

    def chain(stream):
        R.check(R.lib().hgi_recon_encode_u8_dev(stream, img.data_ptr(), sp, w, h, levels, 1, lut.ctypes.data, grid.data_ptr(), gp,
                                                rec.data_ptr(), rp, B, h * sp, h * gp, h * rp))
        M.check(M.lib().hgi_map_decode_dev(stream, mgrid.data_ptr(), mp, w, h, levels, 1, d_table.data_ptr(), E, out.data_ptr(), op, B,
                                           h * mp, h * op))

    with torch.cuda.stream(side):
        chain(side.cuda_stream)          # both code objects loaded before the capture begins
        side.synchronize()
        grid.fill_(SENT)
        rec.fill_(SENT)
        out.fill_(SENT)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(side.cuda_stream)
    rng = np.random.default_rng(0x48474934)
    for rep in range(2):
        pix = rng.integers(0, 256, (B, h, sp), dtype=np.uint8)
        grids = rng.integers(0, 256, (B, h, mp), dtype=np.uint8)
        table = injective_table(E, rep)
        img.copy_(dev(pix))
        mgrid.copy_(dev(grids))
        d_table.copy_(dev(table.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        hg, hr, ho = grid.cpu().numpy(), rec.cpu().numpy(), out.cpu().numpy()
        for f in range(B):
            want = oracle.encode(pix[f, :, :w], levels, lut, 1)
            assert_same(hg[f, :, :w], want, "replay %d grid %d" % (rep, f))
            assert_same(hr[f, :, :w], oracle.decode(want, levels, 1), "replay %d reconstruction %d" % (rep, f))
            dec = oracle.decode(np.ascontiguousarray(grids[f, :, :w]), levels, 1)
            assert_same(np.ascontiguousarray(ho[f, :, :w * E]).view(np.uint32), table[dec], "replay %d mapped %d" % (rep, f))
        assert (hg[:, :, w:] == SENT).all() and (hr[:, :, w:] == SENT).all() and (ho[:, :, w * E:] == SENT).all(), "replay %d: sentinels" % rep
        assert (img.cpu().numpy() == pix).all() and (mgrid.cpu().numpy() == grids).all(), "replay %d: an input was modified" % rep
    del g
