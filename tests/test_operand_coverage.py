"""What the per-pixel code of the kernels is fed, measured on the reference alone (CPU; nothing here touches the library).

The GPU suite compares kernels with the oracle on noise, ramps and photographs, where the Crossed predictor clusters around 128
and the (prediction, pixel) pairs at the ends of the range -- where the quantizer's borrow, overflow, select and wrap decide --
hardly occur.  tests/operand_designs.py builds frames that put EVERY pair in front of every site; this file asserts, with an
instrumented restatement of oracle/hgi_numpy.py that is first shown to equal the oracle bit for bit, that they do, and that six
mutants of the rule each change the bytes of at least one design.  tests/test_operand_coverage_gpu.py pushes the same frames
through every kernel.  Figures (run with -s): profiles/r11_operand_coverage.md."""
import numpy as np
import pytest

import operand_designs as D
from oracle import hgi_numpy as N

TABLES = D.tables()
QUANT = D.quant_designs()
MPX_LIMIT = 32 * 1024 * 1024


def subs_of(req):
    return {sub for sub, _ in req}


def test_window_lattice_holds_all_81_quadruples():
    lat = np.array([[int(c) for c in row] for row in D.WINDOW_LATTICE])
    code = ((lat[:-1, :-1] * 3 + lat[1:, :-1]) * 3 + lat[:-1, 1:]) * 3 + lat[1:, 1:]
    assert lat.shape == (10, 11) and len(np.unique(code)) == 81


def test_tables_keep_a_constant_block_constant_and_pin_the_identity_test():
    ident = np.arange(256, dtype=np.uint8)
    assert set(TABLES) == {"linear1", "linear2", "linear3", "identity", "identity_but_255", "random0"}
    for name, t in TABLES.items():
        assert t.dtype == np.uint8 and t.shape == (256,) and t[0] == 0, name
    assert (TABLES["identity"] == ident).all()
    assert int((TABLES["identity_but_255"] != ident).sum()) == 1
    # ... and its grid differs from the identity's on a design (every residual occurs there), so a kernel that took the
    # residual-only instantiation for it would be caught
    f = D.quant_frame("q8_16")
    assert (N.encode(f, 5, TABLES["identity_but_255"]) != N.encode(f, 5, ident)).any()
    assert D.table_nonzero_origin()[0] != 0


def test_frames_stay_below_32_mpx():
    for name in D.QUANT_FRAMES:
        assert D.quant_frame(name).size <= MPX_LIMIT, name
    for name in D.PRED_FRAMES:
        assert D.pred_frame(name).size <= MPX_LIMIT, name


@pytest.mark.parametrize("levels", [4, 8])
def test_restatement_equals_the_oracle_on_noise(oracle, levels):
    """Two noise cases (the committed 1280 x 640 frame at 4 and at 8 levels), every table, both interpolators, both
    directions, against the C oracle AND the numpy oracle."""
    img, _ = D.noise_case()
    rnd = np.random.default_rng(levels).integers(0, 256, 256, dtype=np.uint8)
    for lut in list(TABLES.values()) + [rnd, D.table_nonzero_origin()]:
        for interp in (1, 0):
            grid, rec, _ = D.encode_cov(img, levels, lut, interp)
            want, wrec, _ = oracle.encode(img, levels, lut, interp, want_rec=True)
            assert (grid == want).all() and (rec == wrec).all()
            assert (grid == N.encode(img, levels, lut, interp)).all()
            out, _ = D.decode_cov(grid, levels, interp)
            assert (out == oracle.decode(want, levels, interp)).all() and (out == rec).all()


@pytest.mark.parametrize("design,frame,levels,req", QUANT, ids=[q[0] for q in QUANT])
def test_quantizer_designs_cover_every_pair_on_every_site(oracle, design, frame, levels, req):
    """The coverage condition, on the reference alone: for every table with lut[0] == 0 and both interpolators, every site of
    every targeted level sees 100 % of the required (p, a) pairs -- all 65 536 at sub 1, 2 and 4, S x S at sub 8 and 16, S' x S'
    above the tile.  The restatement that counts is checked against the oracle on the same call.  The decoder's (p, g) pairs are
    all seen under the identity table, whose g is the residual a - p."""
    img = D.quant_frame(frame)
    assert img.shape[0] % (1 << levels) == 0 and img.shape[1] % (1 << levels) == 0
    for tname, lut in TABLES.items():
        for interp in (1, 0):
            grid, rec, cov = D.encode_cov(img, levels, lut, interp, record=subs_of(req))
            want, wrec, _ = oracle.encode(img, levels, lut, interp, want_rec=True)
            assert (grid == want).all() and (rec == wrec).all(), (design, tname, interp)
            for sub, values in req:
                need = D.required_pairs(values)
                for key in D.site_keys(sub):
                    seen = int((cov.pairs[key] & need).sum())
                    assert seen == int(need.sum()), "%s %s interp %d site %r: %d of %d pairs" % (design, tname, interp, key, seen, need.sum())
            if tname in ("identity", "linear2"):
                out, dcov = D.decode_cov(grid, levels, interp, record=subs_of(req))
                assert (out == oracle.decode(want, levels, interp)).all() and (out == rec).all()
                if tname == "identity":
                    for sub, values in req:
                        if len(values) == 256:
                            assert all(dcov.pairs[key].all() for key in D.site_keys(sub)), (design, interp, sub)
    print("%s: %d x %d (%.1f Mpx), every site of sub %s at 100 %%" % (design, img.shape[1], img.shape[0], img.size / 1e6,
                                                                      sorted(subs_of(req))))


@pytest.mark.parametrize("name", sorted(D.PRED_FRAMES))
def test_predictor_designs_cover_every_quadruple_at_every_level(oracle, name):
    """grid = oracle.encode(D, levels, identity) decodes to D, and the decoder's predictor meets every quadruple over V8 at sub 1,
    2 and 4 and every quadruple over V3 at the deeper levels; so does the lossless encoder's."""
    levels, _ = D.PRED_FRAMES[name]
    img = D.pred_frame(name)
    ident = TABLES["identity"]
    for interp in (1, 0):
        grid = oracle.encode(img, levels, ident, interp)
        out, cov = D.decode_cov(grid, levels, interp)
        assert (out == img).all() and (out == oracle.decode(grid, levels, interp)).all()
        g2, _, ecov = D.encode_cov(img, levels, ident, interp)
        assert (g2 == grid).all()
        for c in (cov, ecov):
            for k in range(levels):
                sub = 1 << k
                assert int(c.quads[sub].sum()) == D.required_quads(sub), (name, interp, sub, int(c.quads[sub].sum()))
    lossy = oracle.encode(img, levels, TABLES["linear2"], 1)
    assert (D.encode_cov(img, levels, TABLES["linear2"], 1, record=False)[0] == lossy).all()
    print("%s: %d x %d (%.1f Mpx), every quadruple at sub 1 ... %d" % (name, img.shape[1], img.shape[0], img.size / 1e6, 1 << (levels - 1)))


MUTANT_DESIGNS = [("q1_L5", "q1", 5), ("q2_L5", "q2", 5), ("q4_L5", "q4", 5), ("q8_16_L5", "q8_16", 5), ("cone7_L7", "cone7", 7),
                  ("pred5_L5", "pred5", 5)]


def _changes(img, levels, lut, mutant, base):
    return bool((D.encode_cov(img, levels, lut, 1, mutant=mutant, record=False)[0] != base).any())


def test_every_mutant_changes_the_bytes_of_a_design():
    """Each mutant of the quantizer step or of the predictor, applied to the restatement, must change the grid of at least one
    design (Crossed, linear_lut(2) and the identity-but-one table; for the borrow test also a table with lut[0] != 0: with
    lut[0] == 0 the mutant `a <= p` is the same function as `a < p`, see operand_designs.table_nonzero_origin, which the
    last assertion states).  The committed noise case beside it: printed, not asserted."""
    luts = {"linear2": TABLES["linear2"], "identity_but_255": TABLES["identity_but_255"], "lut[0]!=0": D.table_nonzero_origin()}
    frames = [(d, D.pred_frame(f) if f in D.PRED_FRAMES else D.quant_frame(f), lv) for d, f, lv in MUTANT_DESIGNS]
    noise, _ = D.noise_case()
    frames.append(("noise_1280x640_L4", noise, 4))
    frames.append(("noise_1280x640_L8", noise, 8))
    caught = {m: [] for m in D.MUTANTS}
    for dname, img, lv in frames:
        for tname, lut in luts.items():
            base = D.encode_cov(img, lv, lut, 1, record=False)[0]
            for m in D.MUTANTS:
                if _changes(img, lv, lut, m, base):
                    caught[m].append((dname, tname))
    print("mutant matrix (x = grid changes), tables " + " / ".join(luts))
    for m in D.MUTANTS:
        print("  %-16s " % m + "  ".join("%s:%s" % (d, "".join("x" if (d, t) in caught[m] else "-" for t in luts)) for d, _, _ in frames))
    for m in D.MUTANTS:
        assert any(not d.startswith("noise") for d, _ in caught[m]), "no design notices the mutant " + m
    assert all(t == "lut[0]!=0" for _, t in caught["borrow_le"])


def test_noise_cases_coverage_report():
    """What the committed noise case shows the per-pixel code (figures only; the one assertion is that it is far from full)."""
    img, _ = D.noise_case()
    for levels in (4, 8):
        _, _, cov = D.encode_cov(img, levels, TABLES["linear2"], 1)
        for label, subs in (("1", [1]), ("2", [2]), (">=4", [1 << k for k in range(2, levels)])):
            keys = [k for k in cov.pairs if k[0] in subs]
            per_site = [cov.pairs[k].mean() for k in keys]
            anywhere = np.zeros(65536, bool)
            for k in keys:
                anywhere |= cov.pairs[k]
            p = np.arange(65536) // 256
            ends = anywhere[(p < 8) | (p > 247)].mean()
            print("noise 1280x640 L%d Crossed linear2, sub %-3s: min per site %.1f %%, any position %.1f %%, p<8 or p>247 %.2f %%"
                  % (levels, label, 100 * min(per_site), 100 * anywhere.mean(), 100 * ends))
            assert min(per_site) < 0.5
