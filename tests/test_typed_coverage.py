"""What the coverage designs can see of typed encode, measured on the reference alone (CPU; nothing here touches the library).

tests/test_operand_coverage_gpu.py, tests/test_geometry_coverage_gpu.py and tests/test_tilewalk_gpu.py put their uint8 designs
through hgi_typed_encode_dev as frames of float16 / bfloat16 / float32 elements.  This file asserts what that rests on:

1. the lift: for every (kind, (scale, bias)) the GPU suites use, tests/typed_reference.py:preimages holds for every pixel value
   finite elements that `quantize` sends to exactly that value -- extremes of the value's group, its centre and a tie where one
   exists -- so a lifted frame converts back to its design; bfloat16 under (-3.5, 300) reaches 224 of the 256 values only, which
   is why no suite runs it under that pair;
2. the pairs: a load outside the image that reads the element 0.0 instead of writing pixel 0 is the mutant `right`, `below` or
   `corner` of tests/geometry_designs.py with the pixel of 0.0 as the fill.  Under (1, 37.25) and (-3.5, 300) it changes the
   grid on exactly the shapes the mutant applies to; under (255, 0) the pixel of 0.0 is 0 and it changes nothing -- that pair
   would make the mistake the same function as the correct kernel, and the geometry family does not use it;
3. the census: the typed calls of the operand suite give every one of the sixteen instantiations of the typed kernel (INTERP,
   IDENT, SEEDED, E) at least one quantizer design and one predictor design.
Figures (run with -s): profiles/r14_typed_coverage.md."""
import numpy as np
import pytest

import geometry_designs as G
import kernel_calls as K
import operand_designs as D
import typed_reference as TR

IDENT = np.arange(256, dtype=np.uint8)
UNUSED = (255.0, 0.0)


def pixel_of_zero(pair):
    return int(TR.quantize(np.zeros(1, np.float32), *pair)[0])


def test_the_pairs_are_what_the_suites_say():
    assert K.TYPED_CHOICES == tuple(sorted([(K.F16, K.PAIR_A), (K.F16, K.PAIR_B), (K.BF16, K.PAIR_A), (K.F32, K.PAIR_A), (K.F32, K.PAIR_B)]))
    assert {K.PAIR_A, K.PAIR_B, UNUSED} == set(TR.PAIRS)
    assert [pixel_of_zero(p) for p in (K.PAIR_A, K.PAIR_B, UNUSED)] == [37, 255, 0]
    for E in (2, 4):
        seen = [K.typed_choice(E, n) for n in range(8)]
        assert seen[:4] == seen[4:] and all(K.ESIZE[kind] == E for kind, _ in seen)
        assert {p for _, p in seen} == {K.PAIR_A, K.PAIR_B}


@pytest.mark.parametrize("kind,pair", K.TYPED_CHOICES + ((K.F16, UNUSED), (K.BF16, UNUSED), (K.F32, UNUSED)),
                         ids=lambda v: v if isinstance(v, str) else "x%g+%g" % v)
def test_preimages_convert_to_their_value(kind, pair):
    """quantize(bank)[v, j] == v for every v and j; every element finite; alternates beyond the distinct ones repeat the first;
    where some finite element of the value's group is a tie (t is exactly k + 0.5), the bank holds one."""
    bank = K.bank(kind, pair)
    x = TR.elements(kind, bank)
    assert bank.shape == (256, 4) and bank.dtype == TR.KINDS[kind]
    assert (TR.quantize(x, *pair) == np.arange(256, dtype=np.uint8)[:, None]).all()
    assert np.isfinite(TR.widen(x)).all()
    distinct = np.array([len(set(r.tolist())) for r in bank])
    for v in range(256):
        assert set(bank[v, distinct[v]:].tolist()) <= {int(bank[v, 0])}, v
    ties = TR._is_tie(TR.conversion_t(x, *pair)).any(axis=1)
    if kind != K.F32:
        allx = TR.elements(kind, np.arange(1 << 16, dtype=np.uint16))
        q, fin = TR.quantize(allx, *pair), np.isfinite(TR.widen(allx))
        has_tie = np.bincount(q[fin & TR._is_tie(TR.conversion_t(allx, *pair))], minlength=256) > 0
        assert (ties == has_tie).all()
        size = np.bincount(q[fin], minlength=256)
        assert (distinct >= np.minimum(size, 3)).all()      # smallest, largest, centre: all three where the group has them
    else:
        assert int(distinct.min()) >= 3 and int(ties.sum()) >= 120      # -0.49, 0, 0.49 everywhere; v -+ 0.5 is a tie of the even v
    print("%-8s x %g + %g: distinct elements per value %s (1, 2, 3, 4), values with a tie element %d"
          % (kind, pair[0], pair[1], np.bincount(distinct, minlength=5)[1:].tolist(), int(ties.sum())))


def test_bfloat16_misses_values_under_the_steep_pair():
    """The finding behind the pairs: bfloat16 has 8 significant bits, and under (-3.5, 300) the elements around 300 / 3.5 lie
    more than a pixel apart -- 224 of the 256 values are reached, and `preimages` refuses.  Every other (kind, pair) of two
    bytes reaches all 256."""
    assert len(TR.reachable(K.BF16, *K.PAIR_B)) == 224
    with pytest.raises(ValueError, match="no finite element converts to"):
        TR.preimages(K.BF16, *K.PAIR_B)
    for kind, pair in ((K.F16, K.PAIR_A), (K.F16, K.PAIR_B), (K.F16, UNUSED), (K.F16, (1.0, 0.0)), (K.BF16, K.PAIR_A), (K.BF16, UNUSED), (K.BF16, (1.0, 0.0))):
        assert len(TR.reachable(kind, *pair)) == 256, (kind, pair)


def test_a_lifted_frame_converts_back_to_its_design():
    """One whole design per kind and pair: the sub-1 quantizer design (every pixel value next to every prediction), a noise
    frame of the geometry sets with a batch, and the same frame narrowed -- the lift of a view is the view of the lift."""
    q1 = D.quant_frame("q1")
    noise = G.content(131, 66, batch=2)
    for kind, pair in K.TYPED_CHOICES:
        bank = K.bank(kind, pair)
        lifted = TR.lift(q1, bank, 5)
        assert lifted.dtype == TR.KINDS[kind] and lifted.shape == q1.shape
        assert (TR.quantize(TR.elements(kind, lifted), *pair) == q1).all()
        used = np.unique(TR.lift_columns(q1.shape[0], q1.shape[1], 4, 5), return_counts=True)
        assert used[0].tolist() == [0, 1, 2, 3] and used[1].min() > q1.size // 5      # every column of the bank, about evenly
        ln = TR.lift(noise, bank, 9)
        assert (TR.quantize(TR.elements(kind, ln), *pair) == noise).all()
        assert (TR.lift(noise[:, :, :129], bank, 9) == ln[:, :, :129]).all()
    assert (TR.lift(noise, K.bank(K.F16, K.PAIR_A), 1) != TR.lift(noise, K.bank(K.F16, K.PAIR_A), 2)).any()


def test_zero_element_outside_the_image_changes_exactly_the_shapes_it_applies_to():
    """`right`, `below`, `corner` with the pixel of the element 0.0 as their fill: Crossed, the identity table, R1 + R0 at 1 and
    4 levels and D at 8.  Under the two pairs of the typed family (fill 37 and 255) the encoder's grid changes on every shape
    the mutant applies to and on no other; under (255, 0) the fill is 0 and no grid changes."""
    fills = {pair: pixel_of_zero(pair) for pair in (K.PAIR_A, K.PAIR_B, UNUSED)}
    mutants = ("right", "below", "corner")
    rows = []
    for name, levels in (("R", 1), ("R", 4), ("D", 8)):
        counts = {(m, pair): [0, 0] for m in mutants for pair in fills}
        shapes = G.shape_set(name)
        for w, h in shapes:
            img = G.content(w, h)
            grid = G.encode_oob(img, levels, IDENT, 1)
            for m in mutants:
                want = G.applies(m, w, h, levels)
                for pair, fill in fills.items():
                    got = bool((G.encode_oob(img, levels, IDENT, 1, mutant=m, fill=fill) != grid).any())
                    assert got == (want and fill != 0), "%s with fill %d on %d x %d at %d levels: applies %s, grid changes %s" % (m, fill, w, h, levels, want, got)
                    counts[m, pair][0] += want
                    counts[m, pair][1] += got
        rows.append((name, levels, len(shapes), counts))
    print("mutant x pair: shapes whose grid changes / shapes the mutant applies to / shapes of the set")
    for name, levels, n, counts in rows:
        for pair, fill in fills.items():
            print("  %-2s L%d  x %g + %g (0.0 is pixel %3d)  " % (name, levels, pair[0], pair[1], fill)
                  + "  ".join("%s %d/%d/%d" % (m, counts[m, pair][1], counts[m, pair][0], n) for m in mutants))
    for name, levels, n, counts in rows:
        for m in mutants:
            assert counts[m, K.PAIR_A][1] == counts[m, K.PAIR_A][0] > n // 2 and counts[m, UNUSED][1] == 0


def test_every_typed_instantiation_meets_a_quantizer_and_a_predictor_design():
    """k_enc_typed<INTERP, IDENT, SEEDED, E> (rustyhgi_amd/typed/hgi_fused_typed_enc.hip): INTERP 0 / 1, IDENT -- the table is
    the identity --, SEEDED 2 at six to eight levels and 0 below, E 2 / 4: sixteen kernels.  From DESIGNS, the tables and the
    typed calls the operand suite makes: every one of them is given a quantizer design (every (p, a) pair in front of the
    quantizer step) and a predictor design (every corner quadruple in front of the packed averages); the narrowed calls reach
    both element sizes; every (kind, pair) of the suites is used."""
    import test_operand_coverage_gpu as OG
    met, narrowed, choices = {}, set(), set()
    for design, (frame, levels, _, _) in OG.DESIGNS.items():
        role = "predictor" if frame in D.PRED_FRAMES else "quantizer"
        for interp in (0, 1):
            for tname, E, kind, pair, also_narrowed in OG.typed_calls(design, interp):
                assert 1 <= levels <= 8 and K.ESIZE[kind] == E
                ident = bool((OG.TABLES_PLUS[tname] == IDENT).all())
                met.setdefault((interp, ident, 2 if levels >= 6 else 0, E), set()).add(role)
                choices.add((kind, pair))
                if also_narrowed:
                    narrowed.add((frame, interp, ident, E))
    every = [(i, ident, seeded, E) for i in (0, 1) for ident in (False, True) for seeded in (0, 2) for E in (2, 4)]
    assert len(every) == 16 and sorted(met) == sorted(every)
    for key in every:
        assert met[key] == {"quantizer", "predictor"}, (key, met[key])
    assert narrowed == {(f, i, ident, E) for f in ("q1", "q2") for i in (0, 1) for ident in (False, True) for E in (2, 4)}
    assert choices == set(K.TYPED_CHOICES)
    assert not OG.typed_calls("q8_16_L9", 1) and not OG.typed_calls("pred5_L12", 0)      # nine levels and more: refused by the ABI
    print("typed instantiations (INTERP, IDENT, SEEDED, E) with a quantizer and a predictor design: %d of 16" % len(met))
