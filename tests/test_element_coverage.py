"""What the element-coverage designs cover, measured on the reference alone (CPU; nothing here touches the library).

tests/test_element_coverage_gpu.py puts rotation batches of float16 / bfloat16 / float32 frames (tests/element_designs.py)
through hgi_typed_encode_dev and compares the grids with the oracle's.  Whether such a batch can tell a wrong conversion from the
right one -- at every site the kernel converts at -- is a property of the designs, asserted here:

1. the twin: element_designs.convert without a mutant IS typed_reference.quantize; fma32 is the exact single rounding;
2. the banks: every class of element_designs.CLASSES is present for every kind, every element's stated pixel is quantize's and
   has the property its class names; for every kind, pair and mutant either some bank element changes its pixel, or the mutant
   is exempt with a proof, and the proof's claim is checked on every 16-bit pattern;
3. the rotation: every position meets every bank element once over the batch;
4. the sites: which of them reach a tile's grid at all, per interpolator and table -- computed, then asserted: LeftTop reads its
   own rows and the cone only; a lossless table only what predicts the tile's own pixels; odd columns of a halo row nothing;
5. the census: under Crossed, for the lossy table of the non-IDENT kernels and for the identity of the IDENT kernels, every
   site live under the table x every non-exempt mutant is killed on an interior tile and, where a ragged tile has the site, on
   a ragged tile -- by the union of the kind's pairs, as the GPU module runs all of them on every instantiation; a design without its fma elements, and a frame of one tile, fail it;
6. the table (instantiation -> kinds, pairs, levels, tables) the GPU module iterates over.
Figures (run with -s): profiles/r18_element_coverage.md."""
import math

import numpy as np
import pytest

import element_designs as E
import typed_reference as TR

LEVELS_FULL, LEVELS_CONE = (5, 8), (6, 7)


def all_patterns(kind):
    return E._candidates(kind, *E.f32pair("fma")) if kind == E.F32 else np.arange(1 << 16, dtype=np.uint16)


def t_of(kind, bits, pname):
    return TR.conversion_t(TR.elements(kind, np.atleast_1d(np.asarray(bits, TR.KINDS[kind]))), *E.f32pair(pname))


# ----------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("kind", E.KINDS)
def test_the_twin_is_the_reference(kind):
    """convert(mutant=None) == typed_reference.quantize: all 65 536 patterns of the 2-byte kinds, the search pool of float32,
    under every pair."""
    for pname in E.KIND_PAIRS[kind]:
        scale, bias = E.f32pair(pname)
        bits = all_patterns(kind) if kind != E.F32 else E._candidates(kind, scale, bias)
        assert (E.convert(kind, bits, scale, bias) == TR.quantize(TR.elements(kind, bits), scale, bias)).all(), pname


def test_the_single_rounding_is_exact():
    """fma32 (float64 two-sum, fractions where the sum lies half way) against fma32_exact (fractions alone): the issue's
    example 44.5 * 0.1 + 0.05 -- 5 under the contract, 4 under an fma --, every bank element, every float32 tie pre-image
    under (0.1, 0.05) and its +-40 ulp, and seeded random patterns under every pair."""
    x = np.array([44.5], np.float32)
    assert TR.quantize(x, 0.1, 0.05)[0] == 5 and E.convert(E.F32, x.view(np.uint32), *E.f32pair("fma"), "fma")[0] == 4
    assert float(E.fma32_exact(44.5, np.float32(0.1), np.float32(0.05))) == 4.5 < float(np.float32(44.5) * np.float32(0.1) + np.float32(0.05))      # a tie, to even
    assert E.round_fraction_to_f32(E.fractions.Fraction(1, 3)) == np.float32(1 / 3)
    assert E.round_fraction_to_f32(E.fractions.Fraction(2) ** 128) == np.inf and E.round_fraction_to_f32(E.fractions.Fraction(2) ** -150) == 0
    assert E.round_fraction_to_f32(3 * E.fractions.Fraction(2) ** -150) == np.float32(2.0 ** -148)      # a denormal tie, to even
    rng = np.random.default_rng(0x48474960)
    checked = 0
    for pname in E.PAIRS:
        scale, bias = E.f32pair(pname)
        pool = [rng.integers(0, 1 << 32, 1500, dtype=np.uint64).astype(np.uint32)]
        pool += [E.bank(E.F32, pname)[1].astype(np.uint32)] if pname in E.KIND_PAIRS[E.F32] else []
        if pname == "fma":
            pool.append(E._candidates(E.F32, scale, bias)[::7])
        xs = np.concatenate(pool).view(np.float32)
        fast = E.fma32(xs, scale, bias)
        slow = np.array([E.fma32_exact(v, scale, bias) for v in xs], np.float32)
        same = (fast == slow) | (np.isnan(fast) & np.isnan(slow))
        assert same.all(), (pname, xs[~same][:4])
        checked += xs.size
    # the fallback itself: a sum that lies exactly half way in float64 with a nonzero error term
    x, s, b = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** 30)
    assert E.fma32(np.array([x]), s, b)[0] == E.fma32_exact(x, s, b)
    print("fma32 == fma32_exact on %d elements" % checked)


# ---------------------------------------------------------------------------------------------------- the banks
@pytest.mark.parametrize("kind", E.KINDS)
def test_the_banks_hold_their_classes(kind):
    """Every class is present under some pair of the kind; under every pair the stated pixel is quantize's, the size is a prime
    (any rotation constants are coprime to it) and every named element has the property of its class."""
    present = set()
    for pname in E.KIND_PAIRS[kind]:
        scale, bias = E.f32pair(pname)
        names, bits, pixels = E.bank(kind, pname)
        n = len(names)
        assert n == bits.size == pixels.size and all(n % p for p in range(2, n)) and n <= 41
        assert (pixels == TR.quantize(TR.elements(kind, bits), scale, bias)).all()
        present |= set(names)
        x = TR.widen(TR.elements(kind, bits))
        t = t_of(kind, bits, pname)
        zero_px = int(TR.quantize(np.zeros(1, np.float32), scale, bias)[0])
        with np.errstate(all="ignore"):
            frac, fl, m = t - np.floor(t), np.floor(t), x * np.float32(scale)
        for i, name in enumerate(names):
            if name.startswith("tie_down") and name[8:] in ("", "2", "3", "4"):
                assert frac[i] == 0.5 and fl[i] % 2 == 0 and pixels[i] == fl[i] and np.isfinite(x[i]), (pname, name)
            elif name == "tie_up":
                assert frac[i] == 0.5 and fl[i] % 2 == 1 and pixels[i] == fl[i] + 1, (pname, name)
            elif name.endswith("_below") or name.endswith("_above"):
                j = names.index(name[:-6])
                step = 1 if name.endswith("_above") else -1      # the nearest element on that side whose t is not the tie's
                assert (int(bits[i]) - int(bits[j])) * step >= 1 and np.isfinite(x[i]) and t[i] != t[j]
                assert t_of(kind, int(bits[i]) - step, pname)[0] == t[j]
            elif name == "negative":
                assert np.isfinite(x[i]) and -200 <= t[i] <= -1.5 and pixels[i] == 0
            elif name == "over":
                assert np.isfinite(x[i]) and np.isfinite(t[i]) and t[i] > 256.5 and pixels[i] == 255
            elif name in ("pinf", "ninf"):
                assert np.isinf(x[i]) and (x[i] > 0) == (name == "pinf")
                assert pixels[i] == (0 if scale == 0 else 255 if (x[i] > 0) == (scale > 0) else 0)      # scale 0: NaN
            elif name in ("qnan", "snan", "negnan"):
                assert np.isnan(x[i]) and pixels[i] == 0
            elif name in ("pzero", "nzero"):
                assert x[i] == 0 and bool(np.signbit(x[i])) == (name == "nzero") and pixels[i] == zero_px
            elif name.startswith("denormal"):
                assert int(bits[i]) & E.EXP_MASK[kind] == 0 and x[i] != 0 and abs(m[i]) >= 0.5 and pixels[i] >= 1
            elif name in ("overflow_pos", "overflow_neg"):
                assert np.isfinite(x[i]) and np.isinf(m[i]) and pixels[i] == (255 if name == "overflow_pos" else 0)
            elif name == "finite_tie":
                assert scale == 0 and t[i] == 36.5 and pixels[i] == 36
            elif name.startswith("fma"):
                assert E.convert(kind, bits[i:i + 1], scale, bias, "fma")[0] != pixels[i]
                tx = E.fma32_exact(x[i], scale, bias)      # ... under the exact single rounding
                assert int(np.clip(np.rint(tx), 0, 255)) != pixels[i], (pname, name)
            else:
                assert name.startswith("ordinary") and np.isfinite(x[i])
        if scale != 0 and not (kind == E.F16 and pname == "den127"):
            assert len(set(pixels.tolist())) >= 10, pname      # frames are not all 0 / 255
    assert present >= set(E.CLASSES), sorted(set(E.CLASSES) - present)


@pytest.mark.parametrize("kind", E.KINDS)
def test_every_mutant_is_killed_or_provably_the_contract(kind):
    """For every pair and mutant: not exempt -> some bank element's pixel changes; exempt -> the proof is named, no bank element
    changes, and for the 2-byte kinds the mutant equals the contract on all 65 536 patterns (float32: on the search pool).
    Every mutant is killed under at least one pair of the kind, unless it does not apply to the kind at all."""
    killed_somewhere = set()
    for pname in E.KIND_PAIRS[kind]:
        scale, bias = E.f32pair(pname)
        names = E.bank(kind, pname)[0]
        bits = all_patterns(kind) if kind != E.F32 else E._candidates(kind, scale, bias)
        want = TR.quantize(TR.elements(kind, bits), scale, bias)
        for m in E.MUTANTS:
            proof = E.exemption(m, kind, pname)
            k = E.kills(kind, pname, m)
            if proof is None:
                assert k.size, "%s under %s: %s survives the bank" % (kind, pname, m)
                killed_somewhere.add(m)
            else:
                assert isinstance(proof, str) and len(proof) > 20 and k.size == 0
                assert (E.convert(kind, bits, scale, bias, m) == want).all(), "%s under %s: the exemption of %s is wrong" % (kind, pname, m)
            print("%-8s %-6s %-22s %s" % (kind, pname, m, "exempt: " + proof if proof else "killed by " + ", ".join(names[i] for i in k)))
    not_applicable = {E.F16: {"ftz_input"}, E.BF16: {"f16_denormal_flushed"}, E.F32: {"f16_denormal_flushed", "kind_swapped"}}[kind]
    assert killed_somewhere == set(E.MUTANTS) - not_applicable


def test_the_issue_figures_for_the_old_pairs():
    """Why the new pairs: under the pairs the suite had, and (1, 0), a single rounding is the contract for every 16-bit
    pattern (the products are exact); under (0.1, 0.05) it is not."""
    for kind in (E.F16, E.BF16):
        bits = all_patterns(kind)
        for pair in TR.PAIRS + ((1.0, 0.0),):
            assert (E.convert(kind, bits, *pair, "fma") == E.convert(kind, bits, *pair)).all()
        assert int((E.convert(kind, bits, *E.f32pair("fma"), "fma") != E.convert(kind, bits, *E.f32pair("fma"))).sum()) == {E.F16: 21, E.BF16: 2}[kind]


# ------------------------------------------------------------------------------------------------- the rotation
def test_every_position_meets_every_element():
    """Frame f holds element (a x + b y + f) mod n at (x, y): over the n frames every position holds every element once,
    and horizontal and vertical neighbours never hold the same one."""
    w, h = E.SHAPE
    assert w * h < 65536 and w % 2 and w % 16 and w // E.TW == 2 and h // E.TH == 2 and h % 2 and 0 < h % E.TH < E.TH
    for n in sorted({len(E.bank(kind, p)[0]) for kind in E.KINDS for p in E.KIND_PAIRS[kind]}):
        assert math.gcd(E.ROT[0], n) == 1 and math.gcd(E.ROT[1], n) == 1
        base = E.rotation_index(w, h, n)
        idx = (base[None] + np.arange(n)[:, None, None]) % n
        assert (np.sort(idx, axis=0) == np.arange(n)[:, None, None]).all()
        assert (base[:, 1:] != base[:, :-1]).all() and (base[1:] != base[:-1]).all()
    bits, px = E.rotation(E.BF16, "A")
    names, bank_bits, bank_px = E.bank(E.BF16, "A")
    assert bits.shape == px.shape == (len(names), h, w) and bits.dtype == np.uint16 and px.dtype == np.uint8
    assert (px == TR.quantize(bits, *E.f32pair("A"))).all() and bits[3, 7, 11] == bank_bits[(5 * 11 + 3 * 7 + 3) % len(names)]


# ---------------------------------------------------------------------------------------------------- the sites
def test_the_sites_restate_the_read_set():
    """Counts that follow from the file header of hgi_fused_typed_enc.hip for the design's shape: four interior tiles and five
    ragged ones; the own rows of an interior tile are 128 x 32 positions, 256 per byte lane; the halo rows are TH + 0, 4, 8,
    16, 32 for five levels; the +16 / +32 singles sit on the rows that are multiples of 16 / 32; no position is read through the
    +64 single at any depth the launch serves (six levels in one tile never happen: the cone takes over); the cone's points
    lie on the stride-16 lattice outside the tile's own 10 x 6 frame."""
    w, h = E.SHAPE
    for levels in range(1, 9):
        st = E.sites(w, h, levels)
        assert len(st) == 9 and sorted(t for t, (ragged, _) in st.items() if not ragged) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        k, up = E.split_levels(levels)
        for txy, (ragged, s) in st.items():
            assert ("hcol", 64) not in s
            assert set(s) <= set(E.site_classes(levels))
            for key, (ys, xs) in s.items():
                assert (ys < h).all() and (xs < w).all() and ((ys >= txy[1] * 64).all() or key == ("cone",))
                if key[0] in ("even", "odd", "hrow"):
                    assert ((xs - txy[0] * 128) % 16 == key[1]).all()
                if levels <= 5:
                    x0, y0, x1, y1 = E.window(w, h, levels, txy)
                    assert (xs >= x0).all() and (xs < x1).all() and (ys >= y0).all() and (ys < y1).all()
            if not ragged:
                assert all(len(s["even", lane][0]) == 256 == len(s["odd", lane][0]) for lane in range(16))
    s5 = E.sites(w, h, 5)[0, 0][1]
    assert sorted(set(s5["hrow", 0][0].tolist())) == [64, 68, 72, 80, 96]
    assert list(zip(*s5["hcol", 32])) == [(0, 160), (32, 160), (64, 160), (96, 160)]
    assert sorted(set(s5["hcol", 16][0].tolist())) == [0, 16, 32, 48, 64, 80, 96] and len(s5["hcol", 0][0]) == 32 + 5
    assert ("cone",) not in s5 and ("hcol", 32) not in E.sites(w, h, 8)[0, 0][1]
    c6, c8 = set(zip(*E.sites(w, h, 6)[0, 0][1]["cone",])), set(zip(*E.sites(w, h, 8)[0, 0][1]["cone",]))
    assert c6 < c8 and (0, 256) in c8 - c6 and (0, 160) in c6 and all(y % 16 == 0 and x % 16 == 0 and (x >= 160 or y >= 96) for y, x in c8)
    ragged_have = {key for ragged, s in E.sites(w, h, 5).values() if ragged for key in s}
    assert ragged_have == set(E.site_classes(5)) - {("hcol", 64)}      # some ragged tile has every site


def live_sites(levels, interp, tname):
    """The (site, ragged) pairs whose positions reach the tile's grid at all: every position of the site inverted (v ^ 255), four
    frames of the float32 batch under A."""
    names, bits, px = E.bank(E.F32, "A")
    n = len(names)
    _, ref = E.rotation(E.F32, "A")
    k = E.census(ref, E.rotation_index(*E.SHAPE, n), n, px ^ np.uint8(255), np.arange(n), levels, interp, E.tables()[tname], frames=range(4))
    return set(k)


def dead_by_rule(levels, interp, tname):
    """What the codec's rules say never reaches the tile's grid.
    - An odd column of an (even) halo row is a pixel of the finest level, which predicts nothing.
    - LeftTop predicts from the left top corner, which never lies right of or below the tile: its halo rows and columns are dead.
      Of the cone it reads the points above and left of the tile that are left top corners of the tile's own pixels of the
      levels above it.
    - Under a lossless table the reconstruction is the image, so only what predicts the tile's own pixels directly is live: the
      halo row and halo column at +0, and the cone's points that are corners of the tile's own pixels.  What serves to
      reconstruct those is not: the halo columns beyond +0 (the halo rows beyond +0 share their site with +0).
      identity_but_255 is lossless except at one residual, and is held to the lossy list.
    - The cone at six levels (up = 2) under a lossless table or LeftTop: the tile's own pixels above its four levels are new
      at steps 64 and 32, whose cells start on multiples of 64 and have their corners at most 64 columns and rows away:
      inside the 160 x 96 frame the tile stages for itself.  No point outside that frame is a corner of a pixel of the tile, so
      what the up = 2 cone converts reaches the grid only through a lossy reconstruction under Crossed.  From seven levels on
      the cells of step 128 reach outside the frame."""
    dead = set()
    for key, ragged in E.available(levels):
        if key[0] in ("even", "odd"):
            continue
        if key[0] == "cone":
            if levels == 6 and (interp == E.LEFTTOP or tname == "identity"):
                dead.add((key, ragged))
        elif interp == E.LEFTTOP or (key[0] == "hrow" and key[1] % 2) or (tname == "identity" and key[0] == "hcol" and key[1] != 0):
            dead.add((key, ragged))
    return dead


@pytest.mark.parametrize("interp,tname", [(E.CROSSED, "random0"), (E.CROSSED, "identity"), (E.LEFTTOP, "random0"), (E.LEFTTOP, "identity")])
def test_which_sites_reach_the_grid(interp, tname):
    """Computed, then compared with the rules: the live sites are exactly the available ones minus dead_by_rule."""
    for levels in (5, 6, 7, 8):
        av = E.available(levels)
        live = live_sites(levels, interp, tname)
        dead = dead_by_rule(levels, interp, tname)
        assert live == av - dead, (levels, sorted(live ^ (av - dead)))
        print("levels %d interp %d %-8s: %d of %d (site, tile class) pairs live; dead: %s" % (levels, interp, tname, len(live), len(av),
              sorted({k[0] if k[0] != "hrow" else "hrow odd lanes" for k, _ in dead}, key=str)))


# --------------------------------------------------------------------------------------------------- the census
def census_rows(kind, shape=E.SHAPE, drop=(), mutants=E.MUTANTS, tname="random0"):
    """{(mutant, levels, site, ragged): [pairs that kill it]} under Crossed and the table, over the sites live under it: levels 5 and 8 with
    every site, 6 and 7 with the cone.  Mutants whose pixels are the same over a bank share their census.  `drop`: class
    name prefixes left out of the banks (the self-check)."""
    lut = E.tables()[tname]
    rows = {}
    for pname in E.KIND_PAIRS[kind]:
        names, bits, px = E.bank(kind, pname)
        keep = np.array([not any(nm.startswith(d) for d in drop) for nm in names])
        n = len(names)
        index = E.rotation_index(shape[0], shape[1], n)
        ref = px[(index[None] + np.arange(n)[:, None, None]) % n]
        done = {}
        for m in mutants:
            if E.exemption(m, kind, pname) is not None:
                continue
            mp = np.where(keep, E.convert(kind, bits, *E.f32pair(pname), m), px)
            for levels in LEVELS_FULL + LEVELS_CONE:
                live = E.available(levels, shape) - dead_by_rule(levels, E.CROSSED, tname)
                if levels in LEVELS_CONE:
                    live = {(key, r) for key, r in live if key[0] == "cone"}
                sig = (mp.tobytes(), levels)
                if sig not in done:
                    done[sig] = E.census(ref, index, n, mp, np.flatnonzero(mp != px), levels, E.CROSSED, lut, shape=shape, want=live)
                for key, ragged in live:
                    rows.setdefault((m, levels, key, ragged), [])
                    if (key, ragged) in done[sig]:
                        rows[m, levels, key, ragged].append(pname)
    return rows


@pytest.mark.parametrize("tname", ["random0", "identity"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_every_site_kills_every_mutant(kind, tname):
    """Crossed, under random0 (the lossy table of the non-IDENT kernels) and under the identity (the only table of the eight
    IDENT kernels): every site class that is live under the table x every mutant the kind has is killed on an interior tile
    and, where a ragged tile has the site, on a ragged one, at five and eight levels; the cone also at six and seven (up = 2,
    3) where it is live.  Killed means: by the batch of at least one pair of the kind -- the GPU module runs every pair on
    every instantiation.  A pair that kills a mutant in its bank but misses it at a site is counted; under random0 that
    happens only at the sites of a few positions per tile (the halo-column singles, the cone)."""
    rows = census_rows(kind, tname=tname)
    wanted = {(lv, key, r) for lv in LEVELS_FULL for key, r in E.available(lv)} | {(lv, ("cone",), r) for lv in LEVELS_CONE for r in (False, True)}
    wanted = {(lv, key, r) for lv, key, r in wanted if (key, r) not in dead_by_rule(lv, E.CROSSED, tname)}
    assert {(lv, key, r) for _, lv, key, r in rows} == wanted
    assert {m for m, _, _, _ in rows} == {m for m in E.MUTANTS if any(E.exemption(m, kind, p) is None for p in E.KIND_PAIRS[kind])}
    unkilled = sorted(k for k, v in rows.items() if not v)
    assert not unkilled, unkilled
    weak = {}
    for (m, levels, key, ragged), pairs in rows.items():
        for p in E.KIND_PAIRS[kind]:
            if E.exemption(m, kind, p) is None and p not in pairs:
                assert tname == "identity" or key[0] in ("hcol", "cone"), (m, levels, key, ragged, p)
                weak.setdefault((key[0], ragged), []).append((m, levels, key, p))
    print("%s %s: %d (mutant, levels, site, tile class) rows, all killed; (row, pair) misses: %s" % (kind, tname, len(rows), {k: len(v) for k, v in sorted(weak.items())}))


def test_an_inadequate_design_fails_the_census():
    """The self-check.  The float32 banks without the elements that tell an fma leave the mutant `fma` alive at every site, which the
    banks as they are kill at every site; a frame cut
    to one tile has no halo row, no halo column and no cone, so its census lacks those rows whatever the bank."""
    killers = set()
    for p in E.KIND_PAIRS[E.F32]:
        if E.exemption("fma", E.F32, p) is None:
            killers |= {E.bank(E.F32, p)[0][i] for i in E.kills(E.F32, p, "fma")}
    assert any(nm.startswith("fma") for nm in killers)
    full = census_rows(E.F32, mutants=("fma",))
    assert full and all(full.values())
    rows = census_rows(E.F32, drop=tuple(sorted(killers)), mutants=("fma",))
    assert set(rows) == set(full) and not any(rows.values())
    one_tile = E.available(5, (128, 64)) | E.available(8, (128, 64))
    assert {key[0] for key, _ in one_tile} == {"even", "odd"} and not any(ragged for _, ragged in one_tile)


# ------------------------------------------------------------------------------- the table of the GPU module
def test_the_instantiation_table():
    """k_enc_typed<INTERP, IDENT, SEEDED, E>: sixteen kernels.  Each gets every kind its E serves under every pair of the kind;
    SEEDED 0 at five levels, SEEDED 2 at eight and at six (2-byte kinds) or seven (float32), so up = 2, 3 and 4 are all met;
    IDENT under the identity, the others under identity_but_255 and the lossy random0.  The GPU module's cases are this table
    expanded, no more and no less; every call is within the contract (finite scale and bias, one to eight levels)."""
    import test_element_coverage_gpu as G
    table = E.instantiations()
    assert len(table) == 16 and set(table) == {(i, d, s, e) for i in (0, 1) for d in (False, True) for s in (0, 2) for e in (2, 4)}
    ups = {}
    for (interp, ident, seeded, esz), (kinds, levels, tnames) in table.items():
        assert kinds == ((E.F16, E.BF16) if esz == 2 else (E.F32,))
        for lv in levels:
            k, up = E.split_levels(lv)
            assert (up > 0) == (seeded == 2)
            for kind in kinds:
                ups.setdefault(up, set()).add(kind)
        for t in tnames:
            assert bool((E.tables()[t] == np.arange(256)).all()) == ident
    assert set(ups) == {0, 2, 3, 4} and ups[4] == set(E.KINDS) and ups[0] == set(E.KINDS) and ups[2] and ups[3]
    want = [(i, d, s, e, kind) for (i, d, s, e), (kinds, _, _) in sorted(table.items()) for kind in kinds]
    assert G.CASES == want and len(want) == 24
    for i, d, s, e, kind in G.CASES:
        calls = G.calls_of(i, d, s, e, kind)
        assert {p for p, _, _ in calls} == set(E.KIND_PAIRS[kind]) and {lv for _, lv, _ in calls} == set(table[i, d, s, e][1])
        assert {t for _, _, t in calls} == set(table[i, d, s, e][2])
        assert all(np.isfinite(E.f32pair(p)).all() and 1 <= lv <= 8 for p, lv, _ in calls)
    assert set(G.COMPOSED) == {(kind, p) for kind in E.KINDS for p in E.KIND_PAIRS[kind]}
