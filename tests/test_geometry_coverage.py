"""What the ragged-tile code and the tile walk of the kernels are fed, measured on the shapes and on the reference alone (CPU;
nothing here touches the library).

The variant suites sample the ragged tile at five or six column remainders out of 127 and four row remainders out of 63.
tests/geometry_designs.py holds shape sets that put EVERY remainder in front of every kernel; this file asserts, from the shapes
alone, that they do (the class census), and -- with a restatement of oracle/hgi_numpy.py that is first shown to equal both oracles
bit for bit on the sets -- that five mutants of the out-of-image rule change the bytes on exactly the shapes they apply to.  The
uniform kernels' block -> tile walk (rustyhgi_amd/csrc/hgi_tilewalk.h) is walked by tests/cpp/test_tilewalk.cpp under ASan and
UBSan, and its census mode shows what the WALK cases of tests/test_tilewalk_gpu.py reach.  tests/test_geometry_coverage_gpu.py
and tests/test_tilewalk_gpu.py push the same shapes through every kernel.  Figures (run with -s):
profiles/r12_geometry_coverage.md."""
import os
import subprocess

import numpy as np
import pytest

import geometry_designs as G
from oracle import hgi_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.arange(256, dtype=np.uint8)
LINEAR2 = N.linear_lut(2)[0]


def test_the_sets_are_what_the_designs_say():
    r1, r0, d = G.shape_set("R1"), G.shape_set("R0"), G.shape_set("D")
    assert len(r1) == 128 * 4 + 64 * 4 - 16 and len(r0) == 128 * 2 + 64 * 2 - 4 and len(d) == 176
    assert len(G.shape_set("R")) == len(r1) + len(r0)
    assert max(w for w, h in r1 + r0) == 256 and max(h for w, h in r1 + r0) == 128
    assert all(w > 128 and h > 64 for w, h in r1) and all(w <= 128 and h <= 64 for w, h in r0)
    for w, h in ((1, 1), (256, 128), (129, 65), (428, 264)):
        c = G.content(w, h)
        assert c.shape == (h, w) and int(c.min()) >= 8
    assert int(G.filler(100000, 3).min()) >= 1
    # (the largest WALK case, 9 x 389 x 387, is 1.35 MB; all others are under 1 MiB)
    assert max(w * h * b for w, h, b in G.walk_cases()) == 9 * 389 * 387 and len(G.walk_cases()) == 600


@pytest.mark.parametrize("th", G.TILE_HEIGHTS)
def test_class_census_of_the_remainder_sets(th):
    """Every ragged tile of every shape of R1 and R0 under 128 x th tiles, classified from the shape alone.

    R1: every cols 1 ... 127 with a full-height tile, an even and an odd ragged `rows`; every rows 1 ... th - 1 with a
    full-width and with a ragged tile; all of them with an interior neighbour to the left (columns) and above (rows).
    R0: every cols with a full-height tile and with an odd ragged `rows` (its two heights are 64 and 37: the even ragged
    height is R1's), every rows with a full-width and with a ragged tile, under 64-row tiles never with an interior neighbour.
    EDGE: the kernels take EDGE == 1 for a tile whose full width lies inside a frame of even height, so that form exists at
    cols == 128 alone; asserted is that it meets every even ragged `rows`, and that EDGE == 2 meets every cols mod 16 under
    both parities of the height."""
    census = {}
    for name in ("R1", "R0"):
        tiles = [t for w, h in G.shape_set(name) for t in G.tile_classes(w, h, th)]
        census[name] = tiles
        col = {k: set() for k in ("full", "even", "odd")}
        row = {k: set() for k in ("full", "ragged")}
        for t in tiles:
            if t["cols"] < G.TW:
                col["full" if t["rows"] == th else "even" if t["rows"] % 2 == 0 else "odd"].add(t["cols"])
            if t["rows"] < th:
                row["full" if t["cols"] == G.TW else "ragged"].add(t["rows"])
        every_col, every_row = set(range(1, G.TW)), set(range(1, th))
        assert col["full"] == every_col and col["odd"] == every_col, (name, th)
        if name == "R1":
            assert col["even"] == every_col, th
        assert row["full"] == every_row and row["ragged"] == every_row, (name, th)
        classes = {(t["cols"], t["rows"], t["even"], t["left"], t["above"]) for t in tiles}
        print("%s, %2d-row tiles: %5d ragged tiles in %4d classes; cols x {full, even, odd rows}: %d / %d / %d of 127; rows x {full, ragged width}: %d / %d of %d"
              % (name, th, len(tiles), len(classes), len(col["full"]), len(col["even"]), len(col["odd"]), len(row["full"]), len(row["ragged"]), th - 1))
    r1 = census["R1"]
    assert {t["cols"] for t in r1 if t["cols"] < G.TW and t["left"]} == set(range(1, G.TW))
    assert {t["rows"] for t in r1 if t["rows"] < th and t["above"]} == set(range(1, th))
    if th == 64:
        assert not any(t["left"] or t["above"] for t in census["R0"])
    for name, tiles in census.items():
        for even in (True, False):
            assert {t["cmod"] for t in tiles if t["edge"] == 2 and t["even"] == even} == set(range(16)), (name, th, even)
        assert all(t["cols"] == G.TW and t["even"] for t in tiles if t["edge"] == 1)
        assert {t["rows"] for t in tiles if t["edge"] == 1} == set(range(2, th, 2)), (name, th)


def test_deep_set_moves_every_coarse_corner_across_the_edge():
    """D: for every pyramid of 6 ... 8 levels and every coarse step s = 16 ... 128 of it, the lattice column k * s next to the
    frame's right edge is the first column outside (W = k * s), one further out (W = k * s - 1) and the last one inside
    (W = k * s + 1) -- and the same for the rows."""
    shapes = G.shape_set("D")
    for levels in (6, 7, 8):
        for s in (16, 32, 64, 128):
            if s > 1 << levels:
                continue
            assert {s - 1, 0, 1} <= {w % s for w, h in shapes}, (levels, s)
            assert {s - 1, 0, 1} <= {h % s for w, h in shapes}, (levels, s)
            assert {(w % s, h % s) for w, h in shapes} >= {(a, b) for a in (s - 1, 0, 1) for b in (s - 1, 0, 1)}, (levels, s)
    print("D: %d shapes; W mod s and H mod s take s - 1, 0 and 1 in every combination for s = 16, 32, 64, 128" % len(shapes))


def _both_oracles(oracle, img, levels, lut, interp):
    grid = G.encode_oob(img, levels, lut, interp)
    assert (grid == oracle.encode(img, levels, lut, interp)).all() and (grid == N.encode(img, levels, lut, interp)).all()
    out = G.decode_oob(grid, levels, interp)
    assert (out == oracle.decode(grid, levels, interp)).all() and (out == N.decode(grid, levels, interp)).all()
    return grid, out


def test_restatement_equals_both_oracles_on_the_sets(oracle):
    """Every shape of R1 and R0 at 1 and 4 levels (Crossed, the identity and linear_lut(2); LeftTop at 4 levels), every shape
    of D at 6, 8 and 12 levels: encode and decode of the restatement against the C oracle and the numpy oracle."""
    n = 0
    for w, h in G.shape_set("R"):
        img = G.content(w, h)
        for levels in (1, 4):
            grid, out = _both_oracles(oracle, img, levels, IDENT, 1)
            assert (out == img).all()
        _both_oracles(oracle, img, 4, LINEAR2, 1)
        _both_oracles(oracle, img, 4, IDENT, 0)
        n += 4
    for w, h in G.shape_set("D"):
        img = G.content(w, h)
        for levels, lut in ((6, LINEAR2), (8, IDENT), (12, LINEAR2)):
            _both_oracles(oracle, img, levels, lut, 1)
            n += 1
    print("restatement == C oracle == numpy oracle on %d (shape, levels, table, interpolator) cases, both directions" % n)


def test_mutants_of_the_out_of_image_rule_change_exactly_the_shapes_they_apply_to():
    """`right`, `below`, `corner`: corners at x >= W, at y >= H, beyond both read 0xC3; `last_col`, `last_row`: a corner at
    x == W - 1, at y == H - 1 reads 0.  Under Crossed and the identity table, at 1 and 4 levels on R1 and R0 and at 8 levels
    on D: the mutant changes the encoder's grid AND the decoder's output on every shape it applies to (geometry_designs.applies:
    it alters a corner of a cell that holds a new in-image pixel) and on no other."""
    rows = []
    for name, levels in (("R1", 1), ("R1", 4), ("R0", 1), ("R0", 4), ("D", 8)):
        counts = {m: [0, 0] for m in G.OOB_MUTANTS}
        shapes = G.shape_set(name)
        for w, h in shapes:
            img = G.content(w, h)
            grid = G.encode_oob(img, levels, IDENT, 1)
            for m in G.OOB_MUTANTS:
                want = G.applies(m, w, h, levels)
                enc = bool((G.encode_oob(img, levels, IDENT, 1, mutant=m) != grid).any())
                dec = bool((G.decode_oob(grid, levels, 1, mutant=m) != img).any())
                assert enc == want and dec == want, "%s on %d x %d at %d levels: applies %s, encoder changes %s, decoder changes %s" % (m, w, h, levels, want, enc, dec)
                counts[m][0] += want
                counts[m][1] += enc and dec
        rows.append((name, levels, len(shapes), counts))
    print("mutant x set: shapes the mutant applies to = shapes whose grid and decode change / shapes of the set")
    for name, levels, n, counts in rows:
        print("  %-3s L%d  " % (name, levels) + "  ".join("%s %d=%d/%d" % (m, counts[m][0], counts[m][1], n) for m in G.OOB_MUTANTS))
    for name, levels, n, counts in rows:
        for m in G.OOB_MUTANTS:
            assert 0 < counts[m][0], (name, levels, m)
    # where it does not apply although the lattice holds such a corner: the one-pixel frame (its only cell has no new pixel),
    # and the far corner when both sizes are odd
    assert not G.applies("right", 1, 1, 4) and not G.applies("below", 1, 1, 4) and not G.applies("corner", 67, 37, 1)
    assert not G.applies("last_col", 1, 1, 1) and G.applies("last_col", 1, 2, 1) and not G.applies("last_row", 1, 1, 1)
    assert G.applies("corner", 68, 37, 1) and G.applies("right", 2, 37, 1) and G.applies("right", 1, 37, 4)


# ----------------------------------------------------------------------------------------------- the tile walk
@pytest.fixture(scope="module")
def tilewalk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tilewalk") / "test_tilewalk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_tilewalk.cpp"), "-o", exe])
    return exe


def test_tile_walk_under_asan_ubsan(tilewalk):
    """tests/cpp/test_tilewalk.cpp: the exhaustive small grids, the order promises and 200 000 large grids against plain 64-bit
    division (see the file's head for what it checks)."""
    p = subprocess.run([tilewalk, "200000", "0x4847493a"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and ", 0 failures" in p.stdout and "200000 large grids" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    print(p.stdout.strip())


WALK_MODES = [(1, 1), (2, 1), (3, 1), (4, 1), (3, 0)]          # (forced band, xmode) of the children of tests/test_tilewalk_gpu.py


def test_walk_census_of_the_walk_cases(tilewalk, tmp_path):
    """What the WALK cases reach under 16-row tiles and every forced band: launches that deal whole rounds of eight bands with
    and without a tail behind them, launches of fewer than eight bands under xmode 1, launches that fall back to contiguous
    eighths because a frame's rows leave a shorter last band, and that shorter band at every height 1 ... band - 1."""
    cases = tmp_path / "walk_cases.txt"
    cases.write_text("".join("%d %d %d\n" % c for c in G.walk_cases()))
    for band, xmode in WALK_MODES:
        p = subprocess.run([tilewalk, "--census", str(cases), "16", str(band), str(xmode)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        got = dict(kv.split("=") for kv in p.stdout.split() if "=" in kv)
        print("band %d xmode %d: %s" % (band, xmode, p.stdout.strip()))
        assert int(got["launches"]) == len(G.walk_cases()) and int(got["interior"]) > 0
        assert {int(v) for v in got["rem_rows"].split(",") if v} >= set(range(1, band)), (band, got["rem_rows"])
        if xmode == 1:
            assert int(got["rr_tail"]) > 0 and int(got["rr_no_tail"]) > 0 and int(got["rr_none"]) > 0, (band, got)
            assert band == 1 or int(got["fallback_rem"]) > 0, (band, got)
        else:
            assert int(got["rr_tail"]) == 0 and int(got["rr_no_tail"]) == 0 and int(got["xmode0"]) == int(got["interior"])
