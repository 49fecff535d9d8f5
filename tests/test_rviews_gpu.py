"""GPU suite of the recon view lists (libhgi_rviews.so, include/hgi_rviews.h; Encoder.encode_views_with_reconstruction): every
case reads its source images -- random bytes -- out of a parent of random bytes and writes into TWO sentinel-filled parents, one
for the grids and one for the reconstructions, that are each compared WHOLE against an expected parent built on the CPU from the
oracle,
    grid  = oracle.encode(img, levels, lut, interp)          recon = oracle.decode(grid, levels, interp),
computed once per (shape, variant, levels, interp, table) -- never from libhgi_hip.so, never from a library under test; the
source parent must come back unmodified.
  1. the mixed list of tests/test_views_gpu.py in separate parents (degenerate sides, ragged only, interior only, mixes, skipped
     entries), gaps drawn independently for each of the three sides, bases at odd addresses and on 128-B lines: levels 1-5 x both
     interpolators x {identity, Medium, a random table}; the same on the sub-lists that change the block map: ragged only,
     interior only, one entry;
  2. the cone: levels 6, 7, 8 on five shapes at two pitches under Medium and identity -- the SEEDED = 2 kernels;
  3. an atlas: the sources side by side in one 1024-byte-pitch canvas, two of them overlapping; grids AND reconstructions side by
     side, in another order, in ONE 1152-byte-pitch output canvas, window origins on 128-B lines, 64 B into a line and at odd x;
  4. one plan launched twice on new contents, then captured into a graph (which writes nothing) and replayed on new contents;
  5. the Python surface: ReconViewPlan on an aligned_arena with an empty entry; the composed route at scale_level 9 and of a list
     with one entry that breaks the page rule; the identity table;
  6. one call per kernel instantiation: 8 calls, each on a list with an interior, an EDGE == 1 and an EDGE == 2 tile;
  7. levels 0 and 9 are refused, with both output parents untouched;
  8. the closure property: hgi_views_decode_dev on the written grid views gives the reconstruction arena."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import SEED0

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1, 4      # hgi_status (include/hgi.h)
GAPS = (0, 1, 3, 16, 61, 128)
SENTINEL = 0xA5
# (width, height): the list of case 1
MIXED = [(1, 1), (1, 70), (200, 1), (127, 63), (128, 64), (129, 65), (0, 5), (256, 128), (255, 129), (7, 0), (384, 64), (128, 192),
         (130, 66), (301, 203), (513, 130)]
CONE = [(300, 200), (513, 257), (64, 64), (1, 300), (257, 1)]
GRID, RECON = 1, 2      # the sides of an entry behind the source (0)


@pytest.fixture(scope="module")
def R():
    """The binding of libhgi_rviews.so."""
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("rviews")


def content(w, h, variant=0):
    """The bytes of a (h, w) source image: random, a function of the shape and the variant alone, so that a reference is computed
    once for every list that holds the view."""
    return np.random.default_rng(SEED0 + 260000 + 7919 * w + 31 * h + 1000003 * variant).integers(0, 256, (h, w), dtype=np.uint8)


def tables(oracle):
    return {"identity": oracle.noop_lut(), "medium": oracle.linear_lut(oracle.MEDIUM)[0],
            "random": np.random.default_rng(SEED0 + 2600).integers(0, 256, 256, dtype=np.uint8)}


_REF = {}


def reference(oracle, src, key, levels, interp, lut_name):
    """(oracle.encode(src), oracle.decode of that grid) under the named table, computed once per key."""
    k = (key, levels, interp, lut_name)
    if k not in _REF:
        grid = oracle.encode(np.ascontiguousarray(src), levels, tables(oracle)[lut_name], interp)
        recon = oracle.decode(grid, levels, interp)
        grid.setflags(write=False)
        recon.setflags(write=False)
        _REF[k] = (grid, recon)
    return _REF[k]


def tail_ok(ptr, w, h, pitch):
    end = ptr + (h - 1) * (pitch if h > 1 else w) + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


def window(parent, off, w, h, pitch):
    return np.lib.stride_tricks.as_strided(parent[off:], (h, w), (pitch, 1))


class Parents:
    """A list of (w, h) views placed in a source parent of random bytes and two output parents of sentinel bytes (grids,
    reconstructions): view i at an odd address (odd i) or on a 128-byte line (even i), its rows `w + gap` bytes apart with a gap
    drawn per side; source offsets are advanced until the page rule holds (`paged`: the sides it is kept on -- the closure
    test reads the grids back through the view lists, which have the rule on what they read)."""

    def __init__(self, F, shapes, seed, gaps=None, variant=0, paged=(0,)):
        import torch
        self.F, self.shapes = F, list(shapes)
        rng = np.random.default_rng(SEED0 + 2600 + seed)
        self.pitch = [tuple(w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[side]) for side in range(3)) for w, h in self.shapes]
        room = sum(h * max(p) + 512 for (w, h), p in zip(self.shapes, self.pitch)) + 8192
        self.h_src = rng.integers(0, 256, room, dtype=np.uint8)
        self.d = [torch.empty((room,), dtype=torch.uint8, device="cuda") for _ in range(3)]      # source, grids, reconstructions
        self.off = []
        at = [64, 192, 320]
        for i, ((w, h), p) in enumerate(zip(self.shapes, self.pitch)):
            o = []
            for side in range(3):
                a = -(-at[side] // 128) * 128 + (2 * ((i + side) % 5) + 1 if (i + side) % 2 else 0)
                base = self.d[side].data_ptr()
                while side in paged and w and h and not tail_ok(base + a, w, h, p[side]):
                    a += 128
                o.append(a)
                at[side] = a + (h * p[side] if w and h else 0) + 5
            self.off.append(tuple(o))
        assert max(at) <= room
        self.fill(variant)

    def fill(self, variant):
        """New source contents: content(w, h, variant) in every window, the random bytes around them unchanged."""
        import torch
        self.variant = variant
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                window(self.h_src, o[0], w, h, p[0])[...] = content(w, h, variant)
        self.d[0].copy_(torch.from_numpy(self.h_src))
        self.d[GRID].fill_(SENTINEL)
        self.d[RECON].fill_(SENTINEL)

    def triples(self):
        F = self.F
        return [F.RViewTriple(*([self.d[s].data_ptr() + o[s] if w and h else 0 for s in range(3)] + [w, h] + list(p)))
                for (w, h), p, o in zip(self.shapes, self.pitch, self.off)]

    def plan(self):
        return make_plan(self.F, self.triples())

    def expect(self, oracle, levels, interp, lut_name):
        want = [None, np.full(self.h_src.shape, SENTINEL, np.uint8), np.full(self.h_src.shape, SENTINEL, np.uint8)]
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                ref = reference(oracle, content(w, h, self.variant), (w, h, self.variant), levels, interp, lut_name)
                for side in (GRID, RECON):
                    window(want[side], o[side], w, h, p[side])[...] = ref[side - 1]
        return want

    def check(self, oracle, levels, interp, lut_name, what):
        import torch
        torch.cuda.synchronize()
        want = self.expect(oracle, levels, interp, lut_name)
        for side, name in ((GRID, "grid"), (RECON, "reconstruction")):
            got = self.d[side].cpu().numpy()
            bad = np.flatnonzero(got != want[side])
            assert bad.size == 0, "%s: %d bytes of the %s parent differ, the first at %d" % (what, bad.size, name, int(bad[0]))
        assert (self.d[0].cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"
        self.d[GRID].fill_(SENTINEL)
        self.d[RECON].fill_(SENTINEL)

    def untouched(self, what):
        import torch
        torch.cuda.synchronize()
        for side, name in ((GRID, "grid"), (RECON, "reconstruction")):
            assert (self.d[side].cpu().numpy() == SENTINEL).all(), "%s: the %s parent was written" % (what, name)
        assert (self.d[0].cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"


def make_plan(F, triples):
    """hgi_rviews_plan of a list of triples: (info, the blob as a device tensor kept alive by the caller)."""
    import torch
    L = F.lib()
    n = len(triples)
    arr = (F.RViewTriple * n)(*triples)
    size = L.hgi_rviews_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    info = F.RViewsInfo()
    st = L.hgi_rviews_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
    assert st == OK, F.last_error()
    assert info.magic == F.MAGIC and info.plan_bytes <= size
    blob = torch.from_numpy(host[:max(int(info.plan_bytes), 16)].copy()).cuda()
    return info, blob


def launch(F, plan, levels, interp, lut, stream=None):
    info, blob = plan
    return F.lib().hgi_rviews_encode_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp, lut.ctypes.data)


def run_all(F, oracle, parents, levels_set, luts, what):
    """Encode with every table, at every level, with both interpolators: each launch against the oracle."""
    plan = parents.plan()
    tabs = tables(oracle)
    for levels in levels_set:
        for interp in (1, 0):
            for name in luts:
                assert launch(F, plan, levels, interp, tabs[name]) == OK, F.last_error()
                parents.check(oracle, levels, interp, name, "%s L%d i%d %s" % (what, levels, interp, name))
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
def test_mixed_list_in_separate_parents(R, oracle):
    p = Parents(R, MIXED, seed=1)
    info, _ = run_all(R, oracle, p, range(1, 6), ("identity", "medium", "random"), "mixed")
    assert info.count == 13 and info.interior_tiles == 29 and info.max_width == 513
    assert len(set(p.pitch)) > 6 and any(len(set(q)) == 3 for q in p.pitch)      # the three sides of an entry at three pitches
    for side in range(3):
        assert any(o[side] % 2 for o in p.off) and any(o[side] % 128 == 0 for o in p.off)


SUBLISTS = {"one-entry": MIXED[:1], "interior-only": [(128, 64), (256, 128)], "ragged-only": MIXED[:4]}


@pytest.mark.parametrize("name", sorted(SUBLISTS))
def test_sublists_that_change_the_block_map(R, oracle, name):
    p = Parents(R, SUBLISTS[name], seed=10 + sorted(SUBLISTS).index(name))
    info, _ = run_all(R, oracle, p, range(1, 6), ("identity", "medium", "random"), name)
    if name == "interior-only":
        assert info.edge_tiles == 0 and info.interior_tiles == 5
    if name == "ragged-only":
        assert info.interior_tiles == 0 and info.edge_tiles == 6 and info.count == 4
    if name == "one-entry":
        assert info.interior_tiles == 0 and info.edge_tiles == 1 and info.count == 1


# ---------------------------------------------------------------------------------------------------- 2. the cone
@pytest.mark.parametrize("gap", (61, 0))
def test_cone_levels(R, oracle, gap):
    """Levels 6, 7, 8 (four fused levels under a cone through the read pitch): the SEEDED = 2 kernels, both IDENT."""
    p = Parents(R, CONE, seed=20 + gap, gaps=(gap, gap, gap))
    run_all(R, oracle, p, (6, 7, 8), ("medium", "identity"), "cone gap %d" % gap)


# --------------------------------------------------------------------------------------------------- 3. the atlas
def shelves(items, pitch, origin_kind):
    """Shelf placement of `items` = [(key, w, h), ...], taken in their order, in a canvas whose rows are `pitch` bytes: x origins
    on 128-B lines, 64 B into a line or at odd x, by origin_kind(position).  Returns ({key: (x, y)}, canvas height)."""
    at, x, y, shelf = {}, 0, 0, 0
    for n, (key, w, h) in enumerate(items):
        kind = origin_kind(n)
        odd = 1 + 2 * (n % 7)
        x0 = -(-x // 128) * 128 + (0, 64, odd)[kind]
        if x0 + w > pitch:
            y, shelf = y + shelf + 1, 0
            x0 = (0, 64, odd)[kind]
        at[key] = (x0, y)
        x, shelf = x0 + w + 1, max(shelf, h)
    return at, y + shelf + 2


def test_atlas_side_by_side(R, oracle):
    import torch
    F = R
    rng = np.random.default_rng(SEED0 + 2630)
    SP, DP = 1024, 1152
    live = [(i, w, h) for i, (w, h) in enumerate(MIXED) if w and h]
    src_at, src_h = shelves(live, SP, lambda n: n % 3)
    # grids and reconstructions in ONE output canvas, in another order: the list backwards, each entry's reconstruction next to
    # its grid
    outs = [((i, side), w, h) for i, w, h in live[::-1] for side in (RECON, GRID)]
    dst_at, dst_h = shelves(outs, DP, lambda n: (n + 1) % 3)
    for at in (src_at, dst_at):
        assert set((x % 128 == 0, x % 128 == 64, x % 2 == 1) for x, _ in at.values()) == {(True, False, False), (False, True, False), (False, False, True)}
    # two sources overlap: the 129 x 65 view is read out of the 256 x 128 view's window
    i_small, i_big = MIXED.index((129, 65)), MIXED.index((256, 128))
    src_at[i_small] = (src_at[i_big][0] + 31, src_at[i_big][1] + 17)
    h_src = rng.integers(0, 256, src_h * SP + 8192, dtype=np.uint8)
    d_src = torch.from_numpy(h_src).cuda()
    d_dst = torch.full((dst_h * DP + 8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    lead = 0      # the canvas' first byte in the parent: on a 128-B line, moved until every view keeps the page rule
    while not all(tail_ok(d_src.data_ptr() + lead + y * SP + x, MIXED[i][0], MIXED[i][1], SP) for i, (x, y) in src_at.items()):
        lead += 128
    assert lead < 4096
    place = lambda key: 128 + dst_at[key][1] * DP + dst_at[key][0]      # noqa: E731
    triples = []
    for i, (w, h) in enumerate(MIXED):
        if w and h:
            sx, sy = src_at[i]
            triples.append(F.RViewTriple(d_src.data_ptr() + lead + sy * SP + sx, d_dst.data_ptr() + place((i, GRID)), d_dst.data_ptr() + place((i, RECON)),
                                         w, h, SP, DP, DP))
        else:
            triples.append(F.RViewTriple(0, 0, 0, w, h, 0, 0, 0))
    plan = make_plan(F, triples)
    medium = tables(oracle)["medium"]
    for levels in (3, 7):
        assert launch(F, plan, levels, 1, medium) == OK, F.last_error()
        torch.cuda.synchronize()
        want = np.full(d_dst.shape[0], SENTINEL, np.uint8)
        for i, (w, h) in enumerate(MIXED):
            if w and h:
                sx, sy = src_at[i]
                ref = reference(oracle, window(h_src, lead + sy * SP + sx, w, h, SP), ("atlas", i), levels, 1, "medium")
                for side in (GRID, RECON):
                    window(want, place((i, side)), w, h, DP)[...] = ref[side - 1]
        got = d_dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "atlas L%d: %d bytes of the canvas differ, the first at %d" % (levels, bad.size, int(bad[0]))
        assert (want == SENTINEL).sum() > dst_h * DP // 4      # the sentinel between and around the windows was compared
        assert (d_src.cpu().numpy() == h_src).all()
        d_dst.fill_(SENTINEL)


# ------------------------------------------------------------------------------------- 4. plan reuse and capture
def test_plan_reuse_and_graph_capture(R, oracle):
    import torch
    F = R
    p = Parents(F, MIXED, seed=3)
    plan = p.plan()
    medium = tables(oracle)["medium"]
    for variant in (0, 1):
        p.fill(variant)
        assert launch(F, plan, 4, 1, medium) == OK, F.last_error()
        p.check(oracle, 4, 1, "medium", "launch %d of one plan" % variant)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = launch(F, plan, 4, 1, medium, stream=side.cuda_stream)
    assert st == OK, F.last_error()
    p.untouched("capturing must not run the launch")
    p.fill(2)
    g.replay()
    p.check(oracle, 4, 1, "medium", "replayed on new contents")


# --------------------------------------------------------------------------------------------- 5. the Python surface
def test_python_surface_composed_routes_and_identity(R, oracle):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    shapes = [(65, 129), (64, 128), (1, 200), (0, 3), (203, 301)]      # (height, width)
    total, places = H.aligned_arena(shapes)
    rng = np.random.default_rng(SEED0 + 2650)
    h_src = rng.integers(0, 256, total, dtype=np.uint8)
    src = torch.from_numpy(h_src).cuda()
    grids, recons = (torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2))
    views = lambda arena: H.views.arena_views(arena, shapes, places)      # noqa: E731
    tabs = tables(oracle)
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    assert (enc._lut == tabs["medium"]).all()

    def settle(levels, lut_name, what):
        want = [np.full(total, SENTINEL, np.uint8), np.full(total, SENTINEL, np.uint8)]
        for (h, w), (o, pitch) in zip(shapes, places):
            if h and w:
                img = np.ascontiguousarray(window(h_src, o, w, h, pitch))
                g = oracle.encode(img, levels, tabs[lut_name], 1)
                window(want[0], o, w, h, pitch)[...] = g
                window(want[1], o, w, h, pitch)[...] = oracle.decode(g, levels, 1)
        torch.cuda.synchronize()
        assert (grids.cpu().numpy() == want[0]).all(), what + ": grids"
        assert (recons.cpu().numpy() == want[1]).all(), what + ": reconstructions"
        assert (src.cpu().numpy() == h_src).all(), what + ": the sources were modified"
        grids.fill_(SENTINEL)
        recons.fill_(SENTINEL)

    plan = H.ReconViewPlan(zip(views(src), views(grids), views(recons)))
    assert plan.fused and plan.reason == "" and plan.info.count == 4 and len(plan) == 5 and len(plan.layouts) == 5
    assert plan.blob is not None and plan.blob.is_cuda and plan.blob.numel() == plan.info.plan_bytes
    g, r = enc.encode_views_with_reconstruction(plan)
    settle(4, "medium", "encode_views_with_reconstruction")
    assert len(g) == len(r) == 5 and g[0].data_ptr() == grids.data_ptr() and r[0].data_ptr() == recons.data_ptr() and tuple(g[3].shape) == (0, 3)
    # the composed route: a depth the one launch does not serve
    deep = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 9)
    deep.encode_views_with_reconstruction(plan)
    settle(9, "medium", "encode_views_with_reconstruction at scale_level 9")
    # the identity table: the reconstruction is the image
    ident = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Lossless), 4)
    assert (ident._lut == np.arange(256)).all()
    ident.encode_views_with_reconstruction(plan)
    torch.cuda.synchronize()
    for s, rv in zip(views(src), views(recons)):
        assert torch.equal(s, rv)
    settle(4, "identity", "encode_views_with_reconstruction under the identity table")
    # one entry whose last source byte is the last byte of a page, width % 4 != 0: the plan is not fused, the calls are composed
    w, h, pitch = 130, 66, 147
    span = (h - 1) * pitch + w
    parent = torch.from_numpy(rng.integers(0, 256, span + 3 * 4096, dtype=np.uint8)).cuda()
    lead = (-(parent.data_ptr() + span)) % 4096
    assert not tail_ok(parent.data_ptr() + lead, w, h, pitch)
    bad_src = parent[lead:lead + h * pitch - (pitch - w)].as_strided((h, w), (pitch, 1))
    good_src = views(src)[0]
    outs = [[torch.full((h, w + 5), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)],
            [torch.full((65, 129 + 3), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]]
    broken = H.ReconViewPlan([(bad_src, outs[0][0][:, :w], outs[0][1][:, :w]), (good_src, outs[1][0][:, :129], outs[1][1][:, :129])])
    assert not broken.fused and "tail" in broken.reason and "view 0" in broken.reason and broken.blob is None
    enc.encode_views_with_reconstruction(broken)
    torch.cuda.synchronize()
    for s, (og, orc), ww in ((bad_src, outs[0], w), (good_src, outs[1], 129)):
        img = np.ascontiguousarray(s.cpu().numpy())
        want = oracle.encode(img, 4, tabs["medium"], 1)
        got = og.cpu().numpy()
        assert (got[:, :ww] == want).all() and (got[:, ww:] == SENTINEL).all()
        got = orc.cpu().numpy()
        assert (got[:, :ww] == oracle.decode(want, 4, 1)).all() and (got[:, ww:] == SENTINEL).all()


# ------------------------------------------------------------------------------- 6. one call per instantiation
INSTANCES = [(i, d, s) for i in (1, 0) for d in (0, 1) for s in (0, 2)]


@functools.lru_cache(maxsize=None)
def _small(F):
    # 129 x 65: an interior tile and three EDGE == 2 tiles; 128 x 130: two interior tiles over an EDGE == 1 tile (full width, even
    # height, two rows); 70 x 1: one more EDGE == 2 tile
    return Parents(F, [(129, 65), (128, 130), (70, 1)], seed=60)


@pytest.mark.parametrize("interp,ident,seeded", INSTANCES, ids=["i%d-d%d-s%d" % t for t in INSTANCES])
def test_one_call_per_instantiation(R, oracle, interp, ident, seeded):
    """k_enc_recon_views<INTERP, IDENT, SEEDED> (8), one launch each against the oracle, on a list that holds an interior tile,
    an EDGE == 1 tile and an EDGE == 2 tile."""
    assert len(INSTANCES) == 8
    p = _small(R)
    levels = 6 if seeded else 3
    plan = p.plan()
    assert plan[0].interior_tiles == 1 + 2 and plan[0].edge_tiles == 3 + 1 + 1
    name = "identity" if ident else "medium"
    assert launch(R, plan, levels, interp, tables(oracle)[name]) == OK, R.last_error()
    p.check(oracle, levels, interp, name, "interp %d ident %d seeded %d" % (interp, ident, seeded))


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_levels_zero_and_nine_are_refused_untouched(R, oracle):
    p = _small(R)
    plan = p.plan()
    tabs = tables(oracle)
    for name in ("medium", "identity"):
        assert launch(R, plan, 0, 1, tabs[name]) == EUNSUPPORTED and "levels 0" in R.last_error()
        assert launch(R, plan, 9, 0, tabs[name]) == EUNSUPPORTED and "levels 9" in R.last_error()
    p.untouched("refused launches")


# ------------------------------------------------------------------------------------------- 8. the closure property
def test_view_list_decode_of_the_grids_gives_the_recon_arena(R, oracle):
    """An extra property (the oracle stays the judge): hgi_views_decode_dev on the grid views just written, into a third arena
    laid out like the reconstructions', gives the reconstruction parent byte for byte."""
    import torch
    import companion_layer as CL
    V = CL.binding("views")
    p = Parents(R, MIXED, seed=80, paged=(0, GRID))
    plan = p.plan()
    medium = tables(oracle)["medium"]
    again = torch.full_like(p.d[RECON], SENTINEL)
    n = len(p.shapes)
    pairs = (V.ViewPair * n)(*[V.ViewPair(p.d[GRID].data_ptr() + o[GRID] if w and h else 0, again.data_ptr() + o[RECON] if w and h else 0, w, h, q[GRID], q[RECON])
                               for (w, h), q, o in zip(p.shapes, p.pitch, p.off)])
    size = V.lib().hgi_views_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    vinfo = V.ViewsInfo()
    st = V.lib().hgi_views_plan(ctypes.addressof(pairs), n, host.ctypes.data, size, ctypes.addressof(vinfo))
    assert st == OK, V.last_error()
    vblob = torch.from_numpy(host[:int(vinfo.plan_bytes)].copy()).cuda()
    for levels in (4, 7):
        assert launch(R, plan, levels, 1, medium) == OK, R.last_error()
        assert V.lib().hgi_views_decode_dev(None, vblob.data_ptr(), ctypes.addressof(vinfo), levels, 1) == OK, V.last_error()
        torch.cuda.synchronize()
        assert torch.equal(again, p.d[RECON]), "L%d: the decode of the written grids differs from the written reconstructions" % levels
        again.fill_(SENTINEL)
        p.check(oracle, levels, 1, "medium", "closure L%d" % levels)
