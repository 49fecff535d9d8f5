"""GPU suite of the requantize view lists (libhgi_qviews.so, include/hgi_qviews.h; Encoder.requantize_views): every case reads
its source GRIDS -- random bytes: any byte array is a grid -- out of parents of random bytes and writes into sentinel-filled
parents that are compared WHOLE against an expected parent built on the CPU from the oracle,
    oracle.encode(oracle.decode(src, levels, interp), levels, lut, interp),
computed once per (shape, variant, levels, interp, table) -- never from libhgi_hip.so, never from a library under test; the
source parents must come back unmodified.  The plan of every case is hgi_views_plan's (libhgi_views.so).
  1. the mixed list of tests/test_views_gpu.py in separate parents (degenerate sides, ragged only, interior only, mixes, skipped
     entries), gaps drawn independently per side, bases at odd addresses and on 128-B lines: levels 1-5 x both interpolators x
     {Medium, a random table}; the same on the sub-lists that change the block map: ragged only, interior only, one entry;
  2. the cone: levels 6, 7, 8 on five shapes at two pitches -- the SEEDED = 2 kernels and their second walk;
  3. an atlas: the sources side by side in one 1024-byte-pitch canvas, two of them overlapping, written side by side in another
     order into a 1152-byte-pitch canvas, window origins on 128-B lines, 64 B into a line and at odd x;
  4. one plan launched twice on new contents, then captured into a graph and replayed on new contents;
  5. the Python surface: ONE ViewPlan through decode_views, encode_views and requantize_views in turn; the composed route at
     scale_level 9 and of a list with one entry that breaks the page rule; the identity table, without a call of the library;
  6. one call per kernel instantiation: 4 calls, each on a list with an interior, an EDGE == 1 and an EDGE == 2 tile;
  7. the identity table and levels = 0 are refused, with the destination parent untouched."""
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


@pytest.fixture(scope="module")
def Q():
    """(binding of libhgi_qviews.so, binding of libhgi_views.so: the plan)"""
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("qviews"), CL.binding("views")


def content(w, h, variant=0):
    """The bytes of a (h, w) source grid: random, a function of the shape and the variant alone, so that a reference is computed
    once for every list that holds the view."""
    return np.random.default_rng(SEED0 + 240000 + 7919 * w + 31 * h + 1000003 * variant).integers(0, 256, (h, w), dtype=np.uint8)


def tables(oracle):
    return {"identity": oracle.noop_lut(), "medium": oracle.linear_lut(oracle.MEDIUM)[0],
            "random": np.random.default_rng(SEED0 + 2400).integers(0, 256, 256, dtype=np.uint8)}


_DEC, _REF = {}, {}


def reference(oracle, src, key, levels, interp, lut_name):
    """oracle.encode(oracle.decode(src)) under the named table, computed once per key; the decoded image once per (key, levels,
    interp)."""
    k = (key, levels, interp, lut_name)
    if k not in _REF:
        if k[:3] not in _DEC:
            _DEC[k[:3]] = oracle.decode(np.ascontiguousarray(src), levels, interp)
            _DEC[k[:3]].setflags(write=False)
        _REF[k] = oracle.encode(_DEC[k[:3]], levels, tables(oracle)[lut_name], interp)
        _REF[k].setflags(write=False)
    return _REF[k]


def tail_ok(ptr, w, h, pitch):
    end = ptr + (h - 1) * (pitch if h > 1 else w) + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


class Parents:
    """A list of (w, h) views placed in a source parent of random bytes and a destination parent of sentinel bytes: view i at
    an odd address (odd i) or on a 128-byte line (even i), its rows `w + gap` bytes apart with a gap drawn per side; source
    offsets are advanced until the page rule holds."""

    def __init__(self, V, shapes, seed, gaps=None, variant=0):
        import torch
        self.V, self.shapes = V, list(shapes)
        rng = np.random.default_rng(SEED0 + 2400 + seed)
        self.pitch = [(w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[0]), w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[1]))
                      for w, h in self.shapes]
        room = sum(h * max(p) + 512 for (w, h), p in zip(self.shapes, self.pitch)) + 8192
        self.h_src = rng.integers(0, 256, room, dtype=np.uint8)
        self.d_src = torch.empty((room,), dtype=torch.uint8, device="cuda")
        self.d_dst = torch.empty((room,), dtype=torch.uint8, device="cuda")
        self.off = []
        at = [64, 192]
        for i, ((w, h), p) in enumerate(zip(self.shapes, self.pitch)):
            o = []
            for side in range(2):
                a = -(-at[side] // 128) * 128 + (2 * (i % 5) + 1 if i % 2 else 0)
                base = (self.d_src if side == 0 else self.d_dst).data_ptr()
                while side == 0 and w and h and not tail_ok(base + a, w, h, p[0]):
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
                self.window(self.h_src, o[0], w, h, p[0])[...] = content(w, h, variant)
        self.d_src.copy_(torch.from_numpy(self.h_src))
        self.d_dst.fill_(SENTINEL)

    @staticmethod
    def window(parent, off, w, h, pitch):
        return np.lib.stride_tricks.as_strided(parent[off:], (h, w), (pitch, 1))

    def plan(self):
        F = self.V
        n = len(self.shapes)
        arr = (F.ViewPair * n)(*[F.ViewPair(self.d_src.data_ptr() + o[0] if w and h else 0, self.d_dst.data_ptr() + o[1] if w and h else 0, w, h, p[0], p[1])
                                 for (w, h), p, o in zip(self.shapes, self.pitch, self.off)])
        return make_plan(F, arr, n)

    def expect(self, oracle, levels, interp, lut_name):
        want = np.full(self.h_src.shape, SENTINEL, np.uint8)
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                self.window(want, o[1], w, h, p[1])[...] = reference(oracle, content(w, h, self.variant), (w, h, self.variant), levels, interp, lut_name)
        return want

    def check(self, oracle, levels, interp, lut_name, what):
        import torch
        torch.cuda.synchronize()
        got = self.d_dst.cpu().numpy()
        want = self.expect(oracle, levels, interp, lut_name)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d bytes of the destination parent differ, the first at %d" % (what, bad.size, int(bad[0]))
        assert (self.d_src.cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"
        self.d_dst.fill_(SENTINEL)

    def untouched(self, what):
        import torch
        torch.cuda.synchronize()
        assert (self.d_dst.cpu().numpy() == SENTINEL).all(), what + ": the destination parent was written"
        assert (self.d_src.cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"


def make_plan(F, arr, n):
    """hgi_views_plan of a ctypes array of pairs: (info, the blob as a device tensor kept alive by the caller)."""
    import torch
    L = F.lib()
    size = L.hgi_views_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    info = F.ViewsInfo()
    st = L.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
    assert st == OK, F.last_error()
    assert info.magic == F.MAGIC and info.plan_bytes <= size
    blob = torch.from_numpy(host[:max(int(info.plan_bytes), 16)].copy()).cuda()
    return info, blob


def launch(F, plan, levels, interp, lut, stream=None):
    info, blob = plan
    return F.lib().hgi_qviews_requant_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp, lut.ctypes.data)


def run_all(Q, oracle, parents, levels_set, luts, what):
    """Requantize with every table, at every level, with both interpolators: each launch against the oracle."""
    F = Q[0]
    plan = parents.plan()
    tabs = tables(oracle)
    for levels in levels_set:
        for interp in (1, 0):
            for name in luts:
                assert launch(F, plan, levels, interp, tabs[name]) == OK, F.last_error()
                parents.check(oracle, levels, interp, name, "%s L%d i%d %s" % (what, levels, interp, name))
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
def test_mixed_list_in_separate_parents(Q, oracle):
    p = Parents(Q[1], MIXED, seed=1)
    info, _ = run_all(Q, oracle, p, range(1, 6), ("medium", "random"), "mixed")
    assert info.count == 13 and info.interior_tiles == 29 and info.max_width == 513
    assert len(set(p.pitch)) > 6 and any(a != b for a, b in p.pitch)
    assert any(o[0] % 2 for o in p.off) and any(o[0] % 128 == 0 for o in p.off)


SUBLISTS = {"one-entry": MIXED[:1], "interior-only": [(128, 64), (256, 128)], "ragged-only": MIXED[:4]}


@pytest.mark.parametrize("name", sorted(SUBLISTS))
def test_sublists_that_change_the_block_map(Q, oracle, name):
    p = Parents(Q[1], SUBLISTS[name], seed=10 + sorted(SUBLISTS).index(name))
    info, _ = run_all(Q, oracle, p, range(1, 6), ("medium", "random"), name)
    if name == "interior-only":
        assert info.edge_tiles == 0 and info.interior_tiles == 5
    if name == "ragged-only":
        assert info.interior_tiles == 0 and info.edge_tiles == 6 and info.count == 4
    if name == "one-entry":
        assert info.interior_tiles == 0 and info.edge_tiles == 1 and info.count == 1


# ---------------------------------------------------------------------------------------------------- 2. the cone
@pytest.mark.parametrize("gap", (61, 0))
def test_cone_levels(Q, oracle, gap):
    """Levels 6, 7, 8 (four fused levels under a cone through the read pitch, walked once in each direction): the SEEDED = 2
    kernels."""
    p = Parents(Q[1], CONE, seed=20 + gap, gaps=(gap, gap))
    run_all(Q, oracle, p, (6, 7, 8), ("medium",), "cone gap %d" % gap)


# --------------------------------------------------------------------------------------------------- 3. the atlas
def shelves(shapes, pitch, order, origin_kind):
    """Shelf placement of the non-empty `shapes`, taken in `order`, in a canvas whose rows are `pitch` bytes: x origins on 128-B
    lines, 64 B into a line or at odd x, by origin_kind(i).  Returns ({index: (x, y)}, canvas height)."""
    at, x, y, shelf = {}, 0, 0, 0
    for i in order:
        w, h = shapes[i]
        if not w or not h:
            continue
        kind = origin_kind(i)
        x0 = -(-x // 128) * 128 + (0, 64, 1 + 2 * (i % 7))[kind]
        if x0 + w > pitch:
            y, shelf = y + shelf + 1, 0
            x0 = (0, 64, 1 + 2 * (i % 7))[kind]
        at[i] = (x0, y)
        x, shelf = x0 + w + 1, max(shelf, h)
    return at, y + shelf + 2


def test_atlas_side_by_side(Q, oracle):
    import torch
    F, V = Q
    rng = np.random.default_rng(SEED0 + 2430)
    SP, DP = 1024, 1152
    order = list(range(len(MIXED)))
    src_at, src_h = shelves(MIXED, SP, order, lambda i: i % 3)
    dst_at, dst_h = shelves(MIXED, DP, order[::-1], lambda i: (i + 1) % 3)
    for at in (src_at, dst_at):
        assert set((x % 128 == 0, x % 128 == 64, x % 2 == 1) for x, _ in at.values()) == {(True, False, False), (False, True, False), (False, False, True)}
    # two sources overlap: the 129 x 65 grid is read out of the 256 x 128 grid's window
    i_small, i_big = MIXED.index((129, 65)), MIXED.index((256, 128))
    src_at[i_small] = (src_at[i_big][0] + 31, src_at[i_big][1] + 17)
    h_src = rng.integers(0, 256, src_h * SP + 8192, dtype=np.uint8)
    d_src = torch.from_numpy(h_src).cuda()
    d_dst = torch.full((dst_h * DP + 8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    lead = 0      # the canvas' first byte in the parent: on a 128-B line, moved until every view keeps the page rule
    while not all(tail_ok(d_src.data_ptr() + lead + y * SP + x, MIXED[i][0], MIXED[i][1], SP) for i, (x, y) in src_at.items()):
        lead += 128
    assert lead < 4096
    pairs = []
    for i, (w, h) in enumerate(MIXED):
        if w and h:
            (sx, sy), (dx, dy) = src_at[i], dst_at[i]
            pairs.append(V.ViewPair(d_src.data_ptr() + lead + sy * SP + sx, d_dst.data_ptr() + 128 + dy * DP + dx, w, h, SP, DP))
        else:
            pairs.append(V.ViewPair(0, 0, w, h, 0, 0))
    plan = make_plan(V, (V.ViewPair * len(pairs))(*pairs), len(pairs))
    medium = tables(oracle)["medium"]
    for levels in (3, 7):
        assert launch(F, plan, levels, 1, medium) == OK, F.last_error()
        torch.cuda.synchronize()
        want = np.full(d_dst.shape[0], SENTINEL, np.uint8)
        for i, (w, h) in enumerate(MIXED):
            if w and h:
                (sx, sy), (dx, dy) = src_at[i], dst_at[i]
                src = Parents.window(h_src, lead + sy * SP + sx, w, h, SP)
                Parents.window(want, 128 + dy * DP + dx, w, h, DP)[...] = reference(oracle, src, ("atlas", i), levels, 1, "medium")
        got = d_dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "atlas L%d: %d bytes of the canvas differ, the first at %d" % (levels, bad.size, int(bad[0]))
        assert (want == SENTINEL).sum() > dst_h * DP // 4      # the sentinel between and around the windows was compared
        assert (d_src.cpu().numpy() == h_src).all()
        d_dst.fill_(SENTINEL)


# ------------------------------------------------------------------------------------- 4. plan reuse and capture
def test_plan_reuse_and_graph_capture(Q, oracle):
    import torch
    F = Q[0]
    p = Parents(Q[1], MIXED, seed=3)
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
    torch.cuda.synchronize()
    assert (p.d_dst.cpu().numpy() == SENTINEL).all(), "capturing must not run the launch"
    p.fill(2)
    g.replay()
    p.check(oracle, 4, 1, "medium", "replayed on new contents")


# --------------------------------------------------------------------------------------------- 5. the Python surface
def test_python_surface_shared_plan_composed_routes_and_identity(Q, oracle, monkeypatch):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd import _ffi_qviews
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    shapes = [(65, 129), (64, 128), (1, 200), (0, 3), (203, 301)]      # (height, width)
    total, places = H.aligned_arena(shapes)
    rng = np.random.default_rng(SEED0 + 2450)
    h_src = rng.integers(0, 256, total, dtype=np.uint8)
    src, dst = torch.from_numpy(h_src).cuda(), torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    views = lambda arena: H.views.arena_views(arena, shapes, places)      # noqa: E731
    medium = tables(oracle)["medium"]
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    assert (enc._lut == medium).all()
    dec = H.Decoder(Crossed())

    def expect(fn):
        want = np.full(total, SENTINEL, np.uint8)
        for (h, w), (o, pitch) in zip(shapes, places):
            if h and w:
                Parents.window(want, o, w, h, pitch)[...] = fn(np.ascontiguousarray(Parents.window(h_src, o, w, h, pitch)))
        return want

    def settle(want, what):
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == want).all(), what
        assert (src.cpu().numpy() == h_src).all(), what + ": the sources were modified"
        dst.fill_(SENTINEL)

    # ONE plan object, three directions: its first views are the side that is read
    plan = H.ViewPlan(zip(views(src), views(dst)))
    assert plan.fused and plan.info.count == 4
    dec.decode_views(plan, 4)
    settle(expect(lambda g: oracle.decode(g, 4, 1)), "decode_views")
    enc.encode_views(plan)
    settle(expect(lambda a: oracle.encode(a, 4, medium, 1)), "encode_views")
    outs = enc.requantize_views(plan)
    requant4 = expect(lambda g: oracle.encode(oracle.decode(g, 4, 1), 4, medium, 1))
    settle(requant4, "requantize_views")
    assert len(outs) == 5 and outs[0].data_ptr() == dst.data_ptr() and tuple(outs[3].shape) == (0, 3)
    # the composed route: a depth the one launch does not serve
    deep = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 9)
    deep.requantize_views(plan)
    settle(expect(lambda g: oracle.encode(oracle.decode(g, 9, 1), 9, medium, 1)), "requantize_views at scale_level 9")
    # the identity table: the destinations equal the sources, and the library is not called
    ident = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Lossless), 4)
    assert (ident._lut == np.arange(256)).all()
    with monkeypatch.context() as m:
        m.setattr(_ffi_qviews, "lib", lambda: pytest.fail("the identity table must not reach the library"))
        ident.requantize_views(plan)
        settle(expect(lambda g: g), "requantize_views under the identity table")
    # one entry whose last source byte is the last byte of a page, width % 4 != 0: the plan is not fused, the calls are composed
    w, h, pitch = 130, 66, 147
    span = (h - 1) * pitch + w
    parent = torch.from_numpy(rng.integers(0, 256, span + 3 * 4096, dtype=np.uint8)).cuda()
    lead = (-(parent.data_ptr() + span)) % 4096
    assert not tail_ok(parent.data_ptr() + lead, w, h, pitch)
    bad_src = parent[lead:lead + h * pitch - (pitch - w)].as_strided((h, w), (pitch, 1))
    good_src = views(src)[0]
    outs = [torch.full((h, w + 5), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((65, 129 + 3), SENTINEL, dtype=torch.uint8, device="cuda")]
    broken = H.ViewPlan([(bad_src, outs[0][:, :w]), (good_src, outs[1][:, :129])])
    assert not broken.fused and "tail" in broken.reason and "view 0" in broken.reason
    for e, name in ((enc, "medium"), (ident, "identity")):
        e.requantize_views(broken)
        torch.cuda.synchronize()
        for s, out, ww in ((bad_src, outs[0], w), (good_src, outs[1], 129)):
            got, g = out.cpu().numpy(), np.ascontiguousarray(s.cpu().numpy())
            assert (got[:, :ww] == oracle.encode(oracle.decode(g, 4, 1), 4, tables(oracle)[name], 1)).all() and (got[:, ww:] == SENTINEL).all(), name
            out.fill_(SENTINEL)


# ------------------------------------------------------------------------------- 6. one call per instantiation
INSTANCES = [(i, s) for i in (1, 0) for s in (0, 2)]


@functools.lru_cache(maxsize=None)
def _small(V):
    # 129 x 65: an interior tile and three EDGE == 2 tiles; 128 x 130: two interior tiles over an EDGE == 1 tile (full width, even
    # height, two rows); 70 x 1: one more EDGE == 2 tile
    return Parents(V, [(129, 65), (128, 130), (70, 1)], seed=60)


@pytest.mark.parametrize("interp,seeded", INSTANCES, ids=["i%d-s%d" % (i, s) for i, s in INSTANCES])
def test_one_call_per_instantiation(Q, oracle, interp, seeded):
    """k_requant_views<INTERP, SEEDED> (4), one launch each against the oracle, on a list that holds an interior tile, an
    EDGE == 1 tile and an EDGE == 2 tile."""
    assert len(INSTANCES) == 4
    p = _small(Q[1])
    levels = 6 if seeded else 3
    plan = p.plan()
    assert plan[0].interior_tiles == 1 + 2 and plan[0].edge_tiles == 3 + 1 + 1
    assert launch(Q[0], plan, levels, interp, tables(oracle)["medium"]) == OK, Q[0].last_error()
    p.check(oracle, levels, interp, "medium", "interp %d seeded %d" % (interp, seeded))


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_identity_table_and_levels_zero_are_refused_untouched(Q, oracle):
    F = Q[0]
    p = _small(Q[1])
    plan = p.plan()
    tabs = tables(oracle)
    assert (tabs["identity"] == np.arange(256)).all()
    for levels in (1, 4, 8):
        assert launch(F, plan, levels, 1, tabs["identity"]) == EUNSUPPORTED and "copy the source" in F.last_error()
    for name in ("medium", "identity"):
        assert launch(F, plan, 0, 1, tabs[name]) == EUNSUPPORTED and "levels 0" in F.last_error()
    assert launch(F, plan, 9, 0, tabs["medium"]) == EUNSUPPORTED
    p.untouched("refused launches")
    # ... and under the identity table the oracle gives the source back: what the refusal's message rests on
    g = content(129, 65)
    assert (oracle.encode(oracle.decode(g, 4, 1), 4, tabs["identity"], 1) == g).all()
