"""GPU suite of the view lists (libhgi_views.so, include/hgi_views.h; Encoder.encode_views / Decoder.decode_views): every
case reads its sources out of parents of random bytes and writes into sentinel-filled parents that are compared WHOLE against
an expected parent built on the CPU from the oracle's output -- never from libhgi_hip.so, never from the library under test;
the sources must come back unmodified.
  1. a mixed list in separate parents (degenerate sides, ragged only, interior only, mixes, skipped entries; 29 interior tiles,
     so the eighths are uneven), gaps drawn independently per side, bases at odd addresses and on 128-B lines: encode at levels
     1-5 x both interpolators x {identity, Medium, a random table}, decode at levels 1-5 x both interpolators; the same on the
     sub-lists that change the map's shape;
  2. the cone: levels 6, 7, 8 on five shapes at two pitches -- the SEEDED = 2 kernels;
  3. an atlas: the views side by side in one 1024-byte-pitch canvas, written side by side in another order into a
     1152-byte-pitch canvas, window origins on 128-B lines, 64 B into a line and at odd x, two sources overlapping;
  4. one plan launched twice on new contents, then captured into a graph and replayed on new contents;
  5. the Python surface: aligned_arena, ViewPlan, encode_views -> decode_views, and the composed route of a list with one
     entry that breaks the page rule;
  6. one call per kernel instantiation: 12 calls."""
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
def V():
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("views")


def content(w, h, variant=0):
    """The bytes of a (h, w) source view: random, a function of the shape and the variant alone, so that a reference is computed
    once for every list that holds the view."""
    return np.random.default_rng(SEED0 + 210000 + 7919 * w + 31 * h + 1000003 * variant).integers(0, 256, (h, w), dtype=np.uint8)


def tables(oracle):
    return {"identity": oracle.noop_lut(), "medium": oracle.linear_lut(oracle.MEDIUM)[0],
            "random": np.random.default_rng(SEED0 + 2100).integers(0, 256, 256, dtype=np.uint8)}


_REF = {}


def reference(oracle, src, key, levels, interp, lut_name=None):
    """oracle.encode (lut_name given) or oracle.decode of `src`, computed once per key."""
    k = (key, levels, interp, lut_name)
    if k not in _REF:
        a = np.ascontiguousarray(src)
        _REF[k] = oracle.encode(a, levels, tables(oracle)[lut_name], interp) if lut_name else oracle.decode(a, levels, interp)
        _REF[k].setflags(write=False)
    return _REF[k]


def tail_ok(ptr, w, h, pitch):
    end = ptr + (h - 1) * (pitch if h > 1 else w) + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


class Parents:
    """A list of (w, h) views placed in a source parent of random bytes and a destination parent of sentinel bytes: view i at
    an odd address (odd i) or on a 128-byte line (even i), its rows `w + gap` bytes apart with a gap drawn per side."""

    def __init__(self, V, shapes, seed, gaps=None, variant=0):
        import torch
        self.V, self.shapes = V, list(shapes)
        rng = np.random.default_rng(SEED0 + 2000 + seed)
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


def launch(F, plan, levels, interp, lut=None, stream=None):
    info, blob = plan
    L = F.lib()
    if lut is None:
        return L.hgi_views_decode_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp)
    return L.hgi_views_encode_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp, lut.ctypes.data)


def run_all(F, oracle, parents, levels_set, luts, what):
    """Encode with every table and decode, at every level, with both interpolators: each launch against the oracle."""
    plan = parents.plan()
    tabs = tables(oracle)
    for levels in levels_set:
        for interp in (1, 0):
            for name in luts:
                assert launch(F, plan, levels, interp, tabs[name]) == OK, F.last_error()
                parents.check(oracle, levels, interp, name, "%s encode L%d i%d %s" % (what, levels, interp, name))
            assert launch(F, plan, levels, interp) == OK, F.last_error()
            parents.check(oracle, levels, interp, None, "%s decode L%d i%d" % (what, levels, interp))
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
def test_mixed_list_in_separate_parents(V, oracle):
    p = Parents(V, MIXED, seed=1)
    info, _ = run_all(V, oracle, p, range(1, 6), ("identity", "medium", "random"), "mixed")
    assert info.count == 13 and info.interior_tiles == 29 and info.max_width == 513
    assert len(set(p.pitch)) > 6 and any(a != b for a, b in p.pitch)


SUBLISTS = {"first": MIXED[:1], "no-edge": [(128, 64), (256, 128)], "nint-2": [(128, 64), (129, 65)], "prefix-2": MIXED[:2],
            "prefix-3": MIXED[:3], "prefix-4": MIXED[:4], "prefix-5": MIXED[:5]}


@pytest.mark.parametrize("name", sorted(SUBLISTS))
def test_sublists_that_change_the_maps_shape(V, oracle, name):
    p = Parents(V, SUBLISTS[name], seed=10 + sorted(SUBLISTS).index(name))
    info, _ = run_all(V, oracle, p, range(1, 6), ("identity", "medium", "random"), name)
    if name == "no-edge":
        assert info.edge_tiles == 0 and info.interior_tiles == 5
    if name == "nint-2":
        assert info.interior_tiles == 2
    if name in ("first", "prefix-2", "prefix-3", "prefix-4"):
        assert info.interior_tiles == 0


# ---------------------------------------------------------------------------------------------------- 2. the cone
@pytest.mark.parametrize("gap", (61, 0))
def test_cone_levels(V, oracle, gap):
    """Levels 6, 7, 8 (four fused levels under a cone through the read pitch): the SEEDED = 2 decoders and encoders."""
    p = Parents(V, CONE, seed=20 + gap, gaps=(gap, gap))
    run_all(V, oracle, p, (6, 7, 8), ("identity", "medium"), "cone gap %d" % gap)


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


def test_atlas_side_by_side(V, oracle):
    import torch
    F = V
    rng = np.random.default_rng(SEED0 + 2300)
    SP, DP = 1024, 1152
    order = list(range(len(MIXED)))
    src_at, src_h = shelves(MIXED, SP, order, lambda i: i % 3)
    dst_at, dst_h = shelves(MIXED, DP, order[::-1], lambda i: (i + 1) % 3)
    for at in (src_at, dst_at):
        assert set((x % 128 == 0, x % 128 == 64, x % 2 == 1) for x, _ in at.values()) == {(True, False, False), (False, True, False), (False, False, True)}
    # two sources overlap: the 129 x 65 view reads out of the 256 x 128 view's window
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
            pairs.append(F.ViewPair(d_src.data_ptr() + lead + sy * SP + sx, d_dst.data_ptr() + 128 + dy * DP + dx, w, h, SP, DP))
        else:
            pairs.append(F.ViewPair(0, 0, w, h, 0, 0))
    plan = make_plan(F, (F.ViewPair * len(pairs))(*pairs), len(pairs))
    medium = tables(oracle)["medium"]
    for levels in (3, 7):
        for lut_name in ("medium", None):
            assert launch(F, plan, levels, 1, medium if lut_name else None) == OK, F.last_error()
            torch.cuda.synchronize()
            want = np.full(d_dst.shape[0], SENTINEL, np.uint8)
            for i, (w, h) in enumerate(MIXED):
                if w and h:
                    (sx, sy), (dx, dy) = src_at[i], dst_at[i]
                    src = Parents.window(h_src, lead + sy * SP + sx, w, h, SP)
                    Parents.window(want, 128 + dy * DP + dx, w, h, DP)[...] = reference(oracle, src, ("atlas", i), levels, 1, lut_name)
            got = d_dst.cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "atlas L%d %s: %d bytes of the canvas differ, the first at %d" % (levels, lut_name or "decode", bad.size, int(bad[0]))
            assert (want == SENTINEL).sum() > dst_h * DP // 4      # the sentinel between and around the windows was compared
            assert (d_src.cpu().numpy() == h_src).all()
            d_dst.fill_(SENTINEL)


# ------------------------------------------------------------------------------------- 4. plan reuse and capture
def test_plan_reuse_and_graph_capture(V, oracle):
    import torch
    p = Parents(V, MIXED, seed=3)
    plan = p.plan()
    medium = tables(oracle)["medium"]
    for variant in (0, 1):
        p.fill(variant)
        assert launch(V, plan, 4, 1, medium) == OK, V.last_error()
        p.check(oracle, 4, 1, "medium", "launch %d of one plan" % variant)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = launch(V, plan, 4, 1, medium, stream=side.cuda_stream)
    assert st == OK, V.last_error()
    torch.cuda.synchronize()
    assert (p.d_dst.cpu().numpy() == SENTINEL).all(), "capturing must not run the launch"
    p.fill(2)
    g.replay()
    p.check(oracle, 4, 1, "medium", "replayed on new contents")


# --------------------------------------------------------------------------------------------- 5. the Python surface
def test_python_surface_fused_and_composed(V, oracle):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    shapes = [(65, 129), (64, 128), (1, 200), (0, 3), (203, 301)]      # (height, width)
    total, places = H.aligned_arena(shapes)
    assert all(o % 128 == 0 and pitch % 128 == 0 for o, pitch in places)
    rng = np.random.default_rng(SEED0 + 2500)
    h_img = rng.integers(0, 256, total, dtype=np.uint8)
    img, grid, back = torch.from_numpy(h_img).cuda(), torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda"), \
        torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    views = lambda arena: H.views.arena_views(arena, shapes, places)      # noqa: E731
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    dec = H.Decoder(Crossed())
    plan_e, plan_d = H.ViewPlan(zip(views(img), views(grid))), H.ViewPlan(zip(views(grid), views(back)))
    assert plan_e.fused and plan_d.fused and plan_e.info.count == 4
    outs = enc.encode_views(plan_e)
    dec.decode_views(plan_d, 4)
    torch.cuda.synchronize()
    medium = tables(oracle)["medium"]
    want_g, want_b = np.full(total, SENTINEL, np.uint8), np.full(total, SENTINEL, np.uint8)
    for (h, w), (o, pitch) in zip(shapes, places):
        if h and w:
            g = oracle.encode(np.ascontiguousarray(Parents.window(h_img, o, w, h, pitch)), 4, medium, 1)
            Parents.window(want_g, o, w, h, pitch)[...] = g
            Parents.window(want_b, o, w, h, pitch)[...] = oracle.decode(g, 4, 1)
    assert (grid.cpu().numpy() == want_g).all() and (back.cpu().numpy() == want_b).all() and (img.cpu().numpy() == h_img).all()
    assert len(outs) == 5 and outs[0].data_ptr() == grid.data_ptr()
    # one entry whose last source byte is the last byte of a page, width % 4 != 0: the plan is not fused, the calls are composed
    w, h, pitch = 130, 66, 147
    span = (h - 1) * pitch + w
    parent = torch.from_numpy(rng.integers(0, 256, span + 3 * 4096, dtype=np.uint8)).cuda()
    lead = (-(parent.data_ptr() + span)) % 4096
    assert not tail_ok(parent.data_ptr() + lead, w, h, pitch)
    bad_src = parent[lead:lead + h * pitch - (pitch - w)].as_strided((h, w), (pitch, 1))
    good_src = views(img)[0]
    outs = [torch.full((h, w + 5), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((65, 129 + 3), SENTINEL, dtype=torch.uint8, device="cuda")]
    plan = H.ViewPlan([(bad_src, outs[0][:, :w]), (good_src, outs[1][:, :129])])
    assert not plan.fused and "tail" in plan.reason and "view 0" in plan.reason
    enc.encode_views(plan)
    torch.cuda.synchronize()
    for src, out, ww in ((bad_src, outs[0], w), (good_src, outs[1], 129)):
        got = out.cpu().numpy()
        assert (got[:, :ww] == oracle.encode(np.ascontiguousarray(src.cpu().numpy()), 4, medium, 1)).all() and (got[:, ww:] == SENTINEL).all()


# ------------------------------------------------------------------------------- 6. one call per instantiation
INSTANCES = [("dec", i, s, None) for i in (1, 0) for s in (0, 2)] + [("enc", i, s, t) for i in (1, 0) for s in (0, 2) for t in ("identity", "medium")]


@functools.lru_cache(maxsize=None)
def _small(V):
    return Parents(V, [(129, 65), (128, 64), (70, 1)], seed=60)


@pytest.mark.parametrize("kind,interp,seeded,table", INSTANCES, ids=["%s-i%d-s%d-%s" % (k, i, s, t or "x") for k, i, s, t in INSTANCES])
def test_one_call_per_instantiation(V, oracle, kind, interp, seeded, table):
    """k_dec_views<INTERP, SEEDED> (4) and k_enc_views<INTERP, IDENT, SEEDED> (8), one launch each against the oracle."""
    assert len(INSTANCES) == 12
    p = _small(V)
    levels = 6 if seeded else 3
    plan = p.plan()
    assert launch(V, plan, levels, interp, tables(oracle)[table] if table else None) == OK, V.last_error()
    p.check(oracle, levels, interp, table, "%s interp %d seeded %d %s" % (kind, interp, seeded, table))
