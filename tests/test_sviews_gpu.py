"""GPU suite of the scaled view lists (libhgi_sviews.so, include/hgi_sviews.h; Decoder.decode_scaled_views): every case reads its
source GRIDS -- random bytes: any byte array is a grid -- out of parents of random bytes and writes into sentinel-filled parents
that are compared WHOLE against an expected parent built on the CPU from the oracle,
    oracle.decode(packed grid, levels, interp)[::2**s, ::2**s],
computed once per (grid, levels, interp) -- never from libhgi_hip.so, never from a library under test; the source parents must come
back unmodified.  Output shapes are the MIXED list of tests/test_qviews_gpu.py; each comes from the smallest and from the largest
grid that maps to it, w = (sw - 1) * 2**s + 1 and sw * 2**s, with gaps drawn per side and bases at odd addresses and on lines.
  1. s = 1, 2 (wide loads) x r = levels - s = 1 ... 5 x both interpolators, and the sub-lists that change the block map; a reduced
     list at s = 3 and s = 5 (byte loads);
  2. the cone: r = 6, 7, 8 on the CONE shapes at s = 1 and 2, two pitches;
  3. the last-row rule: 255 x 127 and 255 x 129 grids at s = 1, packed and at pitch 320, and 509 x 253 and 509 x 257 at s = 2,
     packed and at pitch 640 -- the smallest shapes where an interior tile's wide load would leave the span -- each the last
     bytes of its allocation; and a taller grid of which some interior tile rows remain;
  4. off-lattice and gap bytes rewritten between two launches of one plan: the output is identical;
  5. an atlas: grids side by side in one canvas, two of them overlapping, thumbnails side by side in another canvas;
  6. one plan launched twice on new contents, then captured into a graph and replayed on new contents;
  7. one call per kernel instantiation (12), each on a list with an interior and a ragged tile;
  8. the Python surface: the fused route; the composed routes (levels <= shift, r = 9, a plan of shift 0), each equal to the
     oracle; refusals leave the destination untouched."""
import ctypes

import numpy as np
import pytest

from conftest import SEED0

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1, 4      # hgi_status (include/hgi.h)
GAPS = (0, 1, 3, 16, 61, 128)
SENTINEL = 0xA5
# (sw, sh): the OUTPUT shapes of case 1 -- the mixed list of tests/test_qviews_gpu.py
MIXED = [(1, 1), (1, 70), (200, 1), (127, 63), (128, 64), (129, 65), (0, 5), (256, 128), (255, 129), (7, 0), (384, 64), (128, 192),
         (130, 66), (301, 203), (513, 130)]
CONE = [(300, 200), (513, 257), (64, 64), (1, 300), (257, 1)]
REDUCED = {3: [(1, 1), (129, 65), (256, 128), (0, 5), (301, 203)], 5: [(1, 1), (129, 65), (130, 66)]}
SUBLISTS = {"one-entry": MIXED[:1], "interior-only": [(128, 64), (256, 128)], "ragged-only": MIXED[:4]}


@pytest.fixture(scope="module")
def S():
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("sviews")


def grid_shape(sw, sh, s, large):
    """The smallest or the largest (w, h) grid whose 1 / 2**s image is sw x sh."""
    f = (lambda v: v << s) if large else (lambda v: ((v - 1) << s) + 1)
    return (f(sw) if sw else 0, f(sh) if sh else 0)


def content(w, h, variant=0):
    """The bytes of a (h, w) source grid: random, a function of the shape and the variant alone, so that a reference is computed
    once for every list that holds the grid."""
    return np.random.default_rng(SEED0 + 250000 + 7919 * w + 31 * h + 1000003 * variant).integers(0, 256, (h, w), dtype=np.uint8)


_REF = {}


def reference(oracle, grid, key, levels, interp, s):
    """oracle.decode(packed grid, levels, interp)[::2**s, ::2**s]; with a key, computed once."""
    k = (key, levels, interp, s)
    if key is None or k not in _REF:
        r = np.ascontiguousarray(oracle.decode(np.ascontiguousarray(grid), levels, interp)[::1 << s, ::1 << s])
        r.setflags(write=False)
        if key is None:
            return r
        _REF[k] = r
    return _REF[k]


def window(parent, off, w, h, pitch):
    return np.lib.stride_tricks.as_strided(parent[off:], (h, w), (pitch, 1))


class Parents:
    """A list of (sw, sh) output shapes at shift s: grid i (the smallest or the largest that maps to shape i) in a source parent
    of random bytes, image i in a destination parent of sentinel bytes; each at an odd address (odd i) or on a 128-byte line
    (even i), rows `width + gap` bytes apart with a gap drawn per side.  No page rule: nothing is moved for it."""

    def __init__(self, F, shapes, s, large, seed, gaps=None, variant=0):
        import torch
        self.F, self.s, self.out_shapes = F, s, list(shapes)
        self.grids = [grid_shape(sw, sh, s, large[i % len(large)] if isinstance(large, (list, tuple)) else large) for i, (sw, sh) in enumerate(self.out_shapes)]
        rng = np.random.default_rng(SEED0 + 2500 + seed)
        self.pitch = [(w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[0]), sw + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[1]))
                      for (w, h), (sw, sh) in zip(self.grids, self.out_shapes)]
        rooms = [sum((h, sh)[side] * p[side] + 512 for (w, h), (sw, sh), p in zip(self.grids, self.out_shapes, self.pitch)) + 1024 for side in range(2)]
        self.h_src = rng.integers(0, 256, rooms[0], dtype=np.uint8)
        self.d_src = torch.empty((rooms[0],), dtype=torch.uint8, device="cuda")
        self.d_dst = torch.empty((rooms[1],), dtype=torch.uint8, device="cuda")
        self.off = []
        at = [64, 192]
        for i, ((w, h), (sw, sh), p) in enumerate(zip(self.grids, self.out_shapes, self.pitch)):
            o = []
            for side in range(2):
                a = -(-at[side] // 128) * 128 + (2 * (i % 5) + 1 if i % 2 else 0)
                o.append(a)
                at[side] = a + ((h, sh)[side] * p[side] if w and h else 0) + 5
            self.off.append(tuple(o))
        assert at[0] <= rooms[0] and at[1] <= rooms[1]
        self.fill(variant)

    def fill(self, variant):
        """New source contents: content(w, h, variant) in every window, the random bytes around them unchanged."""
        import torch
        self.variant = variant
        for (w, h), p, o in zip(self.grids, self.pitch, self.off):
            if w and h:
                window(self.h_src, o[0], w, h, p[0])[...] = content(w, h, variant)
        self.d_src.copy_(torch.from_numpy(self.h_src))
        self.d_dst.fill_(SENTINEL)

    def pairs(self):
        return [[self.d_src.data_ptr() + o[0] if w and h else 0, self.d_dst.data_ptr() + o[1] if w and h else 0, w, h, p[0], p[1]]
                for (w, h), p, o in zip(self.grids, self.pitch, self.off)]

    def plan(self):
        return make_plan(self.F, self.pairs(), self.s)

    def views(self):
        """The (grid view, image view) torch pairs of the list."""
        import torch
        return [(torch.as_strided(self.d_src, (h, w), (p[0], 1), o[0]) if w and h else self.d_src.new_empty((h, w)),
                 torch.as_strided(self.d_dst, (sh, sw), (p[1], 1), o[1]) if w and h else self.d_dst.new_empty((sh, sw)))
                for (w, h), (sw, sh), p, o in zip(self.grids, self.out_shapes, self.pitch, self.off)]

    def expect(self, oracle, levels, interp):
        want = np.full(self.d_dst.numel(), SENTINEL, np.uint8)
        for (w, h), (sw, sh), p, o in zip(self.grids, self.out_shapes, self.pitch, self.off):
            if w and h:
                window(want, o[1], sw, sh, p[1])[...] = reference(oracle, content(w, h, self.variant), (w, h, self.variant), levels, interp, self.s)
        return want

    def check(self, oracle, levels, interp, what):
        import torch
        torch.cuda.synchronize()
        got = self.d_dst.cpu().numpy()
        want = self.expect(oracle, levels, interp)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d bytes of the destination parent differ, the first at %d" % (what, bad.size, int(bad[0]))
        assert (self.d_src.cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"
        self.d_dst.fill_(SENTINEL)

    def untouched(self, what):
        import torch
        torch.cuda.synchronize()
        assert (self.d_dst.cpu().numpy() == SENTINEL).all(), what + ": the destination parent was written"
        assert (self.d_src.cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"


def make_plan(F, pairs, s, want=OK):
    """hgi_sviews_plan of [[src, dst, w, h, sp, dp], ...]: (info, the blob as a device tensor kept alive by the caller)."""
    import torch
    L = F.lib()
    n = len(pairs)
    arr = (F.SViewPair * max(n, 1))(*[F.SViewPair(*v) for v in pairs])
    size = L.hgi_sviews_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    info = F.SViewsInfo()
    st = L.hgi_sviews_plan(ctypes.addressof(arr), n, s, host.ctypes.data, size, ctypes.addressof(info))
    assert st == want, F.last_error()
    if st != OK:
        return None
    assert info.magic == F.MAGIC and info.plan_bytes <= size and info.shift == s
    blob = torch.from_numpy(host[:max(int(info.plan_bytes), 16)].copy()).cuda()
    return info, blob


def launch(F, plan, levels, interp, stream=None):
    info, blob = plan
    return F.lib().hgi_sviews_decode_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp)


def run_all(F, oracle, parents, depths, what):
    """Every remaining depth r (levels = s + r) with both interpolators: each launch against the oracle."""
    plan = parents.plan()
    for r in depths:
        for interp in (1, 0):
            assert launch(F, plan, parents.s + r, interp) == OK, F.last_error()
            parents.check(oracle, parents.s + r, interp, "%s s%d r%d i%d" % (what, parents.s, r, interp))
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
@pytest.mark.parametrize("large", (False, True), ids=("smallest", "largest"))
@pytest.mark.parametrize("s", (1, 2))
def test_mixed_list_with_wide_loads(S, oracle, s, large):
    p = Parents(S, MIXED, s, large, seed=10 * s + large)
    info, _ = run_all(S, oracle, p, range(1, 6), "mixed")
    assert info.count == 13 and info.max_width == 513 and info.shift == s
    # the largest grids leave every whole tile interior; of the smallest, the tile rows that reach the last lattice row are ragged
    assert info.edge_tiles + info.interior_tiles == 1 + 2 + 2 + 1 + 1 + 4 + 4 + 6 + 3 + 3 + 4 + 12 + 15
    assert info.interior_tiles == 29 if large else 0 < info.interior_tiles < 29
    assert len(set(p.pitch)) > 6 and any(o[0] % 2 for o in p.off) and any(o[0] % 128 == 0 for o in p.off)


@pytest.mark.parametrize("name", sorted(SUBLISTS))
def test_sublists_that_change_the_block_map(S, oracle, name):
    for s in (1, 2):
        p = Parents(S, SUBLISTS[name], s, (True, False), seed=30 + s)
        info, _ = run_all(S, oracle, p, (1, 3, 5), name)
        if name == "interior-only":
            assert info.edge_tiles == 2 and info.interior_tiles == 3      # (the smallest grid of 256 x 128 gives up its second tile row: the last-row rule)
        else:
            assert info.interior_tiles == 0


@pytest.mark.parametrize("s", (3, 5))
def test_reduced_list_with_byte_loads(S, oracle, s):
    for large in (False, True):
        p = Parents(S, REDUCED[s], s, large, seed=50 + s)
        info, _ = run_all(S, oracle, p, (1, 2, 4, 5), "reduced")
        assert info.shift == s and info.count == len([1 for w, h in REDUCED[s] if w and h])


# ------------------------------------------------------------------------------------------------------ 2. the cone
@pytest.mark.parametrize("s", (1, 2))
def test_cone_at_six_to_eight_remaining_levels(S, oracle, s):
    for gaps, large in (((0, 0), True), ((61, 3), False)):
        p = Parents(S, CONE, s, large, seed=70 + s, gaps=gaps)
        run_all(S, oracle, p, (6, 7, 8), "cone %s" % (gaps,))


# --------------------------------------------------------------------------------------------- 3. the last-row rule
LAST_ROW = {1: ((255, 127, 255), (255, 127, 320), (255, 129, 255), (255, 129, 320), (255, 399, 255), (255, 399, 320)),
            2: ((509, 253, 509), (509, 253, 640), (509, 257, 509), (509, 257, 640), (509, 797, 640))}


@pytest.mark.parametrize("s", (1, 2))
def test_last_row_rule_at_the_end_of_an_allocation(S, oracle, s):
    """An interior tile's wide load on the grid's last lattice row would read the dword behind the row's last byte: behind the
    span, which ends the allocation here.  The plan makes the tile rows that reach that row ragged; every byte is right."""
    import torch
    for w, h, pitch in LAST_ROW[s]:
        span = (h - 1) * pitch + w
        host = content(span, 1, 3)[0].copy()
        grid = window(host, 0, w, h, pitch)
        d_src = torch.from_numpy(host).cuda()      # an allocation of exactly the span: the grid's last byte is its last
        sw, sh = -(-w >> s), -(-h >> s)
        d_dst = torch.full((sh * sw,), SENTINEL, dtype=torch.uint8, device="cuda")
        plan = make_plan(S, [[d_src.data_ptr(), d_dst.data_ptr(), w, h, pitch, sw]], s)
        assert plan[0].interior_tiles == (0 if sh < 128 else (sw // 128) * 2), (w, h, plan[0].interior_tiles)
        for r in (1, 2, 5, 6):
            for interp in (1, 0):
                assert launch(S, plan, s + r, interp) == OK, S.last_error()
                torch.cuda.synchronize()
                want = reference(oracle, grid, None, s + r, interp, s)
                assert (d_dst.cpu().numpy().reshape(sh, sw) == want).all(), (w, h, pitch, r, interp)
                d_dst.fill_(SENTINEL)
        assert (d_src.cpu().numpy() == host).all()


# ------------------------------------------------------------------------------------ 4. off-lattice and gap bytes
@pytest.mark.parametrize("s", (1, 2, 3))
def test_off_lattice_and_gap_bytes_never_influence_a_result(S, oracle, s):
    import torch
    p = Parents(S, [(256, 128), (130, 66), (301, 203), (1, 70)], s, (True, False), seed=90 + s, gaps=(61, 16))
    plan = p.plan()
    levels = s + 4
    assert launch(S, plan, levels, 1) == OK, S.last_error()
    torch.cuda.synchronize()
    first = p.d_dst.cpu().numpy().copy()
    assert (first == p.expect(oracle, levels, 1)).all()
    # every byte of the source parent that is not on a grid's stride-2**s lattice is rewritten: gaps, off-lattice bytes, the rest
    keep = np.zeros(p.h_src.shape, bool)
    for (w, h), pt, o in zip(p.grids, p.pitch, p.off):
        window(keep, o[0], w, h, pt[0])[::1 << s, ::1 << s] = True
    noise = np.random.default_rng(SEED0 + 2599).integers(0, 256, p.h_src.shape, dtype=np.uint8)
    p.h_src = np.where(keep, p.h_src, noise)
    assert (p.h_src != noise).any() and (~keep).sum() > keep.sum()
    p.d_src.copy_(torch.from_numpy(p.h_src))
    p.d_dst.fill_(SENTINEL)
    assert launch(S, plan, levels, 1) == OK, S.last_error()
    torch.cuda.synchronize()
    assert (p.d_dst.cpu().numpy() == first).all(), "bytes off the lattice changed the output"
    assert (p.d_src.cpu().numpy() == p.h_src).all()


# ------------------------------------------------------------------------------------------------------ 5. an atlas
def test_atlas_of_grids_into_a_canvas_of_thumbnails(S, oracle):
    """Grids side by side in one 1536-byte-pitch canvas of random bytes -- window origins on a line, 64 B into one and at odd x,
    two windows overlapping -- decoded at s = 1 and 2 into thumbnails side by side, in another order, in an 896-byte-pitch canvas."""
    import torch
    SP, DP, rows = 1536, 896, 420
    # (x, y, w, h) in the source canvas; the last overlaps the first
    wins = [(0, 0, 512, 256), (512 + 64, 3, 300, 201), (901, 0, 255, 129), (0, 260, 513, 130), (640, 264, 257, 150), (100, 40, 259, 131)]
    rng = np.random.default_rng(SEED0 + 2560)
    h_src = rng.integers(0, 256, rows * SP, dtype=np.uint8)
    d_src = torch.from_numpy(h_src).cuda()
    for s in (1, 2):
        d_dst = torch.full((rows * DP,), SENTINEL, dtype=torch.uint8, device="cuda")
        want = np.full(rows * DP, SENTINEL, np.uint8)
        pairs, places, x, y, rowh = [], [], 0, 0, 0
        for i in (3, 0, 5, 1, 4, 2):
            wx, wy, w, h = wins[i]
            sw, sh = -(-w >> s), -(-h >> s)
            if x + sw > DP:
                x, y, rowh = 0, y + rowh + 1, 0
            pairs.append([d_src.data_ptr() + wy * SP + wx, d_dst.data_ptr() + y * DP + x, w, h, SP, DP])
            places.append((i, x, y, sw, sh))
            x, rowh = x + sw + (i % 3), max(rowh, sh)
        plan = make_plan(S, pairs, s)
        assert plan[0].count == 6
        for r, interp in ((2, 1), (4, 0), (5, 1), (7, 1)):
            assert launch(S, plan, s + r, interp) == OK, S.last_error()
            torch.cuda.synchronize()
            for i, x, y, sw, sh in places:
                wx, wy, w, h = wins[i]
                window(want, y * DP + x, sw, sh, DP)[...] = reference(oracle, window(h_src, wy * SP + wx, w, h, SP), ("atlas", i), s + r, interp, s)
            got = d_dst.cpu().numpy()
            assert (got == want).all(), "atlas s%d r%d: %d bytes differ" % (s, r, int((got != want).sum()))
            d_dst.fill_(SENTINEL)
    assert (d_src.cpu().numpy() == h_src).all()


# ------------------------------------------------------------------------------------- 6. plan reuse, graph capture
def test_plan_reuse_and_graph_replay_on_new_contents(S, oracle):
    import torch
    p = Parents(S, MIXED, 1, (False, True), seed=110)
    plan = p.plan()
    levels = 5
    for variant in (0, 1):
        p.fill(variant)
        assert launch(S, plan, levels, 1) == OK, S.last_error()
        p.check(oracle, levels, 1, "reuse %d" % variant)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = launch(S, plan, levels, 1, stream=side.cuda_stream)
    assert st == OK, S.last_error()
    p.untouched("capturing must not run the launch")
    for variant in (2, 3):
        p.fill(variant)
        g.replay()
        p.check(oracle, levels, 1, "replay %d" % variant)


# --------------------------------------------------------------------------------------- 7. every instantiation
@pytest.mark.parametrize("s", (1, 2, 3))
@pytest.mark.parametrize("r", (3, 6))
@pytest.mark.parametrize("interp", (0, 1))
def test_one_call_per_instantiation(S, oracle, interp, r, s):
    """k_dec_sviews<interp, SEEDED = 0 | 2, SH = 1 | 2 | 0> on a list with an interior tile and ragged ones."""
    p = Parents(S, [(256, 128), (130, 66)], s, True, seed=130, gaps=(16, 3))
    plan = p.plan()
    assert plan[0].interior_tiles == 5 and plan[0].edge_tiles == 3
    assert launch(S, plan, s + r, interp) == OK, S.last_error()
    p.check(oracle, s + r, interp, "instantiation i%d r%d s%d" % (interp, r, s))


# ------------------------------------------------------------------------------------------------------- 8. Python
def test_python_routes_fused_and_composed(S, oracle):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    shapes = [(300, 200), (129, 65), (0, 5), (64, 64), (200, 1)]
    for s, interp, Interp in ((1, 1, Crossed), (2, 0, LeftTop)):
        p = Parents(S, shapes, s, (True, False), seed=150 + s)
        dec = H.Decoder(Interp())
        plan = H.ScaledViewPlan(p.views(), s)
        assert plan.fused and plan.info.count == 4 and plan.shift == s and len(plan) == 5
        # the fused route, then what the launch does not serve: levels <= shift (the grid's own lattice), r = 9
        for levels in (s + 3, s + 7, s, 1, s + 9):
            outs = dec.decode_scaled_views(plan, levels)
            assert len(outs) == 5 and all(o.data_ptr() == d.data_ptr() for o, (_, d) in zip(outs, p.views()) if o.numel())
            p.check(oracle, levels, interp, "python s%d L%d" % (s, levels))
    # a plan of shift 0 is refused by the library and composed: the full decode
    p = Parents(S, shapes, 0, True, seed=160)
    plan = H.ScaledViewPlan(p.views(), 0)
    assert not plan.fused and "hgi_views_plan" in plan.reason and plan.blob is None
    H.Decoder(Crossed()).decode_scaled_views(plan, 4)
    p.check(oracle, 4, 1, "python shift 0")
    # the refusals of the launch leave the destination untouched
    p = Parents(S, shapes, 1, True, seed=161)
    cplan = p.plan()
    for levels, interp, want in ((0, 1, EUNSUPPORTED), (1, 1, EUNSUPPORTED), (10, 0, EUNSUPPORTED), (32, 1, EINVAL), (4, 2, EINVAL)):
        assert launch(S, cplan, levels, interp) == want, (levels, interp, S.last_error())
    assert S.lib().hgi_sviews_decode_dev(None, cplan[1].data_ptr() + 8, ctypes.addressof(cplan[0]), 4, 1) == EINVAL
    p.untouched("refusals")
    # a shape that does not match is the caller's fault, seen before any launch
    with pytest.raises(ValueError, match="pair 0"):
        H.ScaledViewPlan([(torch.zeros((10, 10), dtype=torch.uint8, device="cuda"), torch.zeros((5, 6), dtype=torch.uint8, device="cuda"))], 1)
