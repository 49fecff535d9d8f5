"""GPU suite of the typed view lists (libhgi_tviews.so, include/hgi_tviews.h; Encoder.encode_typed_views): every case reads its
frames out of float parents -- the uint8 contents of test_views_gpu.content lifted to elements (tests/typed_reference.py, lift:
each pixel value becomes one of its preimages under the launch's (scale, bias), so the converted image is known exactly) in
parents whose other elements hold NaN, +-inf and random bits -- and writes into sentinel-filled uint8 parents that are compared
WHOLE, as raw bytes, against an expected parent built on the CPU from the oracle's encode of the known uint8 image -- never from
libhgi_hip.so, never from the library under test; the float parents must come back unmodified.
  1. the mapped view lists' mixed list (17 non-empty views up to 513 wide, every width residue mod 8, sides below a tile,
     (128, 64), (256, 128), empty entries) plus two odd widths that, at E = 2, are placed with the end of their span 2 bytes in
     front of a page boundary and 2 bytes behind one; separate parents, pitches drawn per side (in elements on the read side),
     source bases on 128-B lines and, on odd entries, at E-aligned addresses that are not 16-byte aligned: levels 1-5 x both
     interpolators x the medium and the identity table x float16, bfloat16 and float32 x the (scale, bias) pairs of
     typed_reference.PAIRS (bfloat16 under (-3.5, 300) on contents moved to the nearest values it can reach); the sub-lists that
     change the map's shape, the kinds and pairs taking turns;
  2. the cone: levels 6, 7, 8 on five shapes at two pitches, both E -- the SEEDED = 2 kernels;
  3. the padded tensor: the frames of a NaN-filled [N, Hmax, Wp] tensor of padded_batch encoded into an aligned_arena whose gaps
     keep their sentinel;
  4. an atlas at E = 4: float windows side by side in one canvas's rows, two source windows overlapping;
  5. one plan launched twice on new contents with two (scale, bias) pairs, then captured into a graph and replayed on new contents;
  6. the Python surface: fused, composed for a depth the launch does not serve and for a list with one entry that breaks the
     page rule;
  7. one call per kernel instantiation: 16 calls."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import test_mviews_gpu as TM
import test_views_gpu as TV
import typed_reference as TR
from conftest import SEED0

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1, 4      # hgi_status (include/hgi.h)
SENTINEL = TV.SENTINEL
GAPS = TV.GAPS
UINT = {2: np.uint16, 4: np.uint32}
SINT = {2: np.int16, 4: np.int32}
F16, BF16, F32 = "float16", "bfloat16", "float32"
ESIZE = {F16: 2, BF16: 2, F32: 4}
EKIND = {F16: 0, BF16: 1, F32: 0}
P0, P1, P2 = TR.PAIRS
# (kind, (scale, bias)) per element size: every kind under every pair.  bfloat16 has no preimage of some pixel values under P2
# (its steps there are 1.75 pixels): there the contents are moved to the nearest reachable values first (reach), so that the
# converted image is still known exactly.
CHOICES = {2: ((F16, P0), (F16, P1), (F16, P2), (BF16, P0), (BF16, P1), (BF16, P2)), 4: ((F32, P0), (F32, P1), (F32, P2))}
# NaN, +inf, -inf of each kind, planted among the random bits around the views
SPECIAL = {2: (0x7E00, 0x7C00, 0xFC00, 0x7FC1, 0x7F80, 0xFF80), 4: (0x7FC00000, 0x7F800000, 0xFF800000, 0xFFFFFFFF, 0x7F800001, 0x7FC00001)}
# (width, height): the list of case 1.  The last two are the odd widths whose spans end 2 bytes before / behind a page boundary at E = 2
PAGE_ENDS = {len(TM.MIXED): 4094, len(TM.MIXED) + 1: 2}
MIXED = TM.MIXED + [(133, 5), (135, 67)]
COMBOS = tuple(itertools.product(range(1, 6), (1, 0), ("medium", "identity")))
# the list has what the cases need
assert MIXED[:len(TM.MIXED)] == TM.MIXED and sum(1 for w, h in TM.MIXED if w and h) == 17 and max(w for w, h in MIXED) == 513
assert set(w % 8 for w, h in MIXED if w and h) == set(range(8))
assert any(w == 0 or h == 0 for w, h in MIXED) and any(w < 128 or h < 64 for w, h in MIXED) and (128, 64) in MIXED and (256, 128) in MIXED
assert all(MIXED[i][0] % 2 == 1 for i in PAGE_ENDS) and sorted(PAGE_ENDS.values()) == [2, 4094]
assert set(k for c in CHOICES.values() for k, _ in c) == {F16, BF16, F32} and set(p for c in CHOICES.values() for _, p in c) == set(TR.PAIRS)


@pytest.fixture(scope="module")
def T():
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("tviews")


@functools.lru_cache(maxsize=None)
def reach(kind, pair):
    """(256,) uint8: every pixel value moved to the nearest one that some finite `kind` element converts to under `pair` (the
    identity wherever typed_reference.preimages has a bank: everywhere but bfloat16 under P2)."""
    if ESIZE[kind] == 4:
        return np.arange(256, dtype=np.uint8)
    ok = TR.reachable(kind, *pair).astype(np.int64)
    v = np.arange(256)
    r = ok[np.abs(v[:, None] - ok[None, :]).argmin(axis=1)].astype(np.uint8)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def bank(kind, pair):
    """(256, 4) element bit patterns: preimages of every pixel value under `pair` (of the value reach() moves it to, where it
    has none of its own), checked against the restated conversion."""
    r = reach(kind, pair)
    if (r == np.arange(256)).all():
        b = TR.preimages(kind, *pair)
    else:      # typed_reference.preimages refuses a pair with unreachable values: the smallest, the largest and a middle preimage
        bits = np.arange(1 << 16, dtype=np.uint16)
        x = TR.elements(kind, bits)
        val = TR.widen(x)
        q, fin = TR.quantize(x, *pair), np.isfinite(TR.widen(x))
        b = np.zeros((256, 4), np.uint16)
        for v in np.unique(r):
            m = np.flatnonzero(fin & (q == v))
            m = m[np.argsort(val[m], kind="stable")]
            b[v] = bits[m[[0, m.size - 1, m.size // 2, m.size // 3]]]
        b = b[r]
    assert (TR.quantize(TR.elements(kind, b), *pair) == r[:, None]).all()
    b.setflags(write=False)
    return b


def noise_bytes(rng, n, E):
    """n bytes (a multiple of 4) of random bits with NaN and +-inf patterns planted at every third element."""
    raw = rng.integers(0, 256, n, dtype=np.uint8)
    el = raw.view(UINT[E])
    at = np.arange(0, el.size, 3)
    el[at] = np.array(SPECIAL[E], UINT[E])[(at // 3) % len(SPECIAL[E])]
    return raw


def elem_window(parent, off, w, h, pitch, E):
    """The (h, w) E-byte elements of a window of a byte parent whose rows lie `pitch` BYTES apart, as bit patterns."""
    return np.lib.stride_tricks.as_strided(parent[off:off + (parent.size - off) // E * E].view(UINT[E]), (h, w), (pitch, E))


def page_ok(ptr, w, h, pitch, E):
    """include/hgi_tviews.h: 2-byte elements of an odd width are served iff the frame's span does not end a 4-KiB page."""
    return E == 4 or w % 2 == 0 or (ptr + (h - 1) * (pitch if h > 1 else w * E) + w * E) % 4096 != 0


class Parents:
    """A list of (w, h) views placed in a source parent of E-byte elements (NaN, +-inf and random bits; view i on a 128-byte line
    -- even i -- or at an E-aligned address that is not 16-byte aligned -- odd i --, rows (w + gap) * E bytes apart) and a
    destination parent of sentinel bytes (view i on a 128-byte line or at an odd address, rows w + gap bytes apart), the gaps
    drawn per side.  `ends`: {index: residue} places an entry so that its source span ends at that residue of a 4-KiB page."""

    def __init__(self, T, shapes, E, seed, gaps=None, ends=None):
        import torch
        self.T, self.shapes, self.E = T, list(shapes), E
        ends = ends or {}
        rng = np.random.default_rng(SEED0 + 2300 + seed)
        self.pitch = [(E * (w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[0])), w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[1]))
                      for w, h in self.shapes]
        room = [sum(h * p[s] + 512 for (w, h), p in zip(self.shapes, self.pitch)) + 8192 + 4096 * len(ends) for s in range(2)]
        room[0] = -(-room[0] // 4) * 4
        self.h_src = noise_bytes(rng, room[0], E)
        self.d_src = torch.empty((room[0],), dtype=torch.uint8, device="cuda")
        self.d_dst = torch.empty((room[1],), dtype=torch.uint8, device="cuda")
        assert self.d_src.data_ptr() % 128 == 0
        self.off = []
        at = [64, 192]
        for i, ((w, h), p) in enumerate(zip(self.shapes, self.pitch)):
            o = []
            for side in range(2):
                a = -(-at[side] // 128) * 128
                if i % 2:
                    a += E * (2 * (i % 3) + 1) if side == 0 else 2 * (i % 5) + 1      # 1, 3, 5 elements: never 16-byte aligned; odd bytes
                if side == 0 and w and h:
                    if i in ends and E == 2:
                        a += (ends[i] - (self.d_src.data_ptr() + a + (h - 1) * p[0] + w * E)) % 4096
                        assert (self.d_src.data_ptr() + a + (h - 1) * p[0] + w * E) % 4096 == ends[i]
                    while not page_ok(self.d_src.data_ptr() + a, w, h, p[0], E):
                        a += 128
                o.append(a)
                at[side] = a + (h * p[side] if w and h else 0) + 5
            assert o[0] % E == 0 and (i % 2 == 0 or i in ends or o[0] % 16)
            self.off.append(tuple(o))
        assert at[0] <= room[0] and at[1] <= room[1]
        self.kind = self.pair = self.variant = None

    def fill(self, kind, pair, variant=0):
        """New source contents: TV.content(w, h, variant) lifted to `kind` elements under `pair` in every window, the elements
        around them unchanged."""
        import torch
        assert ESIZE[kind] == self.E
        self.kind, self.pair, self.variant = kind, pair, variant
        for i, ((w, h), p, o) in enumerate(zip(self.shapes, self.pitch, self.off)):
            if w and h:
                img = reach(kind, pair)[TV.content(w, h, variant)]
                bits = TR.lift(img, bank(kind, pair), i)
                assert (TR.quantize(TR.elements(kind, bits), *pair) == img).all()      # the converted image is the known one
                elem_window(self.h_src, o[0], w, h, p[0], self.E)[...] = bits
        self.d_src.copy_(torch.from_numpy(self.h_src))
        self.d_dst.fill_(SENTINEL)

    def plan(self):
        F = self.T
        n = len(self.shapes)
        arr = (F.TViewPair * n)(*[F.TViewPair(self.d_src.data_ptr() + o[0] if w and h else 0, self.d_dst.data_ptr() + o[1] if w and h else 0, w, h, p[0], p[1])
                                  for (w, h), p, o in zip(self.shapes, self.pitch, self.off)])
        return make_plan(F, arr, n, self.E)

    def launch(self, plan, levels, interp, lut, stream=None):
        return launch(self.T, plan, self.kind, self.pair, levels, interp, lut, stream)

    def expect(self, oracle, levels, interp, lut_name):
        want = np.full(self.d_dst.shape[0], SENTINEL, np.uint8)
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                r = reach(self.kind, self.pair)
                moved = bool((r != np.arange(256)).any())      # (the view lists' references are shared wherever nothing is moved)
                key = (w, h, self.variant) + ((self.kind, self.pair) if moved else ())
                TV.Parents.window(want, o[1], w, h, p[1])[...] = TV.reference(oracle, r[TV.content(w, h, self.variant)], key, levels, interp, lut_name)
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


def make_plan(F, arr, n, E):
    """hgi_tviews_plan of a ctypes array of pairs: (info, the blob as a device tensor kept alive by the caller)."""
    import torch
    L = F.lib()
    size = L.hgi_tviews_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    info = F.TViewsInfo()
    st = L.hgi_tviews_plan(ctypes.addressof(arr), n, E, host.ctypes.data, size, ctypes.addressof(info))
    assert st == OK, F.last_error()
    assert info.magic == F.MAGIC and info.plan_bytes <= size and info.elem_size == E
    blob = torch.from_numpy(host[:max(int(info.plan_bytes), 16)].copy()).cuda()
    return info, blob


def launch(F, plan, kind, pair, levels, interp, lut, stream=None):
    info, blob = plan
    lut = np.ascontiguousarray(lut, np.uint8)
    return F.lib().hgi_tviews_encode_dev(stream, blob.data_ptr(), ctypes.addressof(info), EKIND[kind], float(np.float32(pair[0])), float(np.float32(pair[1])),
                                         levels, interp, lut.ctypes.data)


def run_all(F, oracle, parents, combos, what, rotate):
    """Encode every (levels, interpolator, table) of `combos` under the (kind, pair) choices of the parents' element size -- all of
    them, or with `rotate` taking turns over the combos -- each launch against the oracle."""
    plan = parents.plan()
    choices = CHOICES[parents.E]
    luts = TV.tables(oracle)
    for ci, (kind, pair) in enumerate(choices):
        parents.fill(kind, pair)
        for n, (levels, interp, name) in enumerate(combos):
            if rotate and n % len(choices) != ci:
                continue
            assert parents.launch(plan, levels, interp, luts[name]) == OK, F.last_error()
            parents.check(oracle, levels, interp, name, "%s %s (%g, %g) L%d i%d %s" % (what, kind, pair[0], pair[1], levels, interp, name))
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
@pytest.mark.parametrize("E", (2, 4))
def test_mixed_list_in_separate_parents(T, oracle, E):
    p = Parents(T, MIXED, E, seed=1 + E, ends=PAGE_ENDS)
    info, _ = run_all(T, oracle, p, COMBOS, "mixed", rotate=False)
    assert info.count == 19 and info.interior_tiles == sum((w // 128) * (h // 64) for w, h in MIXED) == 31 and info.max_width == 513
    assert len(set(p.pitch)) > 6 and any(a != E * b for a, b in p.pitch)
    if E == 2:
        ends = [(p.d_src.data_ptr() + p.off[i][0] + (MIXED[i][1] - 1) * p.pitch[i][0] + 2 * MIXED[i][0]) % 4096 for i in sorted(PAGE_ENDS)]
        assert ends == [4094, 2]


@pytest.mark.parametrize("name", sorted(TV.SUBLISTS))
def test_sublists_that_change_the_maps_shape(T, oracle, name):
    for E in (2, 4):
        p = Parents(T, TV.SUBLISTS[name], E, seed=10 + sorted(TV.SUBLISTS).index(name))
        info, _ = run_all(T, oracle, p, COMBOS, name, rotate=True)
        if name == "no-edge":
            assert info.edge_tiles == 0 and info.interior_tiles == 5
        if name == "nint-2":
            assert info.interior_tiles == 2
        if name in ("first", "prefix-2", "prefix-3", "prefix-4"):
            assert info.interior_tiles == 0


# ---------------------------------------------------------------------------------------------------- 2. the cone
@pytest.mark.parametrize("E", (2, 4))
@pytest.mark.parametrize("gap", (61, 0))
def test_cone_levels(T, oracle, gap, E):
    """Levels 6, 7, 8 (four fused levels under a cone on the frame's own samples through its byte pitch): the SEEDED = 2 kernels."""
    p = Parents(T, TV.CONE, E, seed=20 + gap, gaps=(gap, gap))
    run_all(T, oracle, p, tuple(itertools.product((6, 7, 8), (1, 0), ("medium", "identity"))), "cone gap %d" % gap, rotate=True)


# ------------------------------------------------------------------------------------------- 3. the padded tensor
def to_torch(bits, dtype):
    """Element bit patterns -> a torch tensor of `dtype` with those bits (host)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(SINT[bits.dtype.itemsize])).view(dtype)


@pytest.mark.parametrize("kind", (F16, BF16, F32))
def test_padded_tensor_into_an_aligned_arena(T, oracle, kind):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    dtype, E, pair = getattr(torch, kind), ESIZE[kind], P1
    shapes = [(h, w) for w, h in TM.MIXED]
    batch, frames = H.padded_batch(shapes, dtype, fill=float("nan"))
    N, Hmax, Wp = batch.shape
    assert (N, Hmax) == (len(TM.MIXED), 203) and Wp * E % 128 == 0 and batch.data_ptr() % 128 == 0
    assert bool(torch.isnan(batch).all())
    for i, ((h, w), f) in enumerate(zip(shapes, frames)):
        if h and w:
            f.copy_(to_torch(TR.lift(TV.content(w, h, 0), bank(kind, pair), i), dtype))
    before = batch.view(torch.uint8).cpu().numpy().copy()
    total, places = H.aligned_arena(shapes)
    arena = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    grids = H.views.arena_views(arena, shapes, places)
    plan = H.TypedViewPlan(zip(frames, grids), dtype)
    assert plan.fused and plan.info.count == 17 and plan.elem_size == E, plan.reason
    for levels in (3, 7):
        enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), levels)
        outs = enc.encode_typed_views(plan, *pair)
        torch.cuda.synchronize()
        want = np.full(total, SENTINEL, np.uint8)
        for (h, w), (o, pitch) in zip(shapes, places):
            if h and w:
                TV.Parents.window(want, o, w, h, pitch)[...] = TV.reference(oracle, TV.content(w, h, 0), (w, h, 0), levels, 1, "medium")
        got = arena.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "padded %s L%d: %d bytes of the arena differ, the first at %d" % (kind, levels, bad.size, int(bad[0]))
        assert (want == SENTINEL).sum() > 1000      # the arena's gaps were compared
        assert len(outs) == len(shapes) and outs[0].data_ptr() == arena.data_ptr() and outs[0].dtype == torch.uint8
        arena.fill_(SENTINEL)
    assert (batch.view(torch.uint8).cpu().numpy() == before).all(), "the padded tensor was modified"


# --------------------------------------------------------------------------------------------------- 4. the atlas
def test_atlas_side_by_side(T, oracle):
    import torch
    F, E, kind, pair = T, 4, F32, P2
    rng = np.random.default_rng(SEED0 + 2400)
    SPE, DP = 1152, 1024      # the float canvas' rows in elements, the grid canvas' in bytes
    SP = SPE * E
    order = list(range(len(TM.MIXED)))
    shapes = TM.MIXED
    src_at, src_h = TV.shelves(shapes, SPE, order, lambda i: i % 3)            # x in elements: on lines, mid-line, at odd elements
    dst_at, dst_h = TV.shelves(shapes, DP, order[::-1], lambda i: (i + 1) % 3)
    # two source windows overlap: the 129 x 65 view reads out of the 256 x 128 view's window
    i_small, i_big = shapes.index((129, 65)), shapes.index((256, 128))
    src_at[i_small] = (src_at[i_big][0] + 31, src_at[i_big][1] + 17)
    h_src = noise_bytes(rng, src_h * SP + 8192, E)
    for i, (w, h) in enumerate(shapes):
        if w and h and i != i_small:
            x, y = src_at[i]
            elem_window(h_src, 128 + y * SP + x * E, w, h, SP, E)[...] = TR.lift(TV.content(w, h, 0), bank(kind, pair), i)
    d_src = torch.from_numpy(h_src).cuda()
    d_dst = torch.full((dst_h * DP + 8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    pairs = []
    for i, (w, h) in enumerate(shapes):
        if w and h:
            (sx, sy), (dx, dy) = src_at[i], dst_at[i]
            pairs.append(F.TViewPair(d_src.data_ptr() + 128 + sy * SP + sx * E, d_dst.data_ptr() + 128 + dy * DP + dx, w, h, SP, DP))
        else:
            pairs.append(F.TViewPair(0, 0, w, h, 0, 0))
    plan = make_plan(F, (F.TViewPair * len(pairs))(*pairs), len(pairs), E)
    luts = TV.tables(oracle)
    for levels in (3, 7):
        assert launch(F, plan, kind, pair, levels, 1, luts["medium"]) == OK, F.last_error()
        torch.cuda.synchronize()
        want = np.full(d_dst.shape[0], SENTINEL, np.uint8)
        for i, (w, h) in enumerate(shapes):
            if w and h:
                (sx, sy), (dx, dy) = src_at[i], dst_at[i]
                img = TR.quantize(TR.elements(kind, elem_window(h_src, 128 + sy * SP + sx * E, w, h, SP, E)), *pair)
                assert i == i_small or (img == TV.content(w, h, 0)).all()
                TV.Parents.window(want, 128 + dy * DP + dx, w, h, DP)[...] = TV.reference(oracle, img, ("tviews atlas", i), levels, 1, "medium")
        got = d_dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "atlas L%d: %d bytes of the canvas differ, the first at %d" % (levels, bad.size, int(bad[0]))
        assert (want == SENTINEL).sum() > dst_h * DP // 4      # the sentinel between and around the windows was compared
        assert (d_src.cpu().numpy() == h_src).all()
        d_dst.fill_(SENTINEL)


# ------------------------------------------------------------------------------------- 5. plan reuse and capture
def test_plan_reuse_and_graph_capture(T, oracle):
    import torch
    p = Parents(T, MIXED, 2, seed=3, ends=PAGE_ENDS)
    plan = p.plan()
    lut = TV.tables(oracle)["medium"]
    for variant, pair in ((0, P0), (1, P1)):
        p.fill(F16, pair, variant)
        assert p.launch(plan, 4, 1, lut) == OK, T.last_error()
        p.check(oracle, 4, 1, "medium", "launch %d of one plan" % variant)
    p.fill(F16, P0, 1)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = p.launch(plan, 4, 1, lut, stream=side.cuda_stream)
    assert st == OK, T.last_error()
    torch.cuda.synchronize()
    assert (p.d_dst.cpu().numpy() == SENTINEL).all(), "capturing must not run the launch"
    p.fill(F16, P0, 2)
    g.replay()
    p.check(oracle, 4, 1, "medium", "replayed on new contents")


# --------------------------------------------------------------------------------------------- 6. the Python surface
def test_python_surface_fused_and_composed(T, oracle):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    shapes = [(65, 129), (64, 128), (1, 200), (0, 3), (203, 301)]      # (height, width)
    total, places = H.aligned_arena(shapes)
    enc = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 4)
    deep = H.Encoder(Crossed(), Linear.from_level(QuantizationLevel.Medium), 9)
    lut = TV.tables(oracle)["medium"]
    for kind, pair in ((BF16, P0), (F32, P2)):
        dtype, E = getattr(torch, kind), ESIZE[kind]
        # the float arena: aligned_arena's layout of rows of w * E bytes, NaN between the frames' rows
        ftotal, fplaces = H.aligned_arena([(h, w * E) for h, w in shapes])
        farena = torch.full((ftotal // E,), float("nan"), dtype=dtype, device="cuda")
        raw = farena.view(torch.uint8)
        srcs = [raw[o:o + h * p].view(h, p).view(dtype)[:, :w] if h and w else torch.empty((h, w), dtype=dtype, device="cuda") for (h, w), (o, p) in zip(shapes, fplaces)]
        imgs = [TV.content(w, h, 0) if h and w else None for h, w in shapes]
        for i, (s, img) in enumerate(zip(srcs, imgs)):
            if img is not None:
                s.copy_(to_torch(TR.lift(img, bank(kind, pair), i), dtype))
        before = raw.cpu().numpy().copy()
        arena = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        grids = H.views.arena_views(arena, shapes, places)
        plan = H.TypedViewPlan(zip(srcs, grids), dtype)
        assert plan.fused and plan.info.count == 4 and plan.elem_size == E, plan.reason
        got = enc.encode_typed_views(plan, *pair)
        torch.cuda.synchronize()
        want = np.full(total, SENTINEL, np.uint8)
        for (h, w), (o, pitch), img in zip(shapes, places, imgs):
            if img is not None:
                TV.Parents.window(want, o, w, h, pitch)[...] = TV.reference(oracle, img, (w, h, 0), 4, 1, "medium")
        assert (arena.cpu().numpy() == want).all() and (raw.cpu().numpy() == before).all()
        assert len(got) == 5 and got[0].data_ptr() == arena.data_ptr() and got[0].dtype == torch.uint8
        # more levels than the one launch serves: composed from one encode_typed per view, the same bytes
        small = H.TypedViewPlan([(srcs[1], grids[1])], dtype)
        arena.fill_(SENTINEL)
        deep.encode_typed_views(small, *pair)
        torch.cuda.synchronize()
        assert (grids[1].cpu().numpy() == oracle.encode(imgs[1], 9, lut, 1)).all()
    # one entry of 2-byte elements and an odd width whose span ends on a page boundary: the plan is not fused, the calls are composed
    w, h, pe = 131, 66, 147      # pitch in elements
    span = (h - 1) * pe * 2 + 2 * w
    parent = torch.full((span // 2 + 3 * 2048,), float("nan"), dtype=torch.float16, device="cuda")
    lead = ((-(parent.data_ptr() + span)) % 4096) // 2
    assert not page_ok(parent.data_ptr() + 2 * lead, w, h, 2 * pe, 2)
    bad_src = parent[lead:lead + (h - 1) * pe + w].as_strided((h, w), (pe, 1))
    good_src = torch.empty((65, 129 + 3), dtype=torch.float16, device="cuda")[:, :129]
    imgs = [TV.content(w, h, 1), TV.content(129, 65, 1)]
    for i, (s, img) in enumerate(zip((bad_src, good_src), imgs)):
        s.copy_(to_torch(TR.lift(img, bank(F16, P1), i), torch.float16))
    outs = [torch.full((h, w + 5), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((65, 129 + 3), SENTINEL, dtype=torch.uint8, device="cuda")]
    plan = H.TypedViewPlan([(bad_src, outs[0][:, :w]), (good_src, outs[1][:, :129])], torch.float16)
    assert not plan.fused and "tail" in plan.reason and "view 0" in plan.reason
    enc.encode_typed_views(plan, *P1)
    torch.cuda.synchronize()
    for img, out, ww in ((imgs[0], outs[0], w), (imgs[1], outs[1], 129)):
        got = out.cpu().numpy()
        assert (got[:, :ww] == oracle.encode(img, 4, lut, 1)).all() and (got[:, ww:] == SENTINEL).all()


# ------------------------------------------------------------------------------- 7. one call per instantiation
INSTANCES = [(i, t, s, e) for i in (1, 0) for t in ("identity", "medium") for s in (0, 2) for e in (2, 4)]


@functools.lru_cache(maxsize=None)
def _small(T, E):
    p = Parents(T, [(129, 65), (128, 64), (70, 1)], E, seed=60)
    p.fill(F16 if E == 2 else F32, P1)
    return p


@pytest.mark.parametrize("interp,table,seeded,E", INSTANCES, ids=["i%d-%s-s%d-e%d" % t for t in INSTANCES])
def test_one_call_per_instantiation(T, oracle, interp, table, seeded, E):
    """k_enc_tviews<INTERP, IDENT, SEEDED, E>, sixteen kernels, one launch each against the oracle."""
    assert len(INSTANCES) == 16
    p = _small(T, E)
    levels = 6 if seeded else 3
    assert p.launch(p.plan(), levels, interp, TV.tables(oracle)[table]) == OK, T.last_error()
    p.check(oracle, levels, interp, table, "interp %d %s seeded %d E %d" % (interp, table, seeded, E))
