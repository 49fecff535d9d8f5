"""GPU suite of the mapped view lists (libhgi_mviews.so, include/hgi_mviews.h; Decoder.decode_mapped_views): every case reads its
grids out of parents of random bytes (any byte plane is a valid grid) and writes into sentinel-filled parents that are compared
WHOLE, as raw bytes, against an expected parent built on the CPU from table[oracle.decode(...)] -- never from libhgi_hip.so, never
from the library under test; the grids and the table must come back unmodified.  The tables: random E-byte bit patterns (NaN
payloads, signalling NaNs, signed zeros among them: the library moves bits) and affine_table(dtype).
  1. the view lists' mixed list plus four entries that make the widths cover every residue mod 8 (every b64 / b32 / b16 split of
     the piece that straddles the right edge at E = 2, every residue mod 4 at E = 4), in separate parents, gaps drawn per side (in
     elements on the written side), destination bases on 128-B lines and at E-aligned addresses that are not 16-byte aligned:
     levels 1-5 x both interpolators x both tables x E in {2, 4}; the same on the sub-lists that change the map's shape;
  2. the cone: levels 6, 7, 8 on five shapes at two pitches, both E -- the SEEDED = 2 kernels;
  3. the padded tensor: the list written into the [N, Hmax, Wp] tensor of padded_batch, the padding keeps its sentinel;
  4. an atlas at E = 4: float windows side by side in one canvas's rows, two grids overlapping;
  5. one plan launched twice on new contents with two different tables, then captured into a graph and replayed on new contents;
  6. the Python surface: fused, and composed for a list with one entry that breaks the page rule;
  7. one call per kernel instantiation: 8 calls;
  8. a table inside the bounding interval of the outputs is refused and nothing is written."""
import ctypes
import functools

import numpy as np
import pytest

import test_views_gpu as TV
from conftest import SEED0

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1, 4      # hgi_status (include/hgi.h)
SENTINEL = TV.SENTINEL
GAPS = TV.GAPS
UINT = {2: np.uint16, 4: np.uint32}
# (width, height): the list of case 1 -- widths mod 8: 1, 1, 0, 7, 0, 1, -, 0, 7, -, 0, 0, 2, 5, 1 and 3, 4, 6, 2
MIXED = TV.MIXED + [(131, 3), (132, 66), (134, 2), (2, 2)]


@pytest.fixture(scope="module")
def M():
    import companion_layer as CL
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "the gpu suite needs cuda:0"
    from rustyhgi_amd import _ffi
    assert (_ffi.OK, _ffi.EINVAL, _ffi.EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return CL.binding("mviews")


def test_the_list_has_what_the_cases_need():
    assert set(w % 8 for w, h in MIXED if w and h) == set(range(8))
    assert any(w == 0 or h == 0 for w, h in MIXED) and any(w < 128 or h < 64 for w, h in MIXED) and (128, 64) in MIXED and (256, 128) in MIXED
    assert sum((w // 128) * (h // 64) for w, h in MIXED) >= 29 and sum((w // 128) * (h // 64) for w, h in MIXED) % 8 != 0


@functools.lru_cache(maxsize=None)
def tables(E):
    """{name: 256 E-byte bit patterns}: random ones with the special float patterns planted, and affine_table of the float type."""
    from rustyhgi_amd import affine_table
    rng = np.random.default_rng(SEED0 + 2200 + E)
    rnd = rng.integers(0, 1 << (8 * E), 256, dtype=np.uint64).astype(UINT[E])
    # -0, +0, a quiet NaN with a payload, all ones, a signalling NaN, an infinity, a subnormal
    special = {2: (0x8000, 0x0000, 0x7E01, 0xFFFF, 0x7D01, 0xFC00, 0x0001), 4: (0x80000000, 0, 0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0xFF800000, 1)}[E]
    rnd[[0, 1, 2, 3, 127, 128, 255]] = special
    aff = affine_table(np.float16 if E == 2 else np.float32).view(UINT[E]).copy()
    out = {"random": rnd, "affine": aff}
    for t in out.values():
        t.setflags(write=False)
    return out


def device_table(tab):
    import torch
    return torch.from_numpy(tab.view({2: np.int16, 4: np.int32}[tab.dtype.itemsize]).copy()).cuda()


def byte_window(parent, off, w, h, pitch, E):
    """The (h, w * E) bytes of a window of E-byte elements whose rows lie `pitch` BYTES apart."""
    return np.lib.stride_tricks.as_strided(parent[off:], (h, w * E), (pitch, 1))


def mapped(tab, decoded):
    """table[decoded] as rows of bytes."""
    return np.ascontiguousarray(tab[decoded]).view(np.uint8).reshape(decoded.shape[0], -1)


class Parents:
    """A list of (w, h) views placed in a source parent of random bytes (view i at an odd address or on a 128-byte line, rows
    w + gap bytes apart) and a destination parent of sentinel bytes: view i on a 128-byte line (even i) or at an E-aligned address
    that is not 16-byte aligned (odd i), its rows (w + gap) * E bytes apart, the gaps drawn per side."""

    def __init__(self, M, shapes, E, seed, gaps=None, variant=0):
        import torch
        self.M, self.shapes, self.E = M, list(shapes), E
        rng = np.random.default_rng(SEED0 + 2600 + seed)
        self.pitch = [(w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[0]), E * (w + (GAPS[int(rng.integers(0, 6))] if gaps is None else gaps[1])))
                      for w, h in self.shapes]
        room = [sum(h * p[s] + 512 for (w, h), p in zip(self.shapes, self.pitch)) + 8192 for s in range(2)]
        self.h_src = rng.integers(0, 256, room[0], dtype=np.uint8)
        self.d_src = torch.empty((room[0],), dtype=torch.uint8, device="cuda")
        self.d_dst = torch.empty((room[1],), dtype=torch.uint8, device="cuda")
        assert self.d_dst.data_ptr() % 128 == 0
        self.off = []
        at = [64, 192]
        for i, ((w, h), p) in enumerate(zip(self.shapes, self.pitch)):
            o = []
            for side in range(2):
                a = -(-at[side] // 128) * 128
                if i % 2:
                    a += 2 * (i % 5) + 1 if side == 0 else E * (2 * (i % 3) + 1)      # odd bytes; 1, 3, 5 elements: never 16-byte aligned
                while side == 0 and w and h and not TV.tail_ok(self.d_src.data_ptr() + a, w, h, p[0]):
                    a += 128
                o.append(a)
                at[side] = a + (h * p[side] if w and h else 0) + 5
            assert o[1] % E == 0 and (i % 2 == 0 or o[1] % 16)
            self.off.append(tuple(o))
        assert at[0] <= room[0] and at[1] <= room[1]
        self.fill(variant)

    def fill(self, variant):
        """New source contents: TV.content(w, h, variant) in every window, the random bytes around them unchanged."""
        import torch
        self.variant = variant
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                TV.Parents.window(self.h_src, o[0], w, h, p[0])[...] = TV.content(w, h, variant)
        self.d_src.copy_(torch.from_numpy(self.h_src))
        self.d_dst.fill_(SENTINEL)

    def plan(self):
        F = self.M
        n = len(self.shapes)
        arr = (F.MViewPair * n)(*[F.MViewPair(self.d_src.data_ptr() + o[0] if w and h else 0, self.d_dst.data_ptr() + o[1] if w and h else 0, w, h, p[0], p[1])
                                  for (w, h), p, o in zip(self.shapes, self.pitch, self.off)])
        return make_plan(F, arr, n, self.E)

    def expect(self, oracle, levels, interp, tab):
        want = np.full(self.d_dst.shape[0], SENTINEL, np.uint8)
        for (w, h), p, o in zip(self.shapes, self.pitch, self.off):
            if w and h:
                dec = TV.reference(oracle, TV.content(w, h, self.variant), (w, h, self.variant), levels, interp)
                byte_window(want, o[1], w, h, p[1], self.E)[...] = mapped(tab, dec)
        return want

    def check(self, oracle, levels, interp, tab, what):
        import torch
        torch.cuda.synchronize()
        got = self.d_dst.cpu().numpy()
        want = self.expect(oracle, levels, interp, tab)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d bytes of the destination parent differ, the first at %d" % (what, bad.size, int(bad[0]))
        assert (self.d_src.cpu().numpy() == self.h_src).all(), what + ": the source parent was modified"
        self.d_dst.fill_(SENTINEL)


def make_plan(F, arr, n, E):
    """hgi_mviews_plan of a ctypes array of pairs: (info, the blob as a device tensor kept alive by the caller)."""
    import torch
    L = F.lib()
    size = L.hgi_mviews_plan_bytes(n)
    host = np.zeros(max(size, 16), np.uint8)
    info = F.MViewsInfo()
    st = L.hgi_mviews_plan(ctypes.addressof(arr), n, E, host.ctypes.data, size, ctypes.addressof(info))
    assert st == OK, F.last_error()
    assert info.magic == F.MAGIC and info.plan_bytes <= size and info.elem_size == E
    blob = torch.from_numpy(host[:max(int(info.plan_bytes), 16)].copy()).cuda()
    return info, blob


def launch(F, plan, levels, interp, d_table, stream=None):
    info, blob = plan
    return F.lib().hgi_mviews_decode_dev(stream, blob.data_ptr(), ctypes.addressof(info), levels, interp, d_table.data_ptr())


def run_all(F, oracle, parents, levels_set, names, what):
    """Decode with every table at every level with both interpolators: each launch against the oracle."""
    plan = parents.plan()
    E = parents.E
    for name in names:
        tab = tables(E)[name]
        d_tab = device_table(tab)
        for levels in levels_set:
            for interp in (1, 0):
                assert launch(F, plan, levels, interp, d_tab) == OK, F.last_error()
                parents.check(oracle, levels, interp, tab, "%s E%d L%d i%d %s" % (what, E, levels, interp, name))
        assert (d_tab.cpu().numpy().view(UINT[E]) == tab).all(), "the table was modified"
    return plan


# ------------------------------------------------------------------------------------------------ 1. the mixed list
@pytest.mark.parametrize("E", (2, 4))
def test_mixed_list_in_separate_parents(M, oracle, E):
    p = Parents(M, MIXED, E, seed=1 + E)
    info, _ = run_all(M, oracle, p, range(1, 6), ("random", "affine"), "mixed")
    assert info.count == 17 and info.interior_tiles == 30 and info.max_width == 513
    assert len(set(p.pitch)) > 6 and any(b != E * a for a, b in p.pitch)
    assert (info.dst_lo, info.dst_hi) == (p.d_dst.data_ptr() + min(o[1] for o, (w, h) in zip(p.off, MIXED) if w and h),
                                          p.d_dst.data_ptr() + max(o[1] + (h - 1) * q[1] + w * E for o, q, (w, h) in zip(p.off, p.pitch, MIXED) if w and h))


@pytest.mark.parametrize("name", sorted(TV.SUBLISTS))
def test_sublists_that_change_the_maps_shape(M, oracle, name):
    for E in (2, 4):
        p = Parents(M, TV.SUBLISTS[name], E, seed=10 + sorted(TV.SUBLISTS).index(name))
        info, _ = run_all(M, oracle, p, range(1, 6), ("random",), name)
        if name == "no-edge":
            assert info.edge_tiles == 0 and info.interior_tiles == 5
        if name == "nint-2":
            assert info.interior_tiles == 2
        if name in ("first", "prefix-2", "prefix-3", "prefix-4"):
            assert info.interior_tiles == 0


# ---------------------------------------------------------------------------------------------------- 2. the cone
@pytest.mark.parametrize("E", (2, 4))
@pytest.mark.parametrize("gap", (61, 0))
def test_cone_levels(M, oracle, gap, E):
    """Levels 6, 7, 8 (four fused levels under a cone through the read pitch): the SEEDED = 2 kernels."""
    p = Parents(M, TV.CONE, E, seed=20 + gap, gaps=(gap, gap))
    run_all(M, oracle, p, (6, 7, 8), ("random",), "cone gap %d" % gap)


# ------------------------------------------------------------------------------------------- 3. the padded tensor
@pytest.mark.parametrize("dtype_name", ("float16", "float32"))
def test_padded_tensor_keeps_its_padding(M, oracle, dtype_name):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    dtype = getattr(torch, dtype_name)
    E = 2 if dtype_name == "float16" else 4
    src = Parents(M, MIXED, E, seed=30)
    shapes = [(h, w) for w, h in MIXED]
    batch, views = H.padded_batch(shapes, dtype)
    N, Hmax, Wp = batch.shape
    assert (N, Hmax) == (len(MIXED), 203) and Wp * E % 128 == 0 and 513 <= Wp < 513 + 128 // E and batch.data_ptr() % 128 == 0
    raw = batch.view(torch.uint8)
    raw.fill_(SENTINEL)
    grids = [src.d_src[o[0]:o[0] + h * p[0]].as_strided((h, w), (p[0], 1)) if w and h else src.d_src.new_empty((h, w))
             for (w, h), p, o in zip(MIXED, src.pitch, src.off)]
    plan = H.MappedViewPlan(zip(grids, views), dtype)
    assert plan.fused and plan.info.count == 17, plan.reason
    tab = tables(E)["affine"]
    d_tab = H.affine_table(dtype, device="cuda")
    assert (d_tab.cpu().numpy().view(UINT[E]) == tab).all()
    dec = H.Decoder(Crossed())
    for levels in (3, 7):
        outs = dec.decode_mapped_views(plan, levels, d_tab)
        torch.cuda.synchronize()
        want = np.full((N, Hmax, Wp * E), SENTINEL, np.uint8)
        for i, (w, h) in enumerate(MIXED):
            if w and h:
                want[i, :h, :w * E] = mapped(tab, TV.reference(oracle, TV.content(w, h, 0), (w, h, 0), levels, 1))
        got = raw.cpu().numpy().reshape(want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "padded %s L%d: %d bytes differ, the first at %s" % (dtype_name, levels, len(bad), tuple(bad[0]))
        assert (want == SENTINEL).mean() > 0.5      # the padding was compared
        assert len(outs) == len(MIXED) and outs[0].data_ptr() == batch.data_ptr()
        raw.fill_(SENTINEL)
    assert (src.d_src.cpu().numpy() == src.h_src).all()


# --------------------------------------------------------------------------------------------------- 4. the atlas
def test_atlas_side_by_side(M, oracle):
    import torch
    F, E = M, 4
    rng = np.random.default_rng(SEED0 + 2700)
    SP, DPE = 1024, 1152      # the grid canvas' rows in bytes, the float canvas' in elements
    DP = DPE * E
    order = list(range(len(MIXED)))
    src_at, src_h = TV.shelves(MIXED, SP, order, lambda i: i % 3)
    dst_at, dst_h = TV.shelves(MIXED, DPE, order[::-1], lambda i: (i + 1) % 3)      # x in elements: on lines, mid-line, at odd elements
    # two grids overlap: the 129 x 65 view reads out of the 256 x 128 view's window
    i_small, i_big = MIXED.index((129, 65)), MIXED.index((256, 128))
    src_at[i_small] = (src_at[i_big][0] + 31, src_at[i_big][1] + 17)
    h_src = rng.integers(0, 256, src_h * SP + 8192, dtype=np.uint8)
    d_src = torch.from_numpy(h_src).cuda()
    d_dst = torch.full((dst_h * DP + 8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    lead = 0      # the canvas' first byte in the parent: on a 128-B line, moved until every view keeps the page rule
    while not all(TV.tail_ok(d_src.data_ptr() + lead + y * SP + x, MIXED[i][0], MIXED[i][1], SP) for i, (x, y) in src_at.items()):
        lead += 128
    assert lead < 4096
    pairs = []
    for i, (w, h) in enumerate(MIXED):
        if w and h:
            (sx, sy), (dx, dy) = src_at[i], dst_at[i]
            pairs.append(F.MViewPair(d_src.data_ptr() + lead + sy * SP + sx, d_dst.data_ptr() + 128 + dy * DP + dx * E, w, h, SP, DP))
        else:
            pairs.append(F.MViewPair(0, 0, w, h, 0, 0))
    plan = make_plan(F, (F.MViewPair * len(pairs))(*pairs), len(pairs), E)
    tab = tables(E)["random"]
    d_tab = device_table(tab)
    for levels in (3, 7):
        assert launch(F, plan, levels, 1, d_tab) == OK, F.last_error()
        torch.cuda.synchronize()
        want = np.full(d_dst.shape[0], SENTINEL, np.uint8)
        for i, (w, h) in enumerate(MIXED):
            if w and h:
                (sx, sy), (dx, dy) = src_at[i], dst_at[i]
                src = TV.Parents.window(h_src, lead + sy * SP + sx, w, h, SP)
                byte_window(want, 128 + dy * DP + dx * E, w, h, DP, E)[...] = mapped(tab, TV.reference(oracle, src, ("mviews atlas", i), levels, 1))
        got = d_dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "atlas L%d: %d bytes of the canvas differ, the first at %d" % (levels, bad.size, int(bad[0]))
        assert (want == SENTINEL).sum() > dst_h * DP // 4      # the sentinel between and around the windows was compared
        assert (d_src.cpu().numpy() == h_src).all()
        d_dst.fill_(SENTINEL)


# ------------------------------------------------------------------------------------- 5. plan reuse and capture
def test_plan_reuse_and_graph_capture(M, oracle):
    import torch
    E = 2
    p = Parents(M, MIXED, E, seed=3)
    plan = p.plan()
    tabs = [tables(E)["random"], tables(E)["affine"]]
    d_tabs = [device_table(t) for t in tabs]
    for variant in (0, 1):
        p.fill(variant)
        assert launch(M, plan, 4, 1, d_tabs[variant]) == OK, M.last_error()
        p.check(oracle, 4, 1, tabs[variant], "launch %d of one plan" % variant)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = launch(M, plan, 4, 1, d_tabs[0], stream=side.cuda_stream)
    assert st == OK, M.last_error()
    torch.cuda.synchronize()
    assert (p.d_dst.cpu().numpy() == SENTINEL).all(), "capturing must not run the launch"
    p.fill(2)
    g.replay()
    p.check(oracle, 4, 1, tabs[0], "replayed on new contents")


# --------------------------------------------------------------------------------------------- 6. the Python surface
def test_python_surface_fused_and_composed(M, oracle):
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    shapes = [(65, 129), (64, 128), (1, 200), (0, 3), (203, 301)]      # (height, width)
    total, places = H.aligned_arena(shapes)
    rng = np.random.default_rng(SEED0 + 2800)
    h_grid = rng.integers(0, 256, total, dtype=np.uint8)
    grid = torch.from_numpy(h_grid).cuda()
    dec = H.Decoder(Crossed())
    for dtype, E in ((torch.bfloat16, 2), (torch.float32, 4)):
        # the float arena: aligned_arena's layout of rows of w * E bytes
        ftotal, fplaces = H.aligned_arena([(h, w * E) for h, w in shapes])
        arena = torch.full((ftotal,), SENTINEL, dtype=torch.uint8, device="cuda")
        outs = [arena[o:o + h * p].view(h, p).view(dtype)[:, :w] if h and w else torch.empty((h, w), dtype=dtype, device="cuda") for (h, w), (o, p) in zip(shapes, fplaces)]
        plan = H.MappedViewPlan(zip(H.views.arena_views(grid, shapes, places), outs), dtype)
        assert plan.fused and plan.info.count == 4 and plan.elem_size == E
        tab = H.affine_table(dtype, scale=2.0 / 255.0, bias=-1.0, device="cuda")
        bits = tab.view(torch.int16 if E == 2 else torch.int32).cpu().numpy().view(UINT[E])
        got = dec.decode_mapped_views(plan, 4, tab)
        torch.cuda.synchronize()
        want = np.full(ftotal, SENTINEL, np.uint8)
        for (h, w), (o, pitch), (fo, fp) in zip(shapes, places, fplaces):
            if h and w:
                d = oracle.decode(np.ascontiguousarray(TV.Parents.window(h_grid, o, w, h, pitch)), 4, 1)
                byte_window(want, fo, w, h, fp, E)[...] = mapped(bits, d)
        assert (arena.cpu().numpy() == want).all() and (grid.cpu().numpy() == h_grid).all()
        assert len(got) == 5 and got[0].data_ptr() == arena.data_ptr() and got[0].dtype == dtype
        with pytest.raises(ValueError, match="table"):
            dec.decode_mapped_views(plan, 4, H.affine_table(torch.float16 if E == 4 else torch.float32, device="cuda"))
        # more levels than the one launch serves: composed, the same bits
        small = H.MappedViewPlan([(H.views.arena_views(grid, shapes, places)[1], outs[1])], dtype)
        arena.fill_(SENTINEL)
        dec.decode_mapped_views(small, 9, tab)
        torch.cuda.synchronize()
        d = oracle.decode(np.ascontiguousarray(TV.Parents.window(h_grid, places[1][0], 128, 64, places[1][1])), 9, 1)
        assert (outs[1].contiguous().view(torch.uint8).cpu().numpy().reshape(64, -1) == mapped(bits, d)).all()
    # one entry whose last grid byte is the last byte of a page, width % 4 != 0: the plan is not fused, the calls are composed
    w, h, pitch = 130, 66, 147
    span = (h - 1) * pitch + w
    parent = torch.from_numpy(rng.integers(0, 256, span + 3 * 4096, dtype=np.uint8)).cuda()
    lead = (-(parent.data_ptr() + span)) % 4096
    assert not TV.tail_ok(parent.data_ptr() + lead, w, h, pitch)
    bad_src = parent[lead:lead + h * pitch - (pitch - w)].as_strided((h, w), (pitch, 1))
    good_src = H.views.arena_views(grid, shapes, places)[0]
    outs = [torch.full((h, (w + 5) * 2), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((65, (129 + 3) * 2), SENTINEL, dtype=torch.uint8, device="cuda")]
    plan = H.MappedViewPlan([(bad_src, outs[0].view(torch.float16)[:, :w]), (good_src, outs[1].view(torch.float16)[:, :129])], torch.float16)
    assert not plan.fused and "tail" in plan.reason and "view 0" in plan.reason
    tab = H.affine_table(torch.float16, device="cuda")
    bits = tab.view(torch.int16).cpu().numpy().view(np.uint16)
    dec.decode_mapped_views(plan, 4, tab)
    torch.cuda.synchronize()
    for src, out, ww in ((bad_src, outs[0], w), (good_src, outs[1], 129)):
        got = out.cpu().numpy()
        assert (got[:, :2 * ww] == mapped(bits, oracle.decode(np.ascontiguousarray(src.cpu().numpy()), 4, 1))).all() and (got[:, 2 * ww:] == SENTINEL).all()


# ------------------------------------------------------------------------------- 7. one call per instantiation
INSTANCES = [(i, s, e) for i in (1, 0) for s in (0, 2) for e in (2, 4)]


@functools.lru_cache(maxsize=None)
def _small(M, E):
    return Parents(M, [(129, 65), (128, 64), (70, 1)], E, seed=60)


@pytest.mark.parametrize("interp,seeded,E", INSTANCES, ids=["i%d-s%d-e%d" % t for t in INSTANCES])
def test_one_call_per_instantiation(M, oracle, interp, seeded, E):
    """k_dec_mviews<INTERP, SEEDED, E>, eight kernels, one launch each against the oracle."""
    assert len(INSTANCES) == 8
    p = _small(M, E)
    levels = 6 if seeded else 3
    tab = tables(E)["random"]
    assert launch(M, p.plan(), levels, interp, device_table(tab)) == OK, M.last_error()
    p.check(oracle, levels, interp, tab, "interp %d seeded %d E %d" % (interp, seeded, E))


# ------------------------------------------------------------------------------------------- 8. table aliasing
@pytest.mark.parametrize("E", (2, 4))
def test_a_table_inside_the_output_interval_is_refused(M, oracle, E):
    """The table lies in the 2 KiB between two outputs of one parent: inside [dst_lo, dst_hi), refused, nothing written; the same
    table just behind the interval is served."""
    import torch
    F = M
    w, h = 70, 9
    rng = np.random.default_rng(SEED0 + 2900 + E)
    h_src = rng.integers(0, 256, 2 * h * w + 64, dtype=np.uint8)
    d_src = torch.from_numpy(h_src).cuda()
    tab = tables(E)["random"]
    frame = h * w * E
    size = 2 * frame + 2048 + 256 * E + 64
    h_dst = np.full(size, SENTINEL, np.uint8)
    hole, behind = frame + 1024 - 128 * E, 2 * frame + 2048
    h_dst[hole:hole + 256 * E] = tab.view(np.uint8)
    h_dst[behind:behind + 256 * E] = tab.view(np.uint8)
    d_dst = torch.from_numpy(h_dst).cuda()
    base = d_dst.data_ptr()
    arr = (F.MViewPair * 2)(F.MViewPair(d_src.data_ptr(), base, w, h, w, w * E), F.MViewPair(d_src.data_ptr() + h * w + 4, base + frame + 2048, w, h, w, w * E))
    plan = make_plan(F, arr, 2, E)
    assert (plan[0].dst_lo, plan[0].dst_hi) == (base, base + 2 * frame + 2048)
    L = F.lib()
    for off in (hole, frame - 256 * E + E, 2 * frame + 2048 - E):      # in the hole; its last / first element on an output element
        assert L.hgi_mviews_decode_dev(None, plan[1].data_ptr(), ctypes.addressof(plan[0]), 3, 1, base + off) == EINVAL
        assert "table" in F.last_error() and "alias" in F.last_error()
    torch.cuda.synchronize()
    assert (d_dst.cpu().numpy() == h_dst).all(), "a refused launch wrote something"
    assert L.hgi_mviews_decode_dev(None, plan[1].data_ptr(), ctypes.addressof(plan[0]), 3, 1, base + behind) == OK, F.last_error()
    torch.cuda.synchronize()
    want = h_dst.copy()
    for i, off in enumerate((0, frame + 2048)):
        src = h_src[i * (h * w + 4):][:h * w].reshape(h, w)
        want[off:off + frame] = mapped(tab, oracle.decode(np.ascontiguousarray(src), 3, 1)).reshape(-1)
    assert (d_dst.cpu().numpy() == want).all() and (d_src.cpu().numpy() == h_src).all()
