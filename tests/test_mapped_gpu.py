"""GPU suite of mapped decode (hgi_map_decode_dev, Decoder.decode_mapped): for every shape, depth, pitch, alignment and element
size the output, read through its pitch, must be `table[oracle.decode(grid)]` bit for bit; no byte outside the element rows may
be written and the grid must come back unmodified.  Every case reads its grid out of a parent buffer of RANDOM bytes (any byte
plane is a valid grid) and writes into a SENTINEL-filled parent that is checked whole.  The tables are random and injective, so
a wrong lookup cannot pass by coincidence; outputs are compared as unsigned integers of the element size (tables hold NaN
patterns).  Expected values: the oracle.  Never the library under test."""
import numpy as np
import pytest

from conftest import SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3
GAPS = (1, 3, 16, 61, 128)
OK, EINVAL, EUNSUPPORTED = 0, 1, 4
UINT = {2: np.uint16, 4: np.uint32}


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from rustyhgi_amd import _ffi_map
    assert _ffi_map.lib() is not None
    return _ffi_map


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %#x want %#x" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def injective_table(rng, E):
    """256 distinct 16- or 32-bit patterns in random order."""
    if E == 2:
        return rng.permutation(1 << 16)[:256].astype(np.uint16)
    t = (rng.permutation(1 << 20)[:256].astype(np.uint32) << np.uint32(12)) | rng.integers(0, 4096, 256, dtype=np.uint32)
    assert len(np.unique(t)) == 256
    return t


def rows_index(B, h, n, lead, pitch, fstride):
    """byte indices of B x h rows of n bytes"""
    return lead + (np.arange(B)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch + np.arange(n)[None, None, :])


def tail_rule(ptr, B, h, w, pitch, fstride):
    """include/hgi_map.h: width % 4 != 0 is served iff the three bytes behind the last grid frame's span lie in the 4-KiB page
    of its last byte."""
    end = ptr + (B - 1) * (fstride if B > 1 else 0) + (h - 1) * pitch + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


class Placed:
    """(B, h, w) grids placed for one call: the grids in a parent of random bytes, the output (E-byte elements) in a sentinel
    parent.  `gaps`: (grid gap in bytes, output gap in ELEMENTS); `leads`: bytes, the output's a multiple of E; `extras`: bytes
    between a frame's span and the next frame, the output's a multiple of E."""

    def __init__(self, grids, E, gaps, leads=(0, 0), extras=(0, 0), seed=1, violate_tail=False):
        import torch
        self.grids, self.E = grids, E
        self.B, self.h, self.w = B, h, w = grids.shape
        assert leads[1] % E == 0 and extras[1] % E == 0
        self.pitch = [w + gaps[0], (w + gaps[1]) * E]
        self.row = [w, w * E]
        self.span = [(h - 1) * p + r for p, r in zip(self.pitch, self.row)]
        self.fs = [s + e for s, e in zip(self.span, extras)]
        self.total = [l + (B - 1) * f + s + 4096 + 64 for l, f, s in zip(leads, self.fs, self.span)]
        self.d_grid = torch.empty((self.total[0],), dtype=torch.uint8, device="cuda")
        self.lead = list(leads)
        p0 = self.d_grid.data_ptr()
        if violate_tail:      # the last frame's last byte on the last byte of a page
            end = p0 + self.lead[0] + (B - 1) * self.fs[0] + self.span[0]
            self.lead[0] += (-end) % 4096
            assert w % 4 and not tail_rule(p0 + self.lead[0], B, h, w, self.pitch[0], self.fs[0])
        elif not tail_rule(p0 + self.lead[0], B, h, w, self.pitch[0], self.fs[0]):
            self.lead[0] += 4      # out of the 3-byte window: the call runs fused
            assert tail_rule(p0 + self.lead[0], B, h, w, self.pitch[0], self.fs[0])
        rng = np.random.default_rng(seed)
        self.src = rng.integers(0, 256, self.total[0], dtype=np.uint8)
        self.src[rows_index(B, h, w, self.lead[0], self.pitch[0], self.fs[0])] = grids
        self.d_grid.copy_(torch.from_numpy(self.src))
        self.d_out = torch.full((self.total[1],), SENT, dtype=torch.uint8, device="cuda")
        assert self.d_out.data_ptr() % 4 == 0

    def call(self, M, levels, interp, d_table, stream=0, elem=None, out_pitch=None, grid_back=0):
        return M.lib().hgi_map_decode_dev(stream or None, self.d_grid.data_ptr() + self.lead[0] - grid_back, self.pitch[0], self.w, self.h,
                                          levels, interp, d_table.data_ptr(), elem or self.E, self.d_out.data_ptr() + self.lead[1],
                                          out_pitch or self.pitch[1], self.B, self.fs[0], self.fs[1])

    def output(self, what):
        """The output read through its pitch as (B, h, w) unsigned integers (after a sync); every other byte of its parent must
        hold the sentinel and the grid parent its bytes."""
        host = self.d_out.cpu().numpy()
        idx = rows_index(self.B, self.h, self.w * self.E, self.lead[1], self.pitch[1], self.fs[1])
        mask = np.zeros(self.total[1], bool)
        mask[idx] = True
        stray = np.nonzero(host[~mask] != SENT)[0]
        assert len(stray) == 0, "%s: %d bytes outside the element rows written" % (what, len(stray))
        assert (self.d_grid.cpu().numpy() == self.src).all(), what + ": the grid parent was modified"
        return np.ascontiguousarray(host[idx]).view(UINT[self.E])

    def untouched(self):
        return bool((self.d_out == SENT).all())


def device_table(table):
    """The table's bits on the device (int16 / int32 carry them; the library never interprets them)."""
    import torch
    return torch.from_numpy(table.view({2: np.int16, 4: np.int32}[table.dtype.itemsize])).cuda()


def check(M, grids, dec, levels, interp, E, gaps, what, seed=1, **kw):
    """One call on `grids` (B, h, w); `dec`: the oracle's decodes of them."""
    import torch
    table = injective_table(np.random.default_rng(seed + 1000 * E), E)
    p = Placed(grids, E, gaps, seed=seed, **kw)
    st = p.call(M, levels, interp, device_table(table))
    assert st == OK, "%s: status %d: %s" % (what, st, M.last_error())
    torch.cuda.synchronize()
    assert_same(p.output(what), table[dec], what)


def test_small_golden_cases(M, golden, small):
    """The tiny / odd shapes of tests/golden/small_cases.npz at levels 1 ... 8, both interpolators as stored: the stored grid in,
    table[stored decode] out.  E alternates 2 / 4."""
    n = 0
    for key in golden:
        if ("grid/" + key) not in small:
            continue
        name, lv, q, i = key.split("/")
        levels, interp = int(lv[1:]), int(i[1:])
        if not 1 <= levels <= 8:
            continue
        E = 2 + 2 * (n & 1)
        check(M, small["grid/" + key][None], small["dec/" + key][None], levels, interp, E, (GAPS[n % 5], GAPS[(n // 5 + 2) % 5]),
              "%s E%d" % (key, E), leads=(n % 31, E * ((5 * n + 3) % 8)), seed=n)
        n += 1
    assert n == 90


RAGGED = [(w, h) for w in (128, 130, 255, 384) for h in (64, 70, 127, 192)]


@pytest.mark.parametrize("w,h", RAGGED)
def test_interior_and_ragged_tiles_levels_1_to_5(M, oracle, w, h):
    """Interior tiles plus every ragged kind (right, bottom, both; odd heights; widths 2 and 3 mod 4: every `nvalid` class of the
    straddling chunk and the E = 2 odd-count b16 store), levels 1 ... 5, batch 3 with frame strides beyond the span, both E,
    noise grids, interpolators alternating."""
    rng = np.random.default_rng(SEED0 + 11 * w + h)
    for levels in range(1, 6):
        interp = (levels + w) & 1
        grids = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        dec = np.stack([oracle.decode(g, levels, interp) for g in grids])
        for E in (2, 4):
            check(M, grids, dec, levels, interp, E, (GAPS[levels % 5], GAPS[(levels + 2 + E) % 5]), "%dx%d L%d E%d" % (w, h, levels, E),
                  leads=(levels + 13 * (E // 4), E * (7 - levels)), extras=(77 + levels, 4 * (250 + levels)), seed=levels)


@pytest.mark.parametrize("w,h", [(300, 200), (520, 264)])
def test_cone_depths(M, oracle, w, h):
    """Levels 6, 7, 8: four fused levels under the cone, which reads the frame's own lattice through the grid pitch.  Batch 2."""
    rng = np.random.default_rng(SEED0 + w)
    for levels in (6, 7, 8):
        grids = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        dec = np.stack([oracle.decode(g, levels, levels & 1) for g in grids])
        for E in (2, 4):
            check(M, grids, dec, levels, levels & 1, E, (GAPS[levels % 5], GAPS[(levels + E) % 5]), "%dx%d L%d E%d" % (w, h, levels, E),
                  leads=(levels + 9, 2 * E), extras=(levels, 4096), seed=levels)


def test_real_frame_with_the_practical_tables(M, oracle, fullhd):
    """1920 x 1080, four levels, Medium, batch 2, packed.  The float16 x / 255 table of affine_table gives the float16 frame a
    conversion would, bit for bit; a float32 table with signed zeros, infinities, a quiet and a signalling NaN keeps their bits."""
    import torch
    from rustyhgi_amd import affine_table
    lut, _ = oracle.linear_lut(oracle.MEDIUM)
    grid = oracle.encode(fullhd, 4, lut, 1)
    dec = oracle.decode(grid, 4, 1)
    grids = np.stack([grid, grid])
    t16 = affine_table(np.float16)
    assert t16.dtype == np.float16 and t16.shape == (256,)
    p = Placed(grids, 2, (0, 0))
    assert p.call(M, 4, 1, device_table(t16)) == OK, M.last_error()
    torch.cuda.synchronize()
    got = p.output("fullhd float16")
    want = (dec.astype(np.float32) * np.float32(1 / 255)).astype(np.float16)
    for f in range(2):
        assert_same(got[f], want.view(np.uint16), "fullhd float16 frame %d" % f)
    t32 = np.random.default_rng(7).standard_normal(256).astype(np.float32).view(np.uint32)
    # the special patterns sit at pixel values the frame really has, so each of them is looked up
    present = np.unique(dec)
    assert len(present) >= 7
    chosen = present[np.linspace(0, len(present) - 1, 7).astype(int)]
    special = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345)      # +-0, +-inf, quiet / signalling NaN
    for i, bits in zip(chosen, special):
        t32[i] = bits
    p = Placed(grids, 4, (0, 0))
    assert p.call(M, 4, 1, device_table(t32)) == OK, M.last_error()
    torch.cuda.synchronize()
    got = p.output("fullhd float32")
    for f in range(2):
        assert_same(got[f], t32[dec], "fullhd float32 frame %d" % f)


def test_table_is_read_in_stream_order(M, oracle):
    """On a side stream: a call with table A, the table overwritten with B on that stream, a call into a second output.  One
    sync.  The first output is A[dec], the second B[dec]."""
    import torch
    rng = np.random.default_rng(SEED0 + 5)
    w, h, B, levels = 384, 127, 2, 3
    grids = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
    dec = np.stack([oracle.decode(g, levels, 1) for g in grids])
    ta, tb = injective_table(rng, 4), injective_table(rng, 4)
    first = Placed(grids, 4, (16, 3), leads=(5, 8), extras=(1, 4))
    second = Placed(grids, 4, (0, 61), leads=(0, 4), extras=(0, 8))
    d_tab, d_b = device_table(ta), device_table(tb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = torch.cuda.current_stream().cuda_stream
        assert s == side.cuda_stream
        assert first.call(M, levels, 1, d_tab, stream=s) == OK, M.last_error()
        d_tab.copy_(d_b, non_blocking=True)
        assert second.call(M, levels, 1, d_tab, stream=s) == OK, M.last_error()
    torch.cuda.synchronize()
    assert_same(first.output("table A"), ta[dec], "table A")
    assert_same(second.output("table B"), tb[dec], "table B")


def test_refusals_write_nothing(M):
    """On a live device: the violated tail rule, elem_size 3 and an odd output pitch at E = 2 return their status and leave the
    sentinel parent untouched; the tail case is served four bytes earlier."""
    import torch
    rng = np.random.default_rng(5)
    grids = rng.integers(0, 256, (2, 70, 130), dtype=np.uint8)
    tab = device_table(injective_table(rng, 2))
    p = Placed(grids, 2, (3, 16), leads=(7, 6), extras=(9, 10), violate_tail=True)
    st = p.call(M, 4, 1, tab)
    assert st == EUNSUPPORTED and "tail" in M.last_error(), (st, M.last_error())
    st = p.call(M, 4, 1, tab, elem=3)
    assert st == EINVAL and "elem_size" in M.last_error(), (st, M.last_error())
    q = Placed(grids, 2, (3, 16), leads=(3, 6), extras=(9, 10))
    st = q.call(M, 4, 1, tab, out_pitch=q.pitch[1] + 1)
    assert st == EINVAL and "pitch" in M.last_error(), (st, M.last_error())
    torch.cuda.synchronize()
    assert p.untouched() and q.untouched()
    # the same placement four bytes earlier is served (the parent's bytes there are as good a grid as any)
    assert p.lead[0] >= 4 and tail_rule(p.d_grid.data_ptr() + p.lead[0] - 4, 2, 70, 130, p.pitch[0], p.fs[0])
    assert p.call(M, 4, 1, tab, grid_back=4) == OK, M.last_error()
    torch.cuda.synchronize()
    assert not p.untouched()


def test_python_mirror_fused_and_composed_routes(M, oracle):
    """Decoder.decode_mapped on CUDA views with `out=` views and on numpy arrays, against table[oracle.decode]: levels 4 and 7
    take the fused launch (shown by calling the library on the same arguments), levels 0 and 9 the composed route."""
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + 9)
    parent = torch.randint(0, 256, (3, 400, 700), dtype=torch.uint8, device="cuda", generator=gen)
    host = parent.cpu().numpy()
    rng = np.random.default_rng(SEED0 + 10)
    for n, (x0, y0, w, h, levels, interp) in enumerate(((0, 0, 700, 400, 4, 1), (33, 7, 520, 300, 9, 1), (100, 50, 16, 16, 0, 0),
                                                        (5, 3, 258, 131, 7, 0), (64, 64, 384, 128, 4, 1))):
        E = 2 + 2 * (n & 1)
        tdt = (torch.bfloat16, torch.float32)[n & 1]
        bits = (torch.int16, torch.int32)[n & 1]
        table = injective_table(rng, E)
        d_table = device_table(table).view(tdt)
        dec = H.Decoder(Crossed() if interp else LeftTop())
        view = parent[:, y0:y0 + h, x0:x0 + w]
        crop = host[:, y0:y0 + h, x0:x0 + w]
        want = table[np.stack([oracle.decode(np.ascontiguousarray(g), levels, interp) for g in crop])]
        what = "view %r L%d E%d" % ((x0, y0, w, h), levels, E)
        r = dec.decode_mapped(view, levels, d_table)
        torch.cuda.synchronize()
        assert r.is_contiguous() and r.dtype == tdt and tuple(r.shape) == (3, h, w)
        assert_same(r.view(bits).cpu().numpy().view(UINT[E]), want, what)
        canvas = torch.full((3, 405, 720 * E), SENT, dtype=torch.uint8, device="cuda").view(tdt)      # (3, 405, 720) elements
        ox = 9
        window = canvas[:, 1:1 + h, ox:ox + w]
        r2 = dec.decode_mapped(view, levels, d_table, out=window)
        torch.cuda.synchronize()
        assert r2.data_ptr() == window.data_ptr()
        hc = canvas.view(bits).cpu().numpy().view(UINT[E]).copy()
        assert_same(hc[:, 1:1 + h, ox:ox + w], want, "canvas " + what)
        hc[:, 1:1 + h, ox:ox + w] = np.array([SENT] * E, np.uint8).view(UINT[E])[0]
        assert (hc.view(np.uint8) == SENT).all(), "written outside the window: " + what
        if levels in (4, 7):      # the fused route ran: the library serves these very arguments
            st = M.lib().hgi_map_decode_dev(torch.cuda.current_stream().cuda_stream or None, view.data_ptr(), view.stride(1), w, h, levels,
                                            interp, d_table.data_ptr(), E, window.data_ptr(), window.stride(1) * E, 3, view.stride(0),
                                            window.stride(0) * E)
            assert st == OK, M.last_error()
        else:
            st = M.lib().hgi_map_decode_dev(None, view.data_ptr(), view.stride(1), w, h, levels, interp, d_table.data_ptr(), E,
                                            window.data_ptr(), window.stride(1) * E, 3, view.stride(0), window.stride(0) * E)
            assert st == EUNSUPPORTED
        torch.cuda.synchronize()
        # numpy: a 2-D crop of frame 1 and a numpy table of a numpy dtype, uploaded and downloaded
        ntab = table.view({2: np.float16, 4: np.float32}[E])
        nr = dec.decode_mapped(crop[1], levels, ntab)
        assert nr.dtype == ntab.dtype and nr.shape == (h, w)
        assert_same(nr.view(UINT[E]), want[1], "numpy " + what)
        assert (parent.cpu().numpy() == host).all(), "the parent was modified"
