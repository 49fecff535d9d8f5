"""GPU suite of encode with reconstruction (hgi_recon_encode_u8_dev, Encoder.encode_with_reconstruction): for every shape,
depth, pitch and alignment the grid, read through its pitch, must be the oracle's encode of the packed frame and the
reconstruction the oracle's decode of that grid, bit for bit; no byte outside the rows of either output may be written and the
input must come back unmodified.  Every case reads its input out of a parent buffer of RANDOM bytes and writes both outputs
into SENTINEL-filled parents that are checked whole.  Expected bytes: the oracle.  Never the library under test."""
import numpy as np
import pytest

from conftest import SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3
GAPS = (1, 3, 16, 61, 128)
OK, EINVAL, EUNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def R():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from rustyhgi_amd import _ffi_recon
    assert _ffi_recon.lib() is not None
    return _ffi_recon


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def rows_index(B, h, w, lead, pitch, fstride):
    return lead + (np.arange(B)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch + np.arange(w)[None, None, :])


def tail_rule(ptr, B, h, w, pitch, fstride):
    """include/hgi_recon.h: width % 4 != 0 is served iff the three bytes behind the last input frame's span lie in the 4-KiB
    page of its last byte."""
    end = ptr + (B - 1) * (fstride if B > 1 else 0) + (h - 1) * pitch + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


class Placed:
    """(B, h, w) frames placed for one call: the input in a parent of random bytes, both outputs in sentinel parents."""

    def __init__(self, frames, pitches, leads=(0, 0, 0), extras=(0, 0, 0), seed=1, violate_tail=False):
        import torch
        self.frames = frames
        self.B, self.h, self.w = B, h, w = frames.shape
        self.pitch = pitches
        self.span = [(h - 1) * p + w for p in pitches]
        self.fs = [s + e for s, e in zip(self.span, extras)]
        self.total = [l + (B - 1) * f + s + 4096 + 64 for l, f, s in zip(leads, self.fs, self.span)]
        self.d_src = torch.empty((self.total[0],), dtype=torch.uint8, device="cuda")
        self.lead = list(leads)
        p0 = self.d_src.data_ptr()
        if violate_tail:      # the last frame's last byte on the last byte of a page
            end = p0 + self.lead[0] + (B - 1) * self.fs[0] + self.span[0]
            self.lead[0] += (-end) % 4096
            assert w % 4 and not tail_rule(p0 + self.lead[0], B, h, w, pitches[0], self.fs[0])
        elif not tail_rule(p0 + self.lead[0], B, h, w, pitches[0], self.fs[0]):
            self.lead[0] += 4      # out of the 3-byte window: the call runs fused
            assert tail_rule(p0 + self.lead[0], B, h, w, pitches[0], self.fs[0])
        rng = np.random.default_rng(seed)
        self.src = rng.integers(0, 256, self.total[0], dtype=np.uint8)
        self.src[rows_index(B, h, w, self.lead[0], pitches[0], self.fs[0])] = frames
        self.d_src.copy_(torch.from_numpy(self.src))
        self.d_grid = torch.full((self.total[1],), SENT, dtype=torch.uint8, device="cuda")
        self.d_rec = torch.full((self.total[2],), SENT, dtype=torch.uint8, device="cuda")

    def call(self, R, levels, interp, lut, stream=0, src_ptr=None, pitch0=None, fs0=None):
        lut = np.ascontiguousarray(lut, np.uint8)
        return R.lib().hgi_recon_encode_u8_dev(
            stream or None, src_ptr or self.d_src.data_ptr() + self.lead[0], pitch0 or self.pitch[0], self.w, self.h, levels, interp,
            lut.ctypes.data, self.d_grid.data_ptr() + self.lead[1], self.pitch[1], self.d_rec.data_ptr() + self.lead[2], self.pitch[2],
            self.B, fs0 or self.fs[0], self.fs[1], self.fs[2])

    def outputs(self, what):
        """(grid, recon) read through their pitches (after a sync); every other byte of both parents must hold the sentinel and
        the input parent its bytes."""
        got = []
        for side, d in ((1, self.d_grid), (2, self.d_rec)):
            host = d.cpu().numpy()
            idx = rows_index(self.B, self.h, self.w, self.lead[side], self.pitch[side], self.fs[side])
            mask = np.zeros(self.total[side], bool)
            mask[idx] = True
            stray = np.nonzero(host[~mask] != SENT)[0]
            assert len(stray) == 0, "%s: %d bytes outside the %s rows written" % (what, len(stray), ("grid", "reconstruction")[side - 1])
            got.append(host[idx])
        assert (self.d_src.cpu().numpy() == self.src).all(), what + ": the input parent was modified"
        return got

    def untouched(self):
        return bool((self.d_grid == SENT).all()) and bool((self.d_rec == SENT).all())


def run(R, frames, levels, interp, lut, pitches, what, **kw):
    import torch
    p = Placed(frames, pitches, **kw)
    st = p.call(R, levels, interp, lut)
    assert st == OK, "%s: status %d: %s" % (what, st, R.last_error())
    torch.cuda.synchronize()
    return p.outputs(what)


def check(R, oracle, frames, levels, interp, lut, pitches, what, **kw):
    grids = np.stack([oracle.encode(im, levels, lut, interp) for im in frames])
    want = np.stack([oracle.decode(g, levels, interp) for g in grids])
    g, r = run(R, frames, levels, interp, lut, pitches, what, **kw)
    assert_same(g, grids, "grid " + what)
    assert_same(r, want, "reconstruction " + what)


def lut_for(oracle, q):
    return oracle.noop_lut() if q == "noop" else oracle.linear_lut(int(q))[0]


def test_small_golden_cases_through_three_pitches(R, oracle, golden, small):
    """The tiny / odd shapes of tests/golden/small_cases.npz at levels 1 ... 8 x their quantizers x both interpolators, against the
    stored grids and decodes (the oracle's); three different gaps from {1, 3, 16, 61, 128} on the three sides, leads 0 ... 15."""
    n = 0
    for key in golden:
        if ("grid/" + key) not in small:
            continue
        name, lv, q, i = key.split("/")
        levels, interp = int(lv[1:]), int(i[1:])
        if not 1 <= levels <= 8:
            continue
        img = small["in/" + name]
        h, w = img.shape
        a = n % 5
        pitches = (w + GAPS[a], w + GAPS[(a + 1 + (n // 5) % 2) % 5], w + GAPS[(a + 3 + (n // 10) % 2) % 5])
        assert len(set(pitches)) == 3
        g, r = run(R, img[None], levels, interp, lut_for(oracle, q[1:]), pitches, key, leads=(n % 16, (5 * n + 3) % 16, (7 * n + 11) % 16), seed=n)
        assert_same(g[0], small["grid/" + key], "grid " + key)
        assert_same(r[0], small["dec/" + key], "reconstruction " + key)
        n += 1
    assert n == 90


RAGGED = [(w, h) for w in (128, 130, 255, 384) for h in (64, 70, 127, 192)]


@pytest.mark.parametrize("w,h", RAGGED)
def test_interior_and_ragged_tiles_levels_1_to_5(R, oracle, w, h):
    """Interior tiles plus every ragged kind (right, bottom, both; odd heights; widths 2 and 3 mod 4), levels 1 ... 5, batch 3 with
    frame strides beyond the span, random 256-byte tables on noise (the overflow fallback fires constantly), interpolators
    alternating."""
    rng = np.random.default_rng(SEED0 + 11 * w + h)
    for levels in range(1, 6):
        interp = (levels + w) & 1
        imgs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        lut = rng.integers(0, 256, 256, dtype=np.uint8)
        pitches = (w + GAPS[levels % 5], w + GAPS[(levels + 2) % 5], w + GAPS[(levels + 4) % 5])
        check(R, oracle, imgs, levels, interp, lut, pitches, "%dx%d L%d" % (w, h, levels), leads=(levels, 16 - levels, 2 * levels),
              extras=(77 + levels, 1000, 333), seed=levels)


@pytest.mark.parametrize("w,h", [(300, 200), (520, 264)])
def test_cone_depths(R, oracle, w, h):
    """Levels 6, 7, 8: four fused levels under the cone, which reads the frame's own lattice through the image pitch.  Batch 2."""
    rng = np.random.default_rng(SEED0 + w)
    for levels in (6, 7, 8):
        imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        lut = oracle.linear_lut(3)[0] if levels % 2 else rng.integers(0, 256, 256, dtype=np.uint8)
        pitches = (w + GAPS[levels % 5], w + GAPS[(levels + 3) % 5], w + GAPS[(levels + 1) % 5])
        check(R, oracle, imgs, levels, levels & 1, lut, pitches, "%dx%d L%d" % (w, h, levels), leads=(levels % 16, 3, 9),
              extras=(levels, 4096, 17), seed=levels)


@pytest.mark.parametrize("w,h", [(255, 70), (384, 128)])
def test_identity_table_writes_the_image_as_reconstruction(R, oracle, w, h):
    rng = np.random.default_rng(SEED0 + w + h)
    imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    lut = np.arange(256, dtype=np.uint8)
    for interp in (0, 1):
        g, r = run(R, imgs, 4, interp, lut, (w + 3, w + 16, w + 61), "identity %dx%d i%d" % (w, h, interp), leads=(1, 2, 3), extras=(5, 6, 7))
        assert_same(g, np.stack([oracle.encode(im, 4, oracle.noop_lut(), interp) for im in imgs]), "identity grid %dx%d i%d" % (w, h, interp))
        assert_same(r, imgs, "identity reconstruction %dx%d i%d" % (w, h, interp))


def test_real_image_packed(R, oracle, fullhd):
    """The packed case: 1920 x 1080, four levels, Medium, batch 2 of one frame twice, all three pitches equal to the width."""
    lut, err = oracle.linear_lut(oracle.MEDIUM)
    imgs = np.stack([fullhd, fullhd])
    w = fullhd.shape[1]
    g, r = run(R, imgs, 4, 1, lut, (w, w, w), "fullhd packed")
    want = oracle.encode(fullhd, 4, lut, 1)
    back = oracle.decode(want, 4, 1)
    for f in range(2):
        assert_same(g[f], want, "fullhd grid %d" % f)
        assert_same(r[f], back, "fullhd reconstruction %d" % f)
    assert int(np.abs(r[0].astype(int) - fullhd.astype(int)).max()) <= err


def test_violated_tail_rule_is_refused_and_writes_nothing(R):
    import torch
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (2, 70, 130), dtype=np.uint8)
    p = Placed(imgs, (133, 146, 191), leads=(3, 5, 7), extras=(9, 11, 13), violate_tail=True)
    st = p.call(R, 4, 1, np.arange(256, dtype=np.uint8) // 2)
    assert st == EUNSUPPORTED and "tail" in R.last_error(), (st, R.last_error())
    torch.cuda.synchronize()
    assert p.untouched()
    # the same placement four bytes earlier is served
    assert tail_rule(p.d_src.data_ptr() + p.lead[0] - 4, 2, 70, 130, 133, p.fs[0])


def test_side_stream_and_chained_call(R, oracle):
    """The call on a non-default torch stream, a second call queued behind it that takes the first one's reconstruction as its
    image, then ONE sync: both results are the oracle's."""
    import torch
    rng = np.random.default_rng(SEED0 + 3)
    w, h, B, levels = 384, 127, 2, 3
    imgs = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
    lut = oracle.linear_lut(oracle.MEDIUM)[0]
    first = Placed(imgs, (w + 16, w + 3, w + 128), leads=(0, 4, 8), extras=(1, 2, 3))
    second = Placed(np.zeros_like(imgs), (w, w + 61, w + 1), leads=(0, 1, 2), extras=(0, 5, 6))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = torch.cuda.current_stream().cuda_stream
        assert s == side.cuda_stream
        assert first.call(R, levels, 1, lut, stream=s) == OK, R.last_error()
        assert second.call(R, levels, 0, lut, stream=s, src_ptr=first.d_rec.data_ptr() + first.lead[2], pitch0=first.pitch[2], fs0=first.fs[2]) == OK, \
            R.last_error()
    torch.cuda.synchronize()
    g1, r1 = first.outputs("first call")
    grids = np.stack([oracle.encode(im, levels, lut, 1) for im in imgs])
    want1 = np.stack([oracle.decode(g, levels, 1) for g in grids])
    assert_same(g1, grids, "first grid")
    assert_same(r1, want1, "first reconstruction")
    second.src = second.d_src.cpu().numpy()      # (its own input parent was not used)
    g2, r2 = second.outputs("second call")
    grids2 = np.stack([oracle.encode(im, levels, lut, 0) for im in want1])
    assert_same(g2, grids2, "second grid")
    assert_same(r2, np.stack([oracle.decode(g, levels, 0) for g in grids2]), "second reconstruction")


def _codec(levels, interp):
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    return H.Encoder(Crossed() if interp else LeftTop(), Linear.from_level(QuantizationLevel.Medium), levels)


def test_python_mirror_fused_and_composed_routes(R, oracle):
    """Encoder.encode_with_reconstruction on CUDA views (into canvas windows) and numpy arrays, against the oracle: the fused
    launch, and the routes composed from encode_view + decode_view -- 16 x 16 at level 0, 520 x 300 at level 9, and a view placed
    against the tail rule."""
    import torch
    lut = oracle.linear_lut(oracle.MEDIUM)[0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + 9)
    parent = torch.randint(0, 256, (3, 400, 700), dtype=torch.uint8, device="cuda", generator=gen)
    host = parent.cpu().numpy()
    for (x0, y0, w, h, levels, interp) in ((0, 0, 700, 400, 4, 1), (33, 7, 520, 300, 9, 1), (100, 50, 16, 16, 0, 0), (5, 3, 258, 131, 7, 0),
                                           (64, 64, 384, 128, 2, 1)):
        enc = _codec(levels, interp)
        view = parent[:, y0:y0 + h, x0:x0 + w]
        crop = host[:, y0:y0 + h, x0:x0 + w]
        grids = np.stack([oracle.encode(im, levels, lut, interp) for im in crop])
        want = np.stack([oracle.decode(g, levels, interp) for g in grids])
        what = "view %r L%d" % ((x0, y0, w, h), levels)
        g, r = enc.encode_with_reconstruction(view)
        torch.cuda.synchronize()
        assert g.is_contiguous() and r.is_contiguous() and tuple(g.shape) == tuple(r.shape) == (3, h, w)
        assert_same(g.cpu().numpy(), grids, "grid " + what)
        assert_same(r.cpu().numpy(), want, "reconstruction " + what)
        gc = torch.full((3, 409, 713), SENT, dtype=torch.uint8, device="cuda")
        rc = torch.full((3, 405, 777), SENT, dtype=torch.uint8, device="cuda")
        g2, r2 = enc.encode_with_reconstruction(view, out=gc[:, 2:2 + h, 5:5 + w], recon=rc[:, 1:1 + h, 9:9 + w])
        torch.cuda.synchronize()
        assert g2.data_ptr() == gc[:, 2:, 5:].data_ptr() and r2.data_ptr() == rc[:, 1:, 9:].data_ptr()
        hg, hr = gc.cpu().numpy(), rc.cpu().numpy()
        assert_same(hg[:, 2:2 + h, 5:5 + w], grids, "canvas grid " + what)
        assert_same(hr[:, 1:1 + h, 9:9 + w], want, "canvas reconstruction " + what)
        hg[:, 2:2 + h, 5:5 + w] = SENT
        hr[:, 1:1 + h, 9:9 + w] = SENT
        assert (hg == SENT).all() and (hr == SENT).all(), "written outside the windows: " + what
        # numpy: a 2-D crop of frame 1, uploaded and downloaded
        ng, nr = enc.encode_with_reconstruction(crop[1])
        assert_same(ng, grids[1], "numpy grid " + what)
        assert_same(nr, want[1], "numpy reconstruction " + what)
        assert (parent.cpu().numpy() == host).all(), "the parent was modified"
    # a (70, 130) view whose last byte is the last byte of a page: composed, the same bytes
    w, h, pitch, levels = 130, 70, 133, 4
    buf = torch.randint(0, 256, (3 * 4096 + h * pitch,), dtype=torch.uint8, device="cuda", generator=gen)
    off = (-(buf.data_ptr() + (h - 1) * pitch + w)) % 4096
    view = buf[off:off + h * pitch].view(h, pitch)[:, :w]
    assert (view.data_ptr() + (h - 1) * pitch + w) % 4096 == 0 and not tail_rule(view.data_ptr(), 1, h, w, pitch, 0)
    st = R.lib().hgi_recon_encode_u8_dev(None, view.data_ptr(), pitch, w, h, levels, 1, lut.ctypes.data, parent.data_ptr(), 700,
                                         parent[1].data_ptr(), 700, 1, 0, 0, 0)
    assert st == EUNSUPPORTED      # (the library refuses this placement: nothing was written, checked below)
    assert (parent.cpu().numpy() == host).all()
    g, r = _codec(levels, 1).encode_with_reconstruction(view)
    torch.cuda.synchronize()
    crop = view.cpu().numpy()
    want = oracle.encode(crop, levels, lut, 1)
    assert_same(g.cpu().numpy(), want, "grid of the view against the tail rule")
    assert_same(r.cpu().numpy(), oracle.decode(want, levels, 1), "reconstruction of the view against the tail rule")
