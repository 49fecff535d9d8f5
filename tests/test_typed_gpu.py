"""GPU suite of typed encode (hgi_typed_encode_dev, Encoder.encode_typed): for every shape, depth, pitch, alignment, element
size and kind the grid, read through its pitch, must be `oracle.encode(quantize(frame, scale, bias))` bit for bit
(tests/typed_reference.py restates the conversion in numpy); no byte outside the grid rows may be written and the frames must
come back unmodified.  Every case reads its frames out of a parent of RANDOM bytes -- the gaps hold arbitrary bit patterns, NaN
and infinity included -- and writes into a SENTINEL-filled parent that is checked whole.  Each call runs once.  Expected values:
the oracle and numpy.  Never the library under test."""
import numpy as np
import pytest

import typed_reference as TR
from conftest import SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3
OK, EINVAL, EUNSUPPORTED = 0, 1, 4
F16, BF16, F32 = "float16", "bfloat16", "float32"
KINDS = (F16, F32, BF16)                       # "E alternating 2 / 4 / bfloat16"
ESIZE = {F16: 2, BF16: 2, F32: 4}
EKIND = {F16: 0, BF16: 1, F32: 0}
BITS = {2: np.uint16, 4: np.uint32}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from rustyhgi_amd import _ffi_typed
    assert _ffi_typed.lib() is not None
    return _ffi_typed


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %#x want %#x" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def rows_index(B, h, n, lead, pitch, fstride):
    """byte indices of B x h rows of n bytes"""
    return lead + (np.arange(B)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch + np.arange(n)[None, None, :])


def page_rule(ptr, B, h, w, E, pitch, fstride):
    """include/hgi_typed.h: 2-byte elements of an odd width are served iff the last image frame's span does not end a 4-KiB page."""
    end = ptr + (B - 1) * (fstride if B > 1 else 0) + (h - 1) * pitch + w * E
    return E == 4 or w % 2 == 0 or end % 4096 != 0


def to_elements(values, kind):
    """float32 values -> the element array the reference takes: float16, float32, or bfloat16 bit patterns (uint16)."""
    v = np.asarray(values, np.float32)
    return {F16: lambda: v.astype(np.float16), F32: lambda: v, BF16: lambda: TR.bf16_bits(v)}[kind]()


def element_bits(x):
    return np.ascontiguousarray(x).view(BITS[x.dtype.itemsize])


class Placed:
    """(B, h, w) frames placed for one call: the frames (E-byte elements) in a parent of random bytes, the grids in a sentinel
    parent.  `gaps`: (image gap in ELEMENTS, grid gap in bytes); `leads`: bytes, the image's a multiple of E; `extras`: bytes
    between a frame's span and the next frame, the image's a multiple of E."""

    def __init__(self, frames, kind, gaps=(0, 0), leads=(0, 0), extras=(0, 0), seed=1, violate_page=False):
        import torch
        self.kind, self.E = kind, ESIZE[kind]
        E = self.E
        bits = element_bits(frames)
        assert bits.dtype == BITS[E]
        self.B, self.h, self.w = B, h, w = bits.shape
        assert leads[0] % E == 0 and extras[0] % E == 0
        self.pitch = [(w + gaps[0]) * E, w + gaps[1]]
        self.row = [w * E, w]
        self.span = [(h - 1) * p + r for p, r in zip(self.pitch, self.row)]
        self.fs = [s + e for s, e in zip(self.span, extras)]
        self.total = [l + (B - 1) * f + s + 4096 + 64 for l, f, s in zip(leads, self.fs, self.span)]
        self.d_img = torch.empty((self.total[0],), dtype=torch.uint8, device="cuda")
        self.lead = list(leads)
        p0 = self.d_img.data_ptr()
        assert p0 % 4 == 0
        if violate_page:      # the last frame's last byte on the last byte of a page
            end = p0 + self.lead[0] + (B - 1) * self.fs[0] + self.span[0]
            self.lead[0] += (-end) % 4096
            assert E == 2 and w % 2 and not page_rule(p0 + self.lead[0], B, h, w, E, self.pitch[0], self.fs[0])
        elif not page_rule(p0 + self.lead[0], B, h, w, E, self.pitch[0], self.fs[0]):
            self.lead[0] += 4      # off the page's end: the call runs fused
        rng = np.random.default_rng(seed)
        self.src = rng.integers(0, 256, self.total[0], dtype=np.uint8)
        self.src[rows_index(B, h, w * E, self.lead[0], self.pitch[0], self.fs[0])] = bits.view(np.uint8).reshape(B, h, w * E)
        self.d_img.copy_(torch.from_numpy(self.src))
        self.d_grid = torch.full((self.total[1],), SENT, dtype=torch.uint8, device="cuda")

    def call(self, T, levels, interp, lut, scale, bias, stream=0, img_back=0, **kw):
        a = dict(elem=self.E, kind=EKIND[self.kind], img_pitch=self.pitch[0])
        a.update(kw)
        lut = np.ascontiguousarray(lut, np.uint8)
        return T.lib().hgi_typed_encode_dev(stream or None, self.d_img.data_ptr() + self.lead[0] - img_back, a["img_pitch"], a["elem"], a["kind"],
                                            float(np.float32(scale)), float(np.float32(bias)), self.w, self.h, levels, interp,
                                            lut.ctypes.data, self.d_grid.data_ptr() + self.lead[1], self.pitch[1], self.B, self.fs[0], self.fs[1])

    def grids(self, what):
        """The grids read through their pitch as (B, h, w) (after a sync); every other byte of their parent must hold the
        sentinel and the image parent its bytes."""
        host = self.d_grid.cpu().numpy()
        idx = rows_index(self.B, self.h, self.w, self.lead[1], self.pitch[1], self.fs[1])
        mask = np.zeros(self.total[1], bool)
        mask[idx] = True
        stray = np.nonzero(host[~mask] != SENT)[0]
        assert len(stray) == 0, "%s: %d bytes outside the grid rows written" % (what, len(stray))
        assert (self.d_img.cpu().numpy() == self.src).all(), what + ": the image parent was modified"
        return np.ascontiguousarray(host[idx])

    def untouched(self):
        return bool((self.d_grid == SENT).all())


def expected(oracle, frames, scale, bias, levels, lut, interp):
    return np.stack([oracle.encode(TR.quantize(f, scale, bias), levels, lut, interp) for f in frames])


def check(T, oracle, frames, kind, levels, interp, lut, scale, bias, what, want=None, **kw):
    """One call on `frames` (B, h, w) elements; `want`: the expected grids when the caller has them already."""
    import torch
    p = Placed(frames, kind, **kw)
    st = p.call(T, levels, interp, lut, scale, bias)
    assert st == OK, "%s: status %d: %s" % (what, st, T.last_error())
    torch.cuda.synchronize()
    if want is None:
        want = expected(oracle, frames, scale, bias, levels, lut, interp)
    assert_same(p.grids(what), want, what)


def table_of(kind):
    """affine_table(dtype) as the reference's element array."""
    import torch
    from rustyhgi_amd import affine_table
    if kind == BF16:
        return affine_table(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return affine_table({F16: np.float16, F32: np.float32}[kind])


def lut_for(oracle, q):
    return oracle.noop_lut() if q == "noop" else oracle.linear_lut(int(q))[0]


GAPS = (1, 3, 16, 61, 128)


def test_small_golden_cases(T, oracle, golden, small):
    """The tiny / odd shapes of tests/golden/small_cases.npz at levels 1 ... 8, both interpolators and the three quantizers as
    stored: the frame is affine_table(dtype)[stored image], scale 255, and the stored grid is expected back (the round trip
    through the table is exact).  Kinds alternate float16 / float32 / bfloat16; leads and pitches vary."""
    n = 0
    tables = {k: table_of(k) for k in KINDS}
    for key in golden:
        if ("grid/" + key) not in small:
            continue
        name, lv, q, i = key.split("/")
        levels, interp = int(lv[1:]), int(i[1:])
        if not 1 <= levels <= 8:
            continue
        kind = KINDS[n % 3]
        E = ESIZE[kind]
        frame = tables[kind][small["in/" + name]]
        check(T, oracle, frame[None], kind, levels, interp, lut_for(oracle, q[1:]), 255.0, 0.0, "%s %s" % (key, kind),
              want=small["grid/" + key][None], gaps=(GAPS[n % 5], GAPS[(n // 5 + 2) % 5]), leads=(E * ((5 * n + 3) % 8), n % 31), seed=n)
        n += 1
    assert n == 90


def pattern_frame(kind):
    """Every 16-bit pattern once, as a 256 x 256 frame in a fixed random permutation; float32: 256 x 256 random bit patterns and
    rows of specials behind them."""
    rng = np.random.default_rng(SEED0 + 0x71)
    if kind != F32:
        bits = rng.permutation(1 << 16).astype(np.uint16).reshape(256, 256)
        return bits if kind == BF16 else bits.view(np.float16)
    body = rng.integers(0, 1 << 32, (256, 256), dtype=np.uint64).astype(np.uint32)
    sp = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345]      # +-0, +-inf, quiet / signalling / negative NaN
    f = lambda v: int(np.float32(v).view(np.uint32))
    for k in range(256):
        h = np.float32(k + 0.5)
        sp += [f(np.nextafter(h, np.float32(-1e9))), f(h), f(np.nextafter(h, np.float32(1e9)))]
    sp += [f(-0.5), f(254.5), f(255.5), f(1e30), f(-1e30), f(np.float32(0.75) * np.float32(2.0 ** -126))]
    sp += [0] * (-len(sp) % 256)
    return np.concatenate([body, np.array(sp, np.uint32).reshape(-1, 256)]).view(np.float32)


@pytest.mark.parametrize("kind", KINDS)
def test_every_pattern(T, oracle, kind):
    """All 65 536 float16 / bfloat16 patterns (float32: random patterns and the specials), levels 1 and 4, Lossless and Medium,
    the three (scale, bias) pairs and (1, 0), under which every k + 0.5 is a tie; float32 also scale 2^127 (the denormal 0.75 * 2^-126 -> 1.5 -> 2 if denormals are honoured)
    and scale 0 (+-inf -> NaN -> 0)."""
    frame = pattern_frame(kind)
    pairs = list(TR.PAIRS) + [(1.0, 0.0)]
    if kind == F32:
        pairs += [(2.0 ** 127, 0.0), (0.0, 0.0)]
        den = np.float32(0.75) * np.float32(2.0 ** -126)
        assert den != 0 and TR.quantize(np.array([den], np.float32), 2.0 ** 127, 0.0)[0] == 2      # the reference honours denormals
        assert TR.quantize(np.array([np.inf, -np.inf], np.float32), 0.0, 0.0).tolist() == [0, 0]
    n = 0
    for scale, bias in pairs:
        px = TR.quantize(frame, scale, bias)
        if scale == 1.0:
            assert len(np.unique(px)) == 256      # every pixel value is met, not a saturated plane
        for levels in (1, 4):
            for q in (oracle.LOSSLESS, oracle.MEDIUM):
                lut = lut_for(oracle, q)
                want = oracle.encode(px, levels, lut, n & 1)[None]
                check(T, oracle, frame[None], kind, levels, n & 1, lut, scale, bias, "%s patterns x %r + %r L%d q%d" % (kind, scale, bias, levels, q),
                      want=want, gaps=(GAPS[n % 5], GAPS[(n + 2) % 5]), leads=(4 * (n % 4), n % 7), seed=n)
                n += 1


def biased_frames(kind, w, h, batch=1, salt=0):
    """Noise pixels v in [8, 255] as the elements v - 37.25 (exact in float16 and float32; bfloat16 rounds them, and the
    reference says which pixel each then means).  With scale 1, bias 37.25 the element 0.0 means pixel 37, so a kernel that
    converts range-checked zeros puts 37 where the codec wants 0."""
    rng = np.random.default_rng(SEED0 + 100003 * w + 1009 * h + salt)
    v = rng.integers(8, 256, (batch, h, w)).astype(np.float32) - np.float32(37.25)
    return to_elements(v, kind)


ZERO_SHAPES = [(1, 1), (3, 2), (5, 63), (127, 65), (129, 129), (131, 1), (257, 2), (1, 63), (3, 65), (5, 129), (257, 63), (129, 65)]


@pytest.mark.parametrize("w,h", ZERO_SHAPES)
def test_zero_means_pixel_zero(T, oracle, w, h):
    """scale 1, bias 37.25: 0.0 converts to 37.  Shapes whose edge predictions read outside the image, both interpolators,
    levels 2, 4, 5, 7, Medium."""
    lut = lut_for(oracle, oracle.MEDIUM)
    assert TR.quantize(np.zeros(1, np.float32), 1.0, 37.25)[0] == 37
    n = 0
    for levels in (2, 4, 5, 7):
        for interp in (1, 0):
            kind = KINDS[(n + w) % 3]
            frames = biased_frames(kind, w, h, salt=n)
            check(T, oracle, frames, kind, levels, interp, lut, 1.0, 37.25, "zero %dx%d L%d i%d %s" % (w, h, levels, interp, kind),
                  gaps=(GAPS[n % 5], GAPS[(n + 3) % 5]), leads=(4 * (n % 3), n % 5), seed=n)
            n += 1


@pytest.mark.parametrize("w,h", [(384, 127), (520, 300)])
def test_zero_means_pixel_zero_under_the_cone(T, oracle, w, h):
    """Levels 6, 7, 8: the cone's points outside the plane and the halo of the ragged tiles, same constants."""
    lut = lut_for(oracle, oracle.MEDIUM)
    n = 0
    for levels in (6, 7, 8):
        for interp in (1, 0):
            kind = KINDS[(n + 1) % 3]
            frames = biased_frames(kind, w, h, salt=n)
            check(T, oracle, frames, kind, levels, interp, lut, 1.0, 37.25, "cone zero %dx%d L%d i%d %s" % (w, h, levels, interp, kind),
                  gaps=(GAPS[n % 5], GAPS[(n + 3) % 5]), leads=(4 * (n % 3), n % 5), seed=n)
            n += 1


# Geometry: the remainder classes of tests/geometry_designs.py restated -- one interior tile followed by ragged ones, (128 + c,
# 64 + r): every right-edge remainder mod 16 (c = 1 ... 16) and a few wider ones, bottom remainders odd, even, short and full;
# EDGE 1 tiles (full width inside, even height), EDGE 2 (any other ragged tile), EDGE 0 (interior); frames below one tile.
GEOMETRY = [(128 + c, 64 + (1, 2, 38, 63, 64)[c % 5]) for c in list(range(1, 17)) + [17, 33, 64, 127, 128]] + \
           [(256, 70), (256, 71), (256, 128), (384, 64), (100, 37), (128, 64), (67, 64), (16, 3), (520, 300)]


@pytest.mark.parametrize("w,h", GEOMETRY)
def test_geometry(T, oracle, w, h):
    """Batch 3 with a frame stride above the span on both sides, float16 and float32 (bfloat16 on every third shape), levels
    cycling through 1 ... 8, pixels as x / 255."""
    n = w + h
    levels, interp = 1 + n % 8, n & 1
    lut = lut_for(oracle, (oracle.MEDIUM, oracle.HIGH, oracle.LOSSLESS)[n % 3])
    rng = np.random.default_rng(SEED0 + 7 * w + h)
    v = rng.integers(8, 256, (3, h, w)).astype(np.float32) * np.float32(1 / 255)
    for kind in (F16 if n % 3 else BF16, F32):
        E = ESIZE[kind]
        check(T, oracle, to_elements(v, kind), kind, levels, interp, lut, 255.0, 0.0, "geometry %dx%d L%d %s" % (w, h, levels, kind),
              gaps=(GAPS[n % 5], GAPS[(n + 1) % 5]), leads=(E * (n % 5), n % 11), extras=(E * (50 + n % 9), 77 + n % 13), seed=n)


@pytest.mark.parametrize("kind", (F16, F32))
def test_pitches_and_alignment(T, oracle, kind):
    """Image pitch = row + {E, 3E, 16E, 61E}, grid pitch = width + {1, 3, 16, 61}, the image pointer at every E-multiple offset
    within 16 bytes.  261 x 70 (an odd width: a ragged chunk, a bottom edge) and 384 x 127."""
    E = ESIZE[kind]
    lut = lut_for(oracle, oracle.MEDIUM)
    n = 0
    for w, h in ((261, 70), (384, 127)):
        rng = np.random.default_rng(SEED0 + w)
        frames = to_elements(rng.integers(0, 256, (2, h, w)).astype(np.float32) * np.float32(1 / 255), kind)
        want = expected(oracle, frames, 255.0, 0.0, 4, lut, 1)
        for off in range(0, 16, E):
            gi, gg = (1, 3, 16, 61)[n % 4], (1, 3, 16, 61)[(n // 4 + n) % 4]
            check(T, oracle, frames, kind, 4, 1, lut, 255.0, 0.0, "%s %dx%d +%d pitches +%dE / +%d" % (kind, w, h, off, gi, gg), want=want,
                  gaps=(gi, gg), leads=(off, (3 * n) % 16), extras=(E * n, n), seed=n)
            n += 1


def test_page_rule_both_sides(T, oracle):
    """2-byte elements of an odd width whose last frame ends on a page's last byte: refused (HGI_EUNSUPPORTED), nothing written;
    the same call one element earlier in the parent -- whose bytes are as good a frame as any -- is served."""
    import torch
    lut = lut_for(oracle, oracle.MEDIUM)
    rng = np.random.default_rng(5)
    frames = to_elements(rng.integers(0, 256, (2, 70, 131)).astype(np.float32) * np.float32(1 / 255), F16)
    p = Placed(frames, F16, gaps=(3, 16), leads=(6, 7), extras=(10, 9), violate_page=True)
    st = p.call(T, 4, 1, lut, 255.0, 0.0)
    assert st == EUNSUPPORTED and "4-KiB page" in T.last_error(), (st, T.last_error())
    # an EINVAL rule on a live device writes nothing either
    assert p.call(T, 4, 1, lut, 255.0, 0.0, elem=3) == EINVAL and "elem_size" in T.last_error()
    assert p.call(T, 4, 1, lut, float("nan"), 0.0) == EINVAL and "finite" in T.last_error()
    torch.cuda.synchronize()
    assert p.untouched()
    assert p.lead[0] >= 2 and page_rule(p.d_img.data_ptr() + p.lead[0] - 2, 2, 70, 131, 2, p.pitch[0], p.fs[0])
    shifted = p.src[rows_index(2, 70, 262, p.lead[0] - 2, p.pitch[0], p.fs[0])].view(np.float16)
    assert shifted.shape == (2, 70, 131)
    assert p.call(T, 4, 1, lut, 255.0, 0.0, img_back=2) == OK, T.last_error()
    torch.cuda.synchronize()
    assert_same(p.grids("one element inside the page"), expected(oracle, shifted, 255.0, 0.0, 4, lut, 1), "one element inside the page")


def test_identity_table(T, oracle):
    """Lossless through the IDENT instantiation (the table is the identity), levels 1, 4, 8, the three kinds."""
    lut = oracle.noop_lut()
    assert (lut == np.arange(256)).all()
    rng = np.random.default_rng(SEED0 + 3)
    for n, levels in enumerate((1, 4, 8)):
        kind = KINDS[n]
        frames = to_elements(rng.integers(0, 256, (2, 131, 300)).astype(np.float32) * np.float32(1 / 255), kind)
        check(T, oracle, frames, kind, levels, n & 1, lut, 255.0, 0.0, "identity L%d %s" % (levels, kind), gaps=(3, 16), leads=(4, 5), extras=(8, 3))


def test_graph_capture(T, oracle):
    """384 x 127, three levels, batch 2, pitches on both sides: the call captured on a side stream and replayed once gives the
    eager call's grids (which are the oracle's)."""
    import torch
    lut = lut_for(oracle, oracle.MEDIUM)
    rng = np.random.default_rng(SEED0 + 4)
    frames = to_elements(rng.integers(0, 256, (2, 127, 384)).astype(np.float32) * np.float32(1 / 255), F16)
    eager = Placed(frames, F16, gaps=(16, 3), leads=(8, 5), extras=(4, 1))
    assert eager.call(T, 3, 1, lut, 255.0, 0.0) == OK, T.last_error()
    torch.cuda.synchronize()
    want = eager.grids("eager")
    assert_same(want, expected(oracle, frames, 255.0, 0.0, 3, lut, 1), "eager")
    cap = Placed(frames, F16, gaps=(16, 3), leads=(8, 5), extras=(4, 1))
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = cap.call(T, 3, 1, lut, 255.0, 0.0, stream=side.cuda_stream)
    assert st == OK, T.last_error()
    torch.cuda.synchronize()
    assert cap.untouched(), "capturing must not run the launch"
    g.replay()
    torch.cuda.synchronize()
    assert_same(cap.grids("replayed"), want, "replayed")


def test_python_mirror_fused_and_composed_routes(T, oracle):
    """Encoder.encode_typed on a strided view of a larger tensor, on a non-default stream, for the three dtypes, against the
    oracle; nine levels (refused by the ABI) go through the composed route and give the oracle's grid too."""
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    lut = lut_for(oracle, oracle.MEDIUM)
    rng = np.random.default_rng(SEED0 + 6)
    host = rng.integers(0, 256, (3, 200, 420)).astype(np.float32) * np.float32(1 / 255)
    side = torch.cuda.Stream()
    for n, (tdt, kind) in enumerate(((torch.float16, F16), (torch.bfloat16, BF16), (torch.float32, F32))):
        parent = torch.from_numpy(host).cuda().to(tdt)
        back = parent.float().cpu().numpy()
        x0, y0, w, h = 6 + n, 3, 261 + n, 131
        view = parent[:, y0:y0 + h, x0:x0 + w]
        crop = to_elements(back[:, y0:y0 + h, x0:x0 + w], kind)
        for levels in (4, 9):
            enc = H.Encoder(Crossed(), Linear(QuantizationLevel.Medium), levels)
            assert (enc._lut == lut).all()
            want = expected(oracle, crop, 255.0, 0.0, levels, lut, 1)
            canvas = torch.full((3, 140, 300), SENT, dtype=torch.uint8, device="cuda")
            window = canvas[:, 2:2 + h, 9:9 + w]
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                r = enc.encode_typed(view)
                r2 = enc.encode_typed(view, out=window)
            torch.cuda.synchronize()
            what = "%s L%d" % (kind, levels)
            assert r.is_contiguous() and r.dtype == torch.uint8 and tuple(r.shape) == (3, h, w)
            assert_same(r.cpu().numpy(), want, what)
            assert r2.data_ptr() == window.data_ptr()
            hc = canvas.cpu().numpy().copy()
            assert_same(hc[:, 2:2 + h, 9:9 + w], want, "canvas " + what)
            hc[:, 2:2 + h, 9:9 + w] = SENT
            assert (hc == SENT).all(), "written outside the window: " + what
            # which route ran: the library serves four levels on these very arguments and refuses nine
            E = ESIZE[kind]
            st = T.lib().hgi_typed_encode_dev(None, view.data_ptr(), view.stride(1) * E, E, EKIND[kind], 255.0, 0.0, w, h, levels, 1,
                                              lut.ctypes.data, window.data_ptr(), window.stride(1), 3, view.stride(0) * E, window.stride(0))
            assert st == (OK if levels == 4 else EUNSUPPORTED), T.last_error()
            torch.cuda.synchronize()
        assert torch.equal(parent.float().cpu(), torch.from_numpy(back)), "the parent was modified"


def test_float_pipeline_round_trip(T, oracle):
    """frame -> grid -> frame without a uint8 image: Decoder.decode_mapped(enc.encode_typed(x), levels, affine_table(dtype))
    differs from x by at most err / 255 plus the table's rounding (half an ulp of the dtype below 1.0 at each end, and the
    float32 arithmetic of the table), on a smooth 512 x 300 frame at Medium."""
    import torch
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    _, err = oracle.linear_lut(oracle.MEDIUM)
    yy, xx = np.mgrid[0:300, 0:512]
    img = (127.5 + 100 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 20 * np.sin((xx + yy) / 11.0)).round().astype(np.uint8)
    half_ulp = {torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9, torch.float32: 2.0 ** -25}
    enc, dec = H.Encoder(Crossed(), Linear(QuantizationLevel.Medium), 4), H.Decoder(Crossed())
    for tdt in (torch.float16, torch.bfloat16, torch.float32):
        table = H.affine_table(tdt, device="cuda") if tdt is torch.bfloat16 else H.affine_table({torch.float16: np.float16, torch.float32: np.float32}[tdt], device="cuda")
        x = table[torch.from_numpy(img.astype(np.int64)).cuda()]
        grid = enc.encode_typed(x)
        y = dec.decode_mapped(grid, 4, table)
        torch.cuda.synchronize()
        assert y.dtype == tdt and tuple(y.shape) == (300, 512)
        assert_same(grid.cpu().numpy(), oracle.encode(img, 4, oracle.linear_lut(oracle.MEDIUM)[0], 1), "grid of table[img] %s" % tdt)
        diff = float((y.double() - x.double()).abs().max())
        tol = err / 255.0 + 2 * half_ulp[tdt] + 2.0 ** -22
        print("round trip %s: max |y - x| = %.6g, bound %.6g" % (tdt, diff, tol))
        assert diff <= tol, (tdt, diff, tol)
