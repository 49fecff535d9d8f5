"""GPU suite of requantize (hgi_requant_dev, Encoder.requantize): for every shape, depth, pitch and alignment the destination,
read through its pitch, must be the oracle's encode, with the new table, of the oracle's decode of the source grid, bit for
bit; no byte outside the destination rows may be written and the source must come back unmodified.  Every case reads its
source out of a parent buffer of RANDOM bytes and writes into a SENTINEL-filled parent that is checked whole.  Expected bytes:
the oracle (or tests/golden).  Never libhgi_hip.so, never the library under test."""
import functools

import numpy as np
import pytest

import geometry_designs as G
import operand_designs as D
from conftest import SEED0
from kernel_calls import Plane, Pool, dev, same_dev

pytestmark = pytest.mark.gpu
SENT = 0xC3
GAPS = (1, 3, 16, 61, 128)
OK, EINVAL, EUNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def Q():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from rustyhgi_amd import _ffi_requant
    assert _ffi_requant.lib() is not None
    return _ffi_requant


def assert_same(a, b, what):
    if a.shape != b.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
    if not (a == b).all():
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def rows_index(B, h, w, lead, pitch, fstride):
    return lead + (np.arange(B)[:, None, None] * fstride + np.arange(h)[None, :, None] * pitch + np.arange(w)[None, None, :])


def tail_rule(ptr, B, h, w, pitch, fstride):
    """include/hgi_requant.h: width % 4 != 0 is served iff the three bytes behind the last source frame's span lie in the 4-KiB
    page of its last byte."""
    end = ptr + (B - 1) * (fstride if B > 1 else 0) + (h - 1) * pitch + w
    return w % 4 == 0 or (end - 1) >> 12 == (end + 2) >> 12


def stream_arg():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


class Placed:
    """(B, h, w) grids placed for one call: the source in a parent of random bytes, the destination in a sentinel parent."""

    def __init__(self, frames, pitches, leads=(0, 0), extras=(0, 0), seed=1, violate_tail=False):
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
        self.d_dst = torch.full((self.total[1],), SENT, dtype=torch.uint8, device="cuda")

    @property
    def src_ptr(self):
        return self.d_src.data_ptr() + self.lead[0]

    @property
    def dst_ptr(self):
        return self.d_dst.data_ptr() + self.lead[1]

    def call(self, Q, levels, interp, lut, stream=0, src_ptr=None, pitch0=None, fs0=None, dst_ptr=None):
        lut = np.ascontiguousarray(lut, np.uint8)
        return Q.lib().hgi_requant_dev(stream or None, src_ptr or self.src_ptr, pitch0 or self.pitch[0], self.w, self.h, levels, interp,
                                       lut.ctypes.data, dst_ptr or self.dst_ptr, self.pitch[1], self.B, fs0 or self.fs[0], self.fs[1])

    def output(self, what):
        """The destination read through its pitch (after a sync); every other byte of its parent must hold the sentinel and
        the source parent its bytes."""
        host = self.d_dst.cpu().numpy()
        idx = rows_index(self.B, self.h, self.w, self.lead[1], self.pitch[1], self.fs[1])
        mask = np.zeros(self.total[1], bool)
        mask[idx] = True
        stray = np.nonzero(host[~mask] != SENT)[0]
        assert len(stray) == 0, "%s: %d bytes outside the destination rows written" % (what, len(stray))
        assert (self.d_src.cpu().numpy() == self.src).all(), what + ": the source parent was modified"
        return host[idx]

    def untouched(self):
        return bool((self.d_dst == SENT).all()) and bool((self.d_src.cpu().numpy() == self.src).all())


def run(Q, grids, levels, interp, lut, pitches, what, **kw):
    import torch
    p = Placed(grids, pitches, **kw)
    st = p.call(Q, levels, interp, lut)
    assert st == OK, "%s: status %d: %s" % (what, st, Q.last_error())
    torch.cuda.synchronize()
    return p.output(what)


def recode(oracle, grids, levels, interp, lut):
    return np.stack([oracle.encode(oracle.decode(g, levels, interp), levels, lut, interp) for g in grids])


def check(Q, oracle, grids, levels, interp, lut, pitches, what, **kw):
    assert_same(run(Q, grids, levels, interp, lut, pitches, what, **kw), recode(oracle, grids, levels, interp, lut), what)


def three_tables(oracle):
    return [("low", oracle.linear_lut(oracle.LOW)[0]), ("medium", oracle.linear_lut(oracle.MEDIUM)[0]), ("high", oracle.linear_lut(oracle.HIGH)[0])]


# ---------------------------------------------------------------------------------------------- 1. golden small cases
def test_small_golden_grids_recoded_with_low_medium_high(Q, oracle, golden, small):
    """Every stored grid of tests/golden/small_cases.npz at levels 1 ... 8 (whatever quantizer made it, both interpolators) as
    the source, re-coded with Low, Medium and High; different gaps from {1, 3, 16, 61, 128} on the two sides, leads 0 ... 15."""
    n = 0
    for key in golden:
        if ("grid/" + key) not in small:
            continue
        name, lv, q, i = key.split("/")
        levels, interp = int(lv[1:]), int(i[1:])
        if not 1 <= levels <= 8:
            continue
        src = small["grid/" + key]
        assert_same(oracle.decode(src, levels, interp), small["dec/" + key], "the oracle against the stored decode of " + key)
        h, w = src.shape
        for t, (tname, lut) in enumerate(three_tables(oracle)):
            a = (n + t) % 5
            pitches = (w + GAPS[a], w + GAPS[(a + 1 + (n // 5) % 3) % 5])
            assert pitches[0] != pitches[1]
            check(Q, oracle, src[None], levels, interp, lut, pitches, "%s -> %s" % (key, tname), leads=((n + t) % 16, (5 * n + 3 + t) % 16), seed=n)
        n += 1
    assert n == 90


# ---------------------------------------------------------------------------------------------- 2. random-byte sources
NOISE = [(1, 1), (5, 3), (128, 64), (131, 67), (256, 128), (300, 200)]


@pytest.mark.parametrize("w,h", NOISE)
def test_random_byte_sources_levels_1_to_8(Q, oracle, w, h):
    """Sources of random bytes -- every residual value appears and the decoder's sums wrap -- at levels 1 ... 8, batches 1 and 3
    with frame strides above the span, the interpolators alternating, linear and random tables alternating."""
    rng = np.random.default_rng(SEED0 + 13 * w + h)
    tabs = three_tables(oracle)
    for levels in range(1, 9):
        for B in (1, 3):
            interp = (levels + B + w) & 1
            grids = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
            lut = tabs[levels % 3][1] if B == 1 else rng.integers(0, 256, 256, dtype=np.uint8)
            pitches = (w + GAPS[levels % 5], w + GAPS[(levels + 2) % 5])
            check(Q, oracle, grids, levels, interp, lut, pitches, "%dx%d L%d B%d" % (w, h, levels, B), leads=(levels, 16 - levels),
                  extras=(77 + levels, 1000 + B), seed=levels)


def test_several_tiles_under_one_cone(Q, oracle):
    """384 x 320 at levels 6, 7 and 8: 3 x 5 interior tiles whose cones overlap; packed and pitched, batches 1 and 3."""
    rng = np.random.default_rng(SEED0 + 384)
    w, h = 384, 320
    for levels in (6, 7, 8):
        for B, interp in ((1, 1), (3, 0), (1, 0), (3, 1)):
            grids = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
            lut = oracle.linear_lut(1 + levels % 3)[0] if interp else rng.integers(0, 256, 256, dtype=np.uint8)
            pitches = (w, w) if B == 1 and interp else (w + GAPS[levels % 5], w + GAPS[(levels + 3) % 5])
            check(Q, oracle, grids, levels, interp, lut, pitches, "384x320 L%d B%d i%d" % (levels, B, interp), leads=(levels % 16, 3),
                  extras=(levels, 4096), seed=levels)


# ---------------------------------------------------------------------------------------------- 3. ragged tiles
@functools.lru_cache(maxsize=2)
def ragged_expected(setname, levels):
    """[(w, h, interp, table, source grids, expected grids)], two frames each: the source is the oracle's LOSSLESS encode of the
    geometry suite's content, so the decoded image is the design; interpolators and the three tables alternate over the shapes."""
    from oracle import hgi_oracle as O
    O.build()
    tabs = three_tables(O)
    out = []
    for k, (w, h) in enumerate(G.shape_set(setname)):
        img = G.content(w, h, batch=2)
        interp, lut = k & 1, tabs[k % 3][1]
        src = np.stack([O.encode(img[f], levels, O.noop_lut(), interp) for f in range(2)])
        dec = np.stack([O.decode(src[f], levels, interp) for f in range(2)])
        assert (dec == img).all(), (w, h, levels)
        out.append((w, h, interp, lut, src, np.stack([O.encode(dec[f], levels, lut, interp) for f in range(2)])))
    return out


@pytest.mark.parametrize("setname,levels", [("R", 4), ("D", 5), ("D", 6), ("D", 7), ("D", 8)], ids=lambda v: str(v))
def test_every_remainder_of_a_ragged_tile(Q, setname, levels):
    """G.shape_set("R") at level 4 -- every column remainder 1 ... 127 and every row remainder 1 ... 63 of a ragged tile, with
    and without an interior neighbour, through both EDGE forms of dec_fine_keep -- and the deep set D at levels 5 ... 8.  All
    destinations lie in ONE sentinel-filled buffer that is compared whole, all sources in one buffer of nonzero random bytes
    that must come back unchanged (the Pool of the geometry suite), batch 2, a pitch and a lead of its own on each side."""
    import torch
    E = ragged_expected(setname, levels)
    inp, out, calls = Pool(False, levels + 900), Pool(True), []
    for w, h, interp, lut, src, want in E:
        ps, pd = w + 16, w + 61
        ss, sd = h * ps + 3, h * pd + 1
        calls.append((w, h, interp, lut, ps, pd, ss, sd, inp.add(src, ps, ss, lead=5, tail_safe=w % 4 != 0),
                      out.add(want, pd, sd, lead=1, tag="%d x %d requant" % (w, h))))
    inp.upload(), out.upload()
    stream = stream_arg()
    for w, h, interp, lut, ps, pd, ss, sd, i_src, o in calls:
        Q.check(Q.lib().hgi_requant_dev(stream, inp.ptr + i_src, ps, w, h, levels, interp, lut.ctypes.data, out.ptr + o, pd, 2, ss, sd))
    what = "requant %s L%d" % (setname, levels)
    out.check(what), inp.check(what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. operand designs
TABLES_PLUS = dict(D.tables(), nonzero_origin=D.table_nonzero_origin())


def _designs():
    """name -> (frame name, levels, table names): the operand suite's designs up to eight levels, without the identity table
    (the library refuses it: test_refusals_write_nothing)."""
    out = {}
    for name, frame, lv, _ in D.quant_designs():
        big = D.quant_frame(frame).size > 12e6
        out[name] = (frame, lv, ("linear2", "identity_but_255", "random0") if big else tuple(t for t in TABLES_PLUS if t != "identity"))
    for frame, (lv, _) in D.PRED_FRAMES.items():
        out["%s_L%d" % (frame, lv)] = (frame, lv, ("linear2",))
    return out


DESIGNS = _designs()
DESIGN_CASES = [(d, i) for d in DESIGNS for i in (1, 0)]


@pytest.mark.parametrize("design,interp", DESIGN_CASES, ids=["%s-i%d" % c for c in DESIGN_CASES])
def test_operand_designs_lifted_losslessly(Q, oracle, design, interp):
    """The quantizer and predictor designs of the operand suite, lifted to a source grid by the oracle's lossless encode (its
    decode is the design: asserted) and re-coded with the designs' own tables: the encoder half meets exactly the (prediction,
    pixel) pairs the operand suite gives hgi_encode_u8_dev, the decoder half every residual that lifts them."""
    frame, levels, tnames = DESIGNS[design]
    img = D.pred_frame(frame) if frame in D.PRED_FRAMES else D.quant_frame(frame)
    h, w = img.shape
    lifted = oracle.encode(img, levels, oracle.noop_lut(), interp)
    dec = oracle.decode(lifted, levels, interp)
    assert (dec == img).all(), "the lift of %s is not lossless" % design
    src = Plane(h, w, w + 16, 5, random=True, seed=levels, tail_w=w).put(dev(lifted))
    before = src.buf.clone()
    import torch
    for tname in tnames:
        lut = np.ascontiguousarray(TABLES_PLUS[tname])
        dst = Plane(h, w, w + 61, 1)
        Q.check(Q.lib().hgi_requant_dev(stream_arg(), src.ptr, src.pitch, w, h, levels, interp, lut.ctypes.data, dst.ptr, dst.pitch, 1,
                                        h * src.pitch, h * dst.pitch))
        what = "%s %s interp %d requant" % (design, tname, interp)
        same_dev(dst.rows(), dev(oracle.encode(dec, levels, lut, interp)), what)
        dst.intact(what)
    assert torch.equal(src.buf, before), design + ": the source parent was modified"


# ---------------------------------------------------------------------------------------------- 5. stream order
def _chain_case(oracle):
    rng = np.random.default_rng(SEED0 + 5)
    w, h, B, levels, interp = 384, 127, 2, 4, 1
    imgs = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
    src = np.stack([oracle.encode(im, levels, oracle.noop_lut(), interp) for im in imgs])
    medium, high = oracle.linear_lut(oracle.MEDIUM)[0], oracle.linear_lut(oracle.HIGH)[0]
    want1 = recode(oracle, src, levels, interp, medium)
    want2 = recode(oracle, want1, levels, interp, high)
    return w, h, levels, interp, src, medium, high, want1, want2


def test_two_calls_in_stream_order(Q, oracle):
    """Lossless-encoded source -> Medium, then that result -> High into a third buffer, on one side stream with no sync between
    the calls: both results are the oracle's two-step composition."""
    import torch
    w, h, levels, interp, src, medium, high, want1, want2 = _chain_case(oracle)
    first = Placed(src, (w + 16, w + 3), leads=(0, 4), extras=(1, 2))
    second = Placed(np.zeros_like(src), (w, w + 61), leads=(0, 1), extras=(0, 5))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = torch.cuda.current_stream().cuda_stream
        assert s == side.cuda_stream
        assert first.call(Q, levels, interp, medium, stream=s) == OK, Q.last_error()
        assert second.call(Q, levels, interp, high, stream=s, src_ptr=first.dst_ptr, pitch0=first.pitch[1], fs0=first.fs[1]) == OK, Q.last_error()
    torch.cuda.synchronize()
    assert_same(first.output("first call"), want1, "first call")
    second.src = second.d_src.cpu().numpy()      # (its own source parent was not used)
    assert_same(second.output("second call"), want2, "second call")


def test_two_calls_captured_into_a_graph(Q, oracle):
    """The same two calls captured once into a graph (a single chain, no parallel branches) and replayed once."""
    import torch
    w, h, levels, interp, src, medium, high, want1, want2 = _chain_case(oracle)
    first = Placed(src, (w + 16, w + 3), leads=(0, 4), extras=(1, 2))
    second = Placed(np.zeros_like(src), (w, w + 61), leads=(0, 1), extras=(0, 5))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        st1 = first.call(Q, levels, interp, medium, stream=s)
        st2 = second.call(Q, levels, interp, high, stream=s, src_ptr=first.dst_ptr, pitch0=first.pitch[1], fs0=first.fs[1])
    assert st1 == OK and st2 == OK, Q.last_error()
    torch.cuda.synchronize()
    assert first.untouched(), "capturing ran the launch"
    graph.replay()
    torch.cuda.synchronize()
    assert_same(first.output("first captured call"), want1, "first captured call")
    second.src = second.d_src.cpu().numpy()
    assert_same(second.output("second captured call"), want2, "second captured call")


# ---------------------------------------------------------------------------------------------- 6. refusals on the device
def test_refusals_write_nothing(Q, oracle):
    """Levels 0 and 9, the identity table, a violated tail rule and in place: each returns its status with both parents untouched."""
    import torch
    rng = np.random.default_rng(5)
    grids = rng.integers(0, 256, (2, 70, 130), dtype=np.uint8)
    lut = oracle.linear_lut(oracle.MEDIUM)[0]
    p = Placed(grids, (133, 146), leads=(3, 5), extras=(9, 11))
    assert p.call(Q, 0, 1, lut) == EUNSUPPORTED and "levels" in Q.last_error()
    assert p.call(Q, 9, 1, lut) == EUNSUPPORTED and "levels" in Q.last_error()
    assert p.call(Q, 4, 1, np.arange(256, dtype=np.uint8)) == EUNSUPPORTED and "identity" in Q.last_error() and "copy" in Q.last_error()
    assert p.call(Q, 4, 1, lut, dst_ptr=p.src_ptr) == EINVAL and "in-place" in Q.last_error()
    assert p.call(Q, 4, 1, lut, dst_ptr=p.src_ptr + 50) == EINVAL and "overlaps" in Q.last_error()
    torch.cuda.synchronize()
    assert p.untouched()
    v = Placed(grids, (133, 146), leads=(3, 5), extras=(9, 11), violate_tail=True)
    st = v.call(Q, 4, 1, lut)
    assert st == EUNSUPPORTED and "tail" in Q.last_error(), (st, Q.last_error())
    torch.cuda.synchronize()
    assert v.untouched()
    # the same placement four bytes earlier is served
    assert tail_rule(v.src_ptr - 4, 2, 70, 130, 133, v.fs[0])


# ---------------------------------------------------------------------------------------------- 7. Python
def _codec(levels, interp, table="medium"):
    import rustyhgi_amd as H
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    from rustyhgi_amd.quantizator import Linear, NoOp, QuantizationLevel
    q = NoOp() if table == "identity" else Linear.from_level(QuantizationLevel.Medium)
    return H.Encoder(Crossed() if interp else LeftTop(), q, levels)


def test_python_requantize_fused_and_composed_routes(Q, oracle):
    """Encoder.requantize on CUDA views (packed, strided, into canvas windows; B = 1 and 3) and numpy arrays against the oracle:
    the fused launch, and the composed route -- 520 x 300 at level 9 -- and the identity table (rows copied) at levels 4, 9 and 0."""
    import torch
    medium = oracle.linear_lut(oracle.MEDIUM)[0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + 9)
    parent = torch.randint(0, 256, (3, 400, 700), dtype=torch.uint8, device="cuda", generator=gen)
    host = parent.cpu().numpy()
    cases = ((0, 0, 700, 400, 4, 1, "medium"), (33, 7, 520, 300, 9, 1, "medium"), (5, 3, 258, 131, 7, 0, "medium"), (64, 64, 384, 128, 2, 1, "medium"),
             (17, 9, 300, 200, 4, 0, "identity"), (3, 11, 258, 131, 9, 1, "identity"), (40, 20, 64, 48, 0, 0, "identity"))
    for (x0, y0, w, h, levels, interp, table) in cases:
        enc = _codec(levels, interp, table)
        lut = medium if table == "medium" else oracle.noop_lut()
        view = parent[:, y0:y0 + h, x0:x0 + w]
        crop = host[:, y0:y0 + h, x0:x0 + w]
        want = recode(oracle, crop, levels, interp, lut)
        if table == "identity":
            assert_same(want, crop, "encode(decode(g), identity) == g")
        what = "view %r L%d %s" % ((x0, y0, w, h), levels, table)
        g = enc.requantize(view)
        torch.cuda.synchronize()
        assert g.is_contiguous() and tuple(g.shape) == (3, h, w)
        assert_same(g.cpu().numpy(), want, what)
        canvas = torch.full((3, 409, 713), SENT, dtype=torch.uint8, device="cuda")
        g2 = enc.requantize(view, out=canvas[:, 2:2 + h, 5:5 + w])
        torch.cuda.synchronize()
        assert g2.data_ptr() == canvas[:, 2:, 5:].data_ptr()
        hc = canvas.cpu().numpy()
        assert_same(hc[:, 2:2 + h, 5:5 + w], want, "canvas " + what)
        hc[:, 2:2 + h, 5:5 + w] = SENT
        assert (hc == SENT).all(), "written outside the window: " + what
        # B = 1: a 2-D strided view of frame 1, and the packed copy of it
        assert_same(enc.requantize(view[1]).cpu().numpy(), want[1], "2-D view " + what)
        assert_same(enc.requantize(view[1].contiguous()).cpu().numpy(), want[1], "packed " + what)
        # numpy: a 2-D crop of frame 2, uploaded and downloaded
        assert_same(enc.requantize(crop[2]), want[2], "numpy " + what)
        assert (parent.cpu().numpy() == host).all(), "the parent was modified"
        with pytest.raises(ValueError, match="shares memory"):
            enc.requantize(view, out=view)
