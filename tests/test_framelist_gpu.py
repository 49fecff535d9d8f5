"""GPU suite of frame lists: every frame of a list of assorted shapes, encoded and decoded in one call, must equal the oracle (or
the uniform call, where the oracle is too slow), bit for bit, in every layout, and nothing outside the output frames may be
written."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEED0

pytestmark = pytest.mark.gpu
SENT = 0xA5
SHAPES = [(1, 1), (1, 97), (97, 1), (127, 63), (128, 64), (129, 65), (1000, 17), (17, 1000), (1300, 700)]      # (w, h)


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rustyhgi_amd
    from rustyhgi_amd import _ffi
    assert _ffi.lib() is not None
    return rustyhgi_amd


@pytest.fixture(scope="module")
def ctx(H):
    import torch
    c = H.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def assert_same(a, b, what):
    if a.shape != b.shape or not (a == b).all():
        if a.shape != b.shape:
            raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def table(q, seed):
    from oracle import hgi_oracle as O
    if q == "rand":
        return np.random.default_rng(seed).integers(0, 256, 256, dtype=np.uint8)
    return O.linear_lut(q)[0]


def images(oracle, shapes, seed):
    out = []
    for i, (w, h) in enumerate(shapes):
        out.append(oracle.synth(oracle.SYNTH_NOISE if i % 2 else oracle.SYNTH_RAMP, seed, i, w, h))
    return out


def assorted(oracle, lena, fullhd):
    return images(oracle, SHAPES, SEED0 + 70) + [lena, fullhd]


class Layout:
    """Where the frames of a list go: one sentinel-filled device buffer per side, frames at the given offsets.  `spans` keeps what
    each output frame may write; everything else must keep the sentinel."""

    def __init__(self, shapes, kind, seed=0):
        import torch
        rng = np.random.default_rng(seed)
        self.shapes = shapes
        self.offs, at = [], 1 + int(rng.integers(0, 15))
        for (w, h) in shapes:
            n = w * h
            if kind == "packed":              # back to back at odd offsets
                self.offs.append(at)
                at += n + 1 + 2 * int(rng.integers(0, 8))
            elif kind == "page_end":          # the frame's last byte 1 ... 3 bytes before a page end
                at = (at + n + 4096 + 4095) // 4096 * 4096 - n - int(rng.integers(1, 4))
                self.offs.append(at)
                at += n
            else:
                raise ValueError(kind)
        self.total = at + 4096
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda")
        self.base = self.buf.data_ptr()

    def ptrs(self):
        return [self.base + o for o in self.offs]

    def fill(self, frames):
        import torch
        for o, f in zip(self.offs, frames):
            if f.size:
                self.buf[o:o + f.size].copy_(torch.from_numpy(np.ascontiguousarray(f).reshape(-1)))

    def frames(self):
        host = self.buf.cpu().numpy()
        return [host[o:o + w * h].reshape(h, w) for o, (w, h) in zip(self.offs, self.shapes)], host

    def check_untouched(self, what):
        _, host = self.frames()
        mask = np.ones(self.total, bool)
        for o, (w, h) in zip(self.offs, self.shapes):
            mask[o:o + w * h] = False
        stray = np.nonzero(host[mask] != SENT)[0]
        assert len(stray) == 0, "%s: %d bytes outside the output frames written" % (what, len(stray))


def call_list(ctx, encode, ins, outs, shapes, levels, interp=1, lut=None):
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    n = len(shapes)
    pi = (ctypes.c_void_p * n)(*ins)
    po = (ctypes.c_void_p * n)(*outs)
    ws = (ctypes.c_uint32 * n)(*[w for w, h in shapes])
    hs = (ctypes.c_uint32 * n)(*[h for w, h in shapes])
    if encode:
        return L.hgi_encode_u8_list_dev(ctx.handle, pi, ws, hs, levels, interp, lut.ctypes.data, po, n), (pi, po, ws, hs)
    return L.hgi_decode_u8_list_dev(ctx.handle, pi, ws, hs, levels, interp, po, n), (pi, po, ws, hs)


def roundtrip(ctx, oracle, imgs, levels, interp, lut, kind, what, seed=0):
    """Encode the list into one layout, decode the oracle's grids into another: both against the oracle, sentinels kept."""
    import torch
    from rustyhgi_amd import _ffi
    shapes = [(f.shape[1], f.shape[0]) for f in imgs]
    want_g = [oracle.encode(f, levels, lut, interp) for f in imgs]
    want_i = [oracle.decode(g, levels, interp) for g in want_g]
    src, dst = Layout(shapes, kind, seed), Layout(shapes, kind, seed + 1)
    src.fill(imgs)
    _ffi.check(call_list(ctx, True, src.ptrs(), dst.ptrs(), shapes, levels, interp, lut)[0])
    torch.cuda.synchronize()
    got, _ = dst.frames()
    for i, (g, wnt) in enumerate(zip(got, want_g)):
        assert_same(g, wnt, "%s encode frame %d %dx%d L%d i%d" % (what, i, shapes[i][0], shapes[i][1], levels, interp))
    dst.check_untouched(what + " encode")
    src2, dst2 = Layout(shapes, kind, seed + 2), Layout(shapes, kind, seed + 3)
    src2.fill(want_g)
    _ffi.check(call_list(ctx, False, src2.ptrs(), dst2.ptrs(), shapes, levels, interp)[0])
    torch.cuda.synchronize()
    got, _ = dst2.frames()
    for i, (g, wnt) in enumerate(zip(got, want_i)):
        assert_same(g, wnt, "%s decode frame %d %dx%d L%d i%d" % (what, i, shapes[i][0], shapes[i][1], levels, interp))
    dst2.check_untouched(what + " decode")
    ins, _ = src2.frames()
    for g, wnt in zip(ins, want_g):
        assert (g == wnt).all(), "the grids were modified"


@pytest.mark.parametrize("levels", list(range(13)), ids=lambda v: "d%02d" % v)
def test_assorted_shapes_every_depth(ctx, oracle, lena, fullhd, levels):
    imgs = assorted(oracle, lena, fullhd)
    for interp in (1, 0):
        for q in (0, 2, 3, "rand"):
            roundtrip(ctx, oracle, imgs, levels, interp, table(q, SEED0 + levels), "packed", "q%s" % q, seed=levels * 7 + interp)


@pytest.mark.parametrize("levels", [3, 4, 7])
def test_layouts(ctx, oracle, lena, levels):
    """Page-end tails; separate allocations; one grid listed several times; zero-size frames interleaved."""
    import torch
    from rustyhgi_amd import _ffi
    lut = table(2, SEED0)
    imgs = images(oracle, SHAPES, SEED0 + 71) + [lena]
    roundtrip(ctx, oracle, imgs, levels, 1, lut, "page_end", "page-end")
    # separate allocations, zero-size frames between them (NULL pointers allowed there), one grid listed three times
    grids = [oracle.encode(f, levels, lut) for f in imgs]
    tg = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in grids]
    order = [0, None, 5, 5, 8, (0, 9), 5, 9, (4, 0), 3]
    ins, outs, shapes, keep = [], [], [], []
    for o in order:
        if o is None or isinstance(o, tuple):
            w, h = o if o else (0, 0)
            ins.append(None)
            outs.append(None)
            shapes.append((w, h))
            continue
        g = tg[o]
        out = torch.full((g.numel() + 64,), SENT, dtype=torch.uint8, device="cuda")
        keep.append((o, out))
        ins.append(g.data_ptr())
        outs.append(out.data_ptr() + 32)
        shapes.append((g.shape[1], g.shape[0]))
    _ffi.check(call_list(ctx, False, ins, outs, shapes, levels)[0])
    torch.cuda.synchronize()
    for o, out in keep:
        host = out.cpu().numpy()
        h, w = grids[o].shape
        assert_same(host[32:32 + w * h].reshape(h, w), oracle.decode(grids[o], levels), "separate frame %d" % o)
        assert (host[:32] == SENT).all() and (host[32 + w * h:] == SENT).all()


@pytest.mark.parametrize("levels", [4, 8])
def test_large_frames_equal_the_uniform_call(ctx, levels):
    """16 frames of 4096^2 (L4) / a 16384^2 L8 frame among small ones: the list call equals the uniform call, both directions."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    shapes = [(4096, 4096)] * 16 if levels == 4 else [(300, 200), (16384, 16384), (1, 1), (1920, 1080), (4099, 17)]
    lut = table(2, 0)
    imgs = []
    for i, (w, h) in enumerate(shapes):
        t = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE if i % 2 else _ffi.SYNTH_RAMP, SEED0 + i, i, w, h, t.data_ptr(), 1, w * h))
        imgs.append(t)
    grids = [torch.empty_like(t) for t in imgs]
    _ffi.check(call_list(ctx, True, [t.data_ptr() for t in imgs], [g.data_ptr() for g in grids], shapes, levels, 1, lut)[0])
    back = [torch.empty_like(t) for t in imgs]
    _ffi.check(call_list(ctx, False, [g.data_ptr() for g in grids], [b.data_ptr() for b in back], shapes, levels)[0])
    for i, ((w, h), t) in enumerate(zip(shapes, imgs)):
        g1 = torch.empty_like(t)
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, t.data_ptr(), w, h, levels, 1, lut.ctypes.data, g1.data_ptr(), 1, w * h))
        d1 = torch.empty_like(t)
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, g1.data_ptr(), w, h, levels, 1, d1.data_ptr(), 1, w * h))
        torch.cuda.synchronize()
        assert torch.equal(grids[i], g1), "frame %d %dx%d encode" % (i, w, h)
        assert torch.equal(back[i], d1), "frame %d %dx%d decode" % (i, w, h)
        del g1, d1


def test_error_cases(ctx, H):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    E = _ffi.EINVAL
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = a.data_ptr()
    lut = table(2, 0)
    shapes = [(16, 8), (10, 10)]
    assert call_list(ctx, False, [p, p + 256], [p + 1024, p + 2048], shapes, 4)[0] == _ffi.OK       # a valid call
    assert call_list(ctx, False, [p, p], [p + 1024, p + 2048], shapes, 4)[0] == _ffi.OK             # inputs may overlap
    assert L.hgi_decode_u8_list_dev(ctx.handle, None, None, None, 4, 1, None, 0) == _ffi.OK         # count == 0
    pi = (ctypes.c_void_p * 2)(p, p + 256)
    po = (ctypes.c_void_p * 2)(p + 1024, p + 2048)
    dims = (ctypes.c_uint32 * 2)(8, 8)
    assert L.hgi_decode_u8_list_dev(ctx.handle, pi, None, dims, 4, 1, po, 2) == E                   # NULL array
    assert L.hgi_decode_u8_list_dev(ctx.handle, None, dims, dims, 4, 1, po, 2) == E
    assert L.hgi_encode_u8_list_dev(ctx.handle, pi, dims, dims, 4, 1, None, po, 2) == E             # NULL lut
    assert call_list(ctx, False, [p, None], [p + 1024, p + 2048], shapes, 4)[0] == E                # NULL frame pointer
    assert call_list(ctx, False, [p, p + 256], [p + 1024, None], shapes, 4)[0] == E
    assert call_list(ctx, False, [p, None], [p + 1024, None], [(16, 8), (0, 7)], 4)[0] == _ffi.OK    # ... of an empty frame: fine
    assert call_list(ctx, False, [p, p + 256], [p + 1024, p + 2048], shapes, 32)[0] == E            # levels
    assert call_list(ctx, False, [p, p + 256], [p + 1024, p + 2048], shapes, 4, interp=5)[0] == _ffi.EUNSUPPORTED
    assert call_list(ctx, False, [p, p + 256], [p + 1024, p + 1100], shapes, 4)[0] == E             # outputs overlap
    assert call_list(ctx, False, [p, p + 256], [p + 1024, p + 100], shapes, 4)[0] == E              # output meets an input
    assert call_list(ctx, True, [p, p + 256], [p + 1024, p + 1024 + 127], shapes, 4, 1, lut)[0] == E
    assert call_list(ctx, True, [p, p + 256], [p + 1024, p + 256 + 99], shapes, 4, 1, lut)[0] == E
    assert call_list(ctx, False, [p, p + 256], [p, p + 2048], shapes, 4)[0] == E                    # in place
    big = [(65535, 65535)] * 4200                                                                   # more tiles than a launch holds
    assert call_list(ctx, False, [p] * 4200, [p + (1 << 40) + (i << 33) for i in range(4200)], big, 4)[0] == E
    assert b"tiles" in L.hgi_last_error()
    lw = H.Context(0)
    lw.set_path(_ffi.PATH_LEVELWISE)
    assert L.hgi_decode_u8_list_dev(lw.handle, pi, dims, dims, 4, 1, po, 2) == _ffi.EUNSUPPORTED
    lw.close()
    # a capturing stream is refused (a replay would read a table later calls overwrite)
    c = H.Context(0)
    side = torch.cuda.Stream()
    c.set_stream(side.cuda_stream)
    x = torch.zeros(16, device="cuda")
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            x.add_(1)
            st = L.hgi_decode_u8_list_dev(c.handle, pi, dims, dims, 4, 1, po, 2)
    assert st == _ffi.EUNSUPPORTED and b"captur" in L.hgi_last_error()
    torch.cuda.synchronize()
    c.close()


def test_ordering_without_syncs(ctx, H, oracle):
    """Back-to-back list calls (more than the ring has slots) with different lists, the host arrays overwritten right after each
    return, and a stream switch between calls: every output must still be right."""
    import torch
    from rustyhgi_amd import _ffi
    rng = np.random.default_rng(3)
    lists = []
    for r in range(7):
        shapes = [(int(rng.integers(1, 700)), int(rng.integers(1, 400))) for _ in range(int(rng.integers(1, 9)))]
        imgs = images(oracle, shapes, SEED0 + 100 + r)
        levels = (2, 4, 5, 6, 8)[r % 5]
        grids = [oracle.encode(f, levels, oracle.linear_lut(2)[0]) for f in imgs]
        lists.append((shapes, levels, grids, [oracle.decode(g, levels) for g in grids]))
    dev_in = [[torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in G] for _, _, G, _ in lists]
    dev_out = [[torch.full_like(g, SENT) for g in D] for D in dev_in]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for r, (shapes, levels, _, _) in enumerate(lists):
        if r == 4:
            ctx.set_stream(side.cuda_stream)          # hgi_ctx_set_stream between two list calls
        st, arrays = call_list(ctx, False, [t.data_ptr() for t in dev_in[r]], [t.data_ptr() for t in dev_out[r]], shapes, levels)
        assert st == _ffi.OK
        pi, po, ws, hs = arrays                       # overwritten at once: the call has copied what it needs
        for i in range(len(shapes)):
            pi[i] = po[i] = 0
            ws[i] = hs[i] = 0xFFFFFFFF
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for r, (shapes, levels, _, want) in enumerate(lists):
        for i, (o, wnt) in enumerate(zip(dev_out[r], want)):
            assert_same(o.cpu().numpy(), wnt, "list %d frame %d L%d" % (r, i, levels))


def test_python_torch_and_numpy_surfaces(H, oracle, lena):
    import torch
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    from rustyhgi_amd.quantizator import Linear, QuantizationLevel
    imgs = images(oracle, SHAPES[:6], SEED0 + 9) + [lena, np.zeros((0, 5), np.uint8)]
    for interp, I in ((1, Crossed), (0, LeftTop)):
        for levels in (3, 7, 10):
            enc = H.Encoder(I(), Linear.from_level(QuantizationLevel.High), levels)
            dec = H.Decoder(I())
            lut = oracle.linear_lut(3)[0]
            want_g = [oracle.encode(f, levels, lut, interp) if f.size else f for f in imgs]
            want_i = [oracle.decode(g, levels, interp) if g.size else g for g in want_g]
            tg = enc.encode_list([torch.from_numpy(f).cuda() for f in imgs])
            assert len(tg) == len(imgs) and all(t.is_cuda and tuple(t.shape) == f.shape for t, f in zip(tg, imgs))
            assert len({t.untyped_storage().data_ptr() for t in tg}) == 1, "the outputs are views into one allocation"
            ti = dec.decode_list(tg, levels)
            torch.cuda.synchronize()
            for i in range(len(imgs)):
                assert_same(tg[i].cpu().numpy(), want_g[i], "torch encode %d L%d" % (i, levels))
                assert_same(ti[i].cpu().numpy(), want_i[i], "torch decode %d L%d" % (i, levels))
            out = [torch.full(t.shape, SENT, dtype=torch.uint8, device="cuda") for t in tg]
            r = dec.decode_list(tg, levels, out=out)
            torch.cuda.synchronize()
            assert all(a is b for a, b in zip(r, out))
            for i in range(len(imgs)):
                assert_same(out[i].cpu().numpy(), want_i[i], "torch out= %d" % i)
            ng = enc.encode_list(imgs)
            ni = dec.decode_list(ng, levels)
            for i in range(len(imgs)):
                assert isinstance(ng[i], np.ndarray)
                assert_same(ng[i], want_g[i], "numpy encode %d" % i)
                assert_same(ni[i], want_i[i], "numpy decode %d" % i)


def test_forced_checked_path_in_a_child_process():
    """The knobs build with HGI_FORCE_CHECKED=1 (every tile through the byte-checked path) re-runs the shape and layout cases: the
    bytes must not change."""
    from rustyhgi_amd import _ffi
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs)
    env = dict(os.environ, HGI_LIB_PATH=knobs, HGI_FORCE_CHECKED="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_framelist_gpu.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "assorted_shapes and (d01 or d04 or d07 or d09) or layouts"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


def _time(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / reps)
    return min(best)


@pytest.mark.perf
def test_list_call_beats_the_per_frame_loop(ctx):
    """Loose guards (targets: DESIGN.md 4.8, profiles/r07_framelist.txt): W1, 1024 frames of sides drawn from [64, 2048], at least
    3x faster than the per-frame loop of the uniform call; W3, the 64 x 4096^2 shard as 64 pointers, at most 1.3x the uniform call."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    lut = table(2, 0)
    rng = np.random.default_rng(SEED0)
    for name, shapes in (("W1", [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]), ("W3", [(4096, 4096)] * 64)):
        offs, at = [], 0
        for w, h in shapes:
            offs.append(at)
            at += (w * h + 255) // 256 * 256
        src = torch.empty(at, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED0, 0, at, 1, src.data_ptr(), 1, at))
        n = len(shapes)
        pi = (ctypes.c_void_p * n)(*[src.data_ptr() + o for o in offs])
        po = (ctypes.c_void_p * n)(*[dst.data_ptr() + o for o in offs])
        ws = (ctypes.c_uint32 * n)(*[w for w, h in shapes])
        hs = (ctypes.c_uint32 * n)(*[h for w, h in shapes])
        t_list = _time(lambda: _ffi.check(L.hgi_decode_u8_list_dev(ctx.handle, pi, ws, hs, 4, 1, po, n)))
        if name == "W1":
            t_ref = _time(lambda: [_ffi.check(L.hgi_decode_u8_dev(ctx.handle, pi[i], ws[i], hs[i], 4, 1, po[i], 1, ws[i] * hs[i]))
                                   for i in range(n)])
            print("W1 decode: list %.3f ms, loop %.3f ms (%.1fx)" % (t_list, t_ref, t_ref / t_list))
            assert t_ref >= 3 * t_list, (t_list, t_ref)
        else:
            t_ref = _time(lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, src.data_ptr(), 4096, 4096, 4, 1, dst.data_ptr(), 64, 4096 * 4096)))
            print("W3 decode: list %.3f ms, uniform %.3f ms (%.3fx)" % (t_list, t_ref, t_list / t_ref))
            assert t_list <= 1.3 * t_ref, (t_list, t_ref)
        del src, dst
        torch.cuda.empty_cache()
