"""GPU suite of scaled decode: every shape, depth, shift and layout must give the stride-2^s lattice of the full decode, bit for
bit, and nothing outside the sw x sh output frames may be written.  Expected bytes: oracle.decode(grid, levels)[::S, ::S], or --
where the oracle is too slow -- the library's own hgi_decode_u8_dev output sliced the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEED0

pytestmark = pytest.mark.gpu
SENT = 0xC3


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


def ssize(w, h, s):
    return -(-w >> s), -(-h >> s)


def assert_same(a, b, what):
    if a.shape != b.shape or not (a == b).all():
        if a.shape != b.shape:
            raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def scaled_dev(ctx, grids, w, h, levels, shift, interp=1, pitch=None, ostride=None, lead=0, frame_stride=None):
    """hgi_decode_scaled_u8_dev on the (B, ...) device grids into a sentinel-filled buffer with the given layout; returns the
    (B, sh, sw) frames and checks that every other byte is still the sentinel."""
    import torch
    from rustyhgi_amd import _ffi
    sw, sh = ssize(w, h, shift)
    B = grids.shape[0]
    pitch = pitch or sw
    span = (sh - 1) * pitch + sw
    ostride = ostride or span
    total = lead + (B - 1) * ostride + span + 64
    buf = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    fs = frame_stride or w * h
    _ffi.check(_ffi.lib().hgi_decode_scaled_u8_dev(ctx.handle, grids.data_ptr(), w, h, levels, interp, shift, buf.data_ptr() + lead,
                                                   pitch, B, fs, ostride))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    mask = np.zeros(total, bool)
    outs = []
    for f in range(B):
        idx = lead + f * ostride + (np.arange(sh)[:, None] * pitch + np.arange(sw)[None, :])
        mask[idx] = True
        outs.append(host[idx])
    stray = np.nonzero(host[~mask] != SENT)[0]
    assert len(stray) == 0, "%dx%d L%d s%d pitch %d: %d bytes outside the output frames written" % (w, h, levels, shift, pitch, len(stray))
    return np.stack(outs)


def full_dev(ctx, g, w, h, levels, interp=1):
    """The library's whole decode of the (B, h, w) device grids (what the scaled call must sample)."""
    import torch
    from rustyhgi_amd import _ffi
    out = torch.empty_like(g)
    _ffi.check(_ffi.lib().hgi_decode_u8_dev(ctx.handle, g.data_ptr(), w, h, levels, interp, out.data_ptr(), g.shape[0], w * h))
    torch.cuda.synchronize()
    return out


def shifts(levels):
    return list(range(levels + 3)) + [31]


def check_all_shifts(ctx, grid, levels, interp, want_full, what, lshifts=None):
    """grid: (h, w) numpy; want_full: the full decode.  Every shift, the layout varied along the list."""
    import torch
    h, w = grid.shape
    g = torch.from_numpy(np.ascontiguousarray(grid)).cuda()[None]
    for i, s in enumerate(lshifts or shifts(levels)):
        sw, sh = ssize(w, h, s)
        got = scaled_dev(ctx, g, w, h, levels, s, interp, pitch=sw + (0, 1, 13, 64)[i % 4], lead=(0, 1, 3, 16)[i % 4])
        S = 1 << s
        assert_same(got[0], want_full[::S, ::S], "%s %dx%d L%d i%d s%d" % (what, w, h, levels, interp, s))
    assert (g[0].cpu().numpy() == grid).all(), "the grid was modified"


SMALL = [(1, 1), (1, 37), (37, 1), (127, 5), (128, 64), (129, 65), (5, 127), (64, 128), (65, 129), (255, 257), (257, 255), (300, 1)]


@pytest.mark.parametrize("w,h", SMALL)
def test_small_shapes_every_depth_and_shift_against_the_oracle(ctx, oracle, w, h):
    rng = np.random.default_rng(SEED0 + 7 * w + h)
    for levels in range(13):
        for interp in (1, 0):
            grid = rng.integers(0, 256, (h, w), dtype=np.uint8)        # raw noise: every byte string is a grid
            check_all_shifts(ctx, grid, levels, interp, oracle.decode(grid, levels, interp), "noise")


@pytest.mark.parametrize("levels", list(range(13)))
def test_lena_every_shift_both_interpolators(ctx, oracle, lena, levels):
    for interp in (1, 0):
        for q in (2, "rand"):
            lut = oracle.linear_lut(2)[0] if q == 2 else np.random.default_rng(levels).integers(0, 256, 256, dtype=np.uint8)
            grid = oracle.encode(lena, levels, lut, interp)
            check_all_shifts(ctx, grid, levels, interp, oracle.decode(grid, levels, interp), "lena q%s" % q)


def test_fullhd_both_luma_readings(ctx, oracle, fullhd, fullhd709):
    for img, name in ((fullhd, "fullhd"), (fullhd709, "fullhd709")):
        for levels in (4, 8, 10):
            grid = oracle.encode(img, levels, oracle.linear_lut(2)[0])
            check_all_shifts(ctx, grid, levels, 1, oracle.decode(grid, levels), name)


@pytest.mark.parametrize("w,h", [(1960, 1960), (2368, 2614), (4097, 4097)])
def test_large_shapes_against_the_full_decode(ctx, w, h):
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED0 + w)
    for levels in (0, 1, 3, 4, 6, 8, 9, 12):
        for interp in (1, 0):
            g = torch.randint(0, 256, (1, h, w), dtype=torch.uint8, device="cuda", generator=gen)
            full = full_dev(ctx, g, w, h, levels, interp)[0].cpu().numpy()
            check_all_shifts(ctx, g[0].cpu().numpy(), levels, interp, full, "noise",
                             lshifts=[s for s in shifts(levels) if s <= 4 or s >= levels or s == 31])


def test_batch_layouts(ctx, oracle):
    """Three frames with frame_stride > w*h; out_pitch > sw, odd pitches, an unaligned output, out_frame_stride beyond the span."""
    import torch
    w, h, levels = 1001, 333, 7
    fs = w * h + 77
    host = np.full((3, fs), 0x11, np.uint8)
    wants = []
    rng = np.random.default_rng(SEED0 + 3)
    for f in range(3):
        grid = rng.integers(0, 256, (h, w), dtype=np.uint8)
        host[f, :w * h] = grid.reshape(-1)
        wants.append(oracle.decode(grid, levels))
    g = torch.from_numpy(host).cuda()
    for s in (0, 1, 2, 3, 5, 7, 8, 31):
        sw, sh = ssize(w, h, s)
        for pitch, lead, extra in ((sw, 0, 0), (sw + 1, 1, 5), (sw + 33, 7, 1000)):
            span = (sh - 1) * pitch + sw
            got = scaled_dev(ctx, g, w, h, levels, s, pitch=pitch, ostride=span + extra, lead=lead, frame_stride=fs)
            for f in range(3):
                assert_same(got[f], wants[f][::1 << s, ::1 << s], "batch frame %d s%d pitch %d" % (f, s, pitch))
    assert (g.cpu().numpy() == host).all()


def test_host_call_equals_device_call(H, ctx, oracle):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(SEED0 + 9)
    for (w, h) in ((1001, 999), (130, 33), (4096, 17), (3, 3000)):
        for levels in (2, 5, 9):
            grid = rng.integers(0, 256, (h, w), dtype=np.uint8)
            g = torch.from_numpy(grid).cuda()[None]
            for s in range(levels + 2):
                sw, sh = ssize(w, h, s)
                out = np.full((sh, sw + 3), SENT, np.uint8)
                _ffi.check(L.hgi_decode_scaled_u8(ctx.handle, grid.ctypes.data, w, h, levels, 1, s, out.ctypes.data, sw + 3))
                assert (out[:, sw:] == SENT).all()
                dev = scaled_dev(ctx, g, w, h, levels, s)[0]
                assert_same(out[:, :sw], dev, "host %dx%d L%d s%d" % (w, h, levels, s))


def test_error_cases(H, ctx):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h = 300, 200
    g = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    o = torch.full((2 * w * h,), SENT, dtype=torch.uint8, device="cuda")
    gp, op = g.data_ptr(), o.data_ptr()

    def call(**k):
        a = dict(grid=gp, w=w, h=h, levels=4, interp=1, shift=2, out=op, pitch=75, batch=1, fs=w * h, ofs=75 * 50, c=ctx.handle)
        a.update(k)
        return L.hgi_decode_scaled_u8_dev(a["c"], a["grid"], a["w"], a["h"], a["levels"], a["interp"], a["shift"], a["out"], a["pitch"],
                                          a["batch"], a["fs"], a["ofs"])
    E = _ffi.EINVAL
    assert call() == _ffi.OK
    assert call(shift=32) == E and call(pitch=74) == E and call(shift=3, pitch=37) == E and call(shift=3, pitch=38) == _ffi.OK
    assert call(batch=2, fs=w * h - 1) == E
    assert call(batch=2, ofs=49 * 75 + 74) == E and call(batch=2, ofs=49 * 75 + 75) == _ffi.OK
    assert call(out=gp + 5) == E and call(out=gp - 50) == E
    assert call(batch=2, out=gp + 2 * w * h - 50) == E
    assert call(grid=0) == E and call(out=0) == E
    assert call(levels=32) == E and call(interp=7) == _ffi.EUNSUPPORTED and call(c=None) == E
    torch.cuda.synchronize()
    o.fill_(SENT)
    torch.cuda.synchronize()
    assert call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    torch.cuda.synchronize()
    assert (o == SENT).all()
    lw = H.Context(0)
    lw.set_path(_ffi.PATH_LEVELWISE)
    assert call(c=lw.handle) == _ffi.EUNSUPPORTED and b"LEVELWISE" in L.hgi_last_error()
    lw.close()
    gh = np.zeros((h, w), np.uint8)
    oh = np.zeros(w * h, np.uint8)
    assert L.hgi_decode_scaled_u8(ctx.handle, gh.ctypes.data, w, h, 4, 1, 32, oh.ctypes.data, 10) == E
    assert L.hgi_decode_scaled_u8(ctx.handle, gh.ctypes.data, w, h, 4, 1, 1, oh.ctypes.data, 149) == E
    assert L.hgi_decode_scaled_u8(ctx.handle, gh.ctypes.data, w, h, 4, 9, 1, oh.ctypes.data, 150) == _ffi.EUNSUPPORTED


def test_reserved_ctx_does_not_grow_and_graph_replay(H, oracle):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h, B = 1300, 700, 2
    rng = np.random.default_rng(SEED0 + 11)
    for levels in (4, 8, 12):
        c = H.Context(0)
        _ffi.check(L.hgi_ctx_reserve(c.handle, w, h, levels, B))
        before = c.scratch_bytes()
        grids = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
        g = torch.from_numpy(grids).cuda()
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        want = [oracle.decode(grids[f], levels) for f in range(B)]
        for s in range(levels + 2):
            sw, sh = ssize(w, h, s)
            out = torch.empty((B, sh, sw), dtype=torch.uint8, device="cuda")
            _ffi.check(L.hgi_decode_scaled_u8_dev(c.handle, g.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B, w * h, sw * sh))
            ho = np.empty((sh, sw), np.uint8)
            _ffi.check(L.hgi_decode_scaled_u8(c.handle, grids[1].ctypes.data, w, h, levels, 1, s, ho.ctypes.data, sw))
            torch.cuda.synchronize()
            assert c.scratch_bytes() == before, "L%d s%d: %d -> %d" % (levels, s, before, c.scratch_bytes())
            for f in range(B):
                assert_same(out[f].cpu().numpy(), want[f][::1 << s, ::1 << s], "reserved L%d s%d frame %d" % (levels, s, f))
            assert_same(ho, want[1][::1 << s, ::1 << s], "reserved host L%d s%d" % (levels, s))
        if levels == 12:       # captured into a graph on one stream and replayed on new grids
            s = 1
            sw, sh = ssize(w, h, s)
            out = torch.zeros((B, sh, sw), dtype=torch.uint8, device="cuda")
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                c.set_stream(side.cuda_stream)
                gr = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(gr, stream=side):
                    _ffi.check(L.hgi_decode_scaled_u8_dev(c.handle, g.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B, w * h, sw * sh))
            grids2 = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
            g.copy_(torch.from_numpy(grids2).cuda())
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            for f in range(B):
                assert_same(out[f].cpu().numpy(), oracle.decode(grids2[f], levels)[::2, ::2], "graph replay frame %d" % f)
            assert c.scratch_bytes() == before
        c.close()


def _synth_grids(ctx, w, h, B, levels, seed):
    import torch
    from rustyhgi_amd import _ffi
    grid = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
    _ffi.check(_ffi.lib().hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, seed, 0, w, h, grid.data_ptr(), B, w * h))
    return grid


def test_batch_scale_c3_and_c4_against_the_sliced_full_decode(ctx):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    for (w, h, B, levels, ss) in ((4096, 4096, 64, 4, (1, 2, 3)), (16384, 16384, 1, 8, (1, 4))):
        grid = _synth_grids(ctx, w, h, B, levels, SEED0 + 21)
        full = full_dev(ctx, grid, w, h, levels)
        for s in ss:
            sw, sh = ssize(w, h, s)
            out = torch.full((B, sh, sw), SENT, dtype=torch.uint8, device="cuda")
            _ffi.check(L.hgi_decode_scaled_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B, w * h, sw * sh))
            torch.cuda.synchronize()
            S = 1 << s
            assert torch.equal(out, full[:, ::S, ::S]), "%d x %d^2 L%d s%d" % (B, w, levels, s)
        del grid, full
        torch.cuda.empty_cache()


def test_python_numpy_torch_and_batch_surfaces(H, oracle, lena):
    import torch
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    for interp, I in ((1, Crossed), (0, LeftTop)):
        dec = H.Decoder(I())
        for levels in (4, 7, 10):
            grid = oracle.encode(lena, levels, oracle.linear_lut(1)[0], interp)
            full = oracle.decode(grid, levels, interp)
            for s in (0, 1, 3, levels + 1):
                S = 1 << s
                got = dec.decode_scaled((256, 256), levels, grid, s)
                assert isinstance(got, np.ndarray) and got.shape == full[::S, ::S].shape
                assert_same(got, full[::S, ::S], "numpy L%d s%d" % (levels, s))
                tg = torch.from_numpy(grid).cuda()
                got = dec.decode_scaled((256, 256), levels, tg, s)
                assert torch.is_tensor(got) and got.is_cuda
                assert_same(got.cpu().numpy(), full[::S, ::S], "torch L%d s%d" % (levels, s))
                stack = torch.stack([tg, torch.from_numpy(oracle.encode(lena[::-1].copy(), levels, oracle.linear_lut(1)[0], interp)).cuda()])
                sw, sh = ssize(256, 256, s)
                out = torch.full((2, sh, sw), SENT, dtype=torch.uint8, device="cuda")
                r = dec.decode_scaled_batch(stack, levels, s, out=out)
                torch.cuda.synchronize()
                assert r is out
                assert_same(out[0].cpu().numpy(), full[::S, ::S], "batch frame 0")
                assert_same(out[1].cpu().numpy(), oracle.decode(stack[1].cpu().numpy(), levels, interp)[::S, ::S], "batch frame 1")
                nb = dec.decode_scaled_batch(stack.cpu().numpy(), levels, s)
                assert (nb == out.cpu().numpy()).all()


def test_cli_scale_equals_the_python_call(H, oracle, lena, tmp_path):
    exe = str(tmp_path / "hgi")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "cli", "hgi_cli.cpp"),
                           "-L", os.path.join(ROOT, "rustyhgi_amd"), "-lhgi_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "rustyhgi_amd"),
                           "-o", exe])
    img = lena[:, :201].copy()       # 201 x 256: a ragged width
    with open(str(tmp_path / "in.pgm"), "wb") as f:
        f.write(b"P5\n201 256\n255\n" + img.tobytes())
    run = lambda *a: subprocess.run([exe] + list(a), cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    r = run("encode", "-i", "in.pgm", "-o", "a.hgi", "-l", "5")
    assert r.returncode == 0, r.stderr
    from rustyhgi_amd import Archive
    from rustyhgi_amd.interpolator import Crossed
    with open(str(tmp_path / "a.hgi"), "rb") as f:
        arc = Archive.deserialize_from_reader(f)
    want = H.Decoder(Crossed()).decode_scaled((201, 256), 5, arc.grid, 2)
    for n, s in (("4", 2), ("1", 0), ("2147483648", 31)):
        r = run("decode", "-i", "a.hgi", "-o", "s.pgm", "--scale", n)
        assert r.returncode == 0, r.stderr
        sw, sh = ssize(201, 256, s)
        data = open(str(tmp_path / "s.pgm"), "rb").read()
        head = ("P5\n%d %d\n255\n" % (sw, sh)).encode()
        assert data.startswith(head)
        got = np.frombuffer(data[len(head):], np.uint8).reshape(sh, sw)
        if s == 2:
            assert_same(got, want, "cli --scale 4")
    for bad in (("--scale", "3"), ("--scale", "0"), ("--scale", "-4"), ("--scale", "4294967296"), ("--scale", "x"),
                ("--scale", "2", "--region", "0,0,8,8")):
        r = run("decode", "-i", "a.hgi", "-o", "bad.pgm", *bad)
        assert r.returncode != 0 and "scale" in r.stderr, (bad, r.stderr)


FORCED_MODES = ["HGI_FORCE_CHECKED=1", "HGI_NO_LATTICE_KERNEL=1", "HGI_NO_LATTICE_KERNEL=1,HGI_FORCE_CHECKED=1"]


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """The knobs build re-runs the shape-heavy cases with the byte-checked path and / or the host recursion for the lattice plane
    forced: the bytes must not change."""
    from rustyhgi_amd import _ffi
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs)
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_scaled_gpu.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "lena_every_shift or batch_layouts or host_call_equals"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]


def _time(fn, reps=20):
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
def test_scaled_cost_guard(ctx):
    """Loose guards (targets: DESIGN.md 4.7, profiles/r06_scaled.txt) on 64 x 4096^2 L4: s = 1 <= 0.55 x the whole-batch decode,
    s = 2 <= 0.30 x; s = 1 faster than the composed route (torch's strided gather + hgi_decode_u8_dev on levels - 1)."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w = h = 4096
    B, levels = 64, 4
    grid = _synth_grids(ctx, w, h, B, levels, SEED0 + 31)
    full = torch.empty_like(grid)
    t_full = _time(lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, full.data_ptr(), B, w * h)))
    t = {}
    for s, bound in ((1, 0.55), (2, 0.30)):
        sw, sh = ssize(w, h, s)
        out = torch.empty((B, sh, sw), dtype=torch.uint8, device="cuda")
        t[s] = _time(lambda: _ffi.check(L.hgi_decode_scaled_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B,
                                                                   w * h, sw * sh)))
        torch.cuda.synchronize()
        assert torch.equal(out, full[:, ::1 << s, ::1 << s])
        print("64 x 4096^2 L4 s%d: %.1f us of %.1f us (%.3f)" % (s, t[s] * 1e3, t_full * 1e3, t[s] / t_full))
        assert t[s] <= bound * t_full, (s, t[s], t_full)
    sub = torch.empty((B, 2048, 2048), dtype=torch.uint8, device="cuda")
    comp = torch.empty_like(sub)

    def composed():
        sub.copy_(grid[:, ::2, ::2])
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, sub.data_ptr(), 2048, 2048, levels - 1, 1, comp.data_ptr(), B, 2048 * 2048))
    t_comp = _time(composed)
    torch.cuda.synchronize()
    assert torch.equal(comp, full[:, ::2, ::2])
    print("composed route s1: %.1f us; fused %.1f us (%.3f)" % (t_comp * 1e3, t[1] * 1e3, t[1] / t_comp))
    assert t[1] < t_comp, (t[1], t_comp)
