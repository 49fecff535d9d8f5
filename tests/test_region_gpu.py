"""GPU suite of region decode: every window of every shape, depth and layout must be the crop of the full decode, bit for bit,
and nothing outside the window may be written.  Expected bytes: oracle.decode(grid)[y0:y0+h, x0:x0+w], or -- where the oracle
is too slow -- the crop of the library's own hgi_decode_u8_dev."""
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


def assert_same(a, b, what):
    if a.shape != b.shape or not (a == b).all():
        if a.shape != b.shape:
            raise AssertionError("%s: shape %s, want %s" % (what, a.shape, b.shape))
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def grid_of(oracle, w, h, levels, q, kind, frame=0, seed=SEED0 + 50):
    lut = oracle.linear_lut(q)[0] if q != "rand" else None
    img = oracle.synth(kind, seed, frame, w, h)
    if q == "rand":        # a random (non-monotone) table
        lut = np.random.default_rng(seed + w * 7 + h).integers(0, 256, 256, dtype=np.uint8)
    return oracle.encode(img, levels, lut)


def windows(w, h, n_random, seed):
    """The full frame, 1x1 at both corners, tile-aligned, straddling 128/64 tile and 16-B chunk borders with widths 1..17, touching
    the right and bottom edges, and seeded random ones."""
    r = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1)]
    if w >= 256 and h >= 128:
        r += [(128, 64, 128, 64), (0, 0, 128, 64), (128, 0, min(256, w - 128), min(128, h))]
    for ww in range(1, 18):
        for x in (127 - ww // 2, 15 - ww // 2 + 16, 113):
            x = max(0, min(x, w - ww))
            y = max(0, min(63 - ww // 3, h - 3))
            if x + ww <= w and y + 3 <= h:
                r.append((x, y, ww, min(3 + ww % 5, h - y)))
    r.append((max(0, w - 37), max(0, h - 5), min(37, w), min(5, h)))     # touches the right and bottom edges
    r.append((max(0, w - 200), max(0, h - 70), min(200, w), min(70, h)))
    rng = np.random.default_rng(seed)
    for _ in range(n_random):
        rw = int(rng.integers(1, w + 1)) if rng.random() < 0.3 else int(rng.integers(1, min(w, 300) + 1))
        rh = int(rng.integers(1, h + 1)) if rng.random() < 0.3 else int(rng.integers(1, min(h, 150) + 1))
        r.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    return r


def region_dev(ctx, grids, w, h, levels, rect, interp=1, pitch=None, ostride=None, lead=0, frame_stride=None):
    """Runs hgi_decode_region_u8_dev on the (B, ...) device grids into a sentinel-filled buffer with the given layout; returns the
    (B, rh, rw) windows and checks that every other byte is still the sentinel."""
    import torch
    from rustyhgi_amd import _ffi
    x0, y0, rw, rh = rect
    B = grids.shape[0]
    pitch = pitch or rw
    span = (rh - 1) * pitch + rw
    ostride = ostride or span
    total = lead + (B - 1) * ostride + span + 64
    buf = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    fs = frame_stride or w * h
    _ffi.check(_ffi.lib().hgi_decode_region_u8_dev(ctx.handle, grids.data_ptr(), w, h, levels, interp, x0, y0, rw, rh,
                                                   buf.data_ptr() + lead, pitch, B, fs, ostride))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    mask = np.zeros(total, bool)
    outs = []
    for f in range(B):
        base = lead + f * ostride
        idx = base + (np.arange(rh)[:, None] * pitch + np.arange(rw)[None, :])
        mask[idx] = True
        outs.append(host[idx])
    stray = np.nonzero(host[~mask] != SENT)[0]
    assert len(stray) == 0, "region %r pitch %d: %d bytes outside the windows written" % (rect, pitch, len(stray))
    return np.stack(outs)


def check_windows(ctx, oracle, grid, levels, rects, interp=1, what="", full=None):
    import torch
    h, w = grid.shape
    want = oracle.decode(grid, levels, interp) if full is None else full
    g = torch.from_numpy(np.ascontiguousarray(grid)).cuda()[None]
    for i, r in enumerate(rects):
        x0, y0, rw, rh = r
        # vary the layout along the list: odd pitch, wider pitch, unaligned output
        pitch = rw + (0, 1, 13, 64)[i % 4]
        got = region_dev(ctx, g, w, h, levels, r, interp, pitch=pitch, lead=(0, 1, 3, 16)[i % 4])
        assert_same(got[0], want[y0:y0 + rh, x0:x0 + rw], "%s %dx%d L%d i%d window %r" % (what, w, h, levels, interp, r))
    assert (g[0].cpu().numpy() == grid).all(), "the grid was modified"


@pytest.mark.parametrize("levels", [0, 1, 3, 4, 5, 6, 7, 8, 9, 13, 31])
def test_lena_all_depths_both_interpolators(ctx, oracle, lena, levels):
    for interp in (1, 0):
        for q in (2, "rand"):
            lut = oracle.linear_lut(2)[0] if q == 2 else np.random.default_rng(levels).integers(0, 256, 256, dtype=np.uint8)
            grid = oracle.encode(lena, levels, lut, interp)
            check_windows(ctx, oracle, grid, levels, windows(256, 256, 12, SEED0 + levels), interp, "lena q%s" % q)


def test_fullhd_both_luma_readings(ctx, oracle, fullhd, fullhd709):
    for img, name in ((fullhd, "fullhd"), (fullhd709, "fullhd709")):
        for levels in (4, 8):
            grid = oracle.encode(img, levels, oracle.linear_lut(2)[0])
            check_windows(ctx, oracle, grid, levels, windows(1920, 1080, 50, SEED0 + levels), 1, name)


@pytest.mark.parametrize("w,h,levels", [(1001, 999, 4), (1001, 999, 7), (13, 7, 3), (13, 7, 7), (130, 33, 7), (130, 33, 2),
                                        (2048, 2048, 9), (2048, 2048, 12), (2048, 2048, 31), (704, 300, 13), (1001, 999, 9)])
def test_ragged_and_deep_shapes(ctx, oracle, w, h, levels):
    for q, kind in ((3, oracle.SYNTH_NOISE), ("rand", oracle.SYNTH_RAMP)):
        grid = grid_of(oracle, w, h, levels, q, kind)
        check_windows(ctx, oracle, grid, levels, windows(w, h, 50, SEED0 + w + levels), 1, "q%s" % q)


def test_batch_layouts(ctx, oracle):
    """Three frames with frame_stride > w*h, out_pitch > w, an odd pitch, an unaligned output, out_frame_stride beyond the span."""
    import torch
    w, h, levels = 1001, 333, 7
    fs = w * h + 77
    host = np.full((3, fs), 0x11, np.uint8)
    wants = []
    for f in range(3):
        grid = grid_of(oracle, w, h, levels, 2, oracle.SYNTH_NOISE, frame=f)
        host[f, :w * h] = grid.reshape(-1)
        wants.append(oracle.decode(grid, levels))
    g = torch.from_numpy(host).cuda()
    for rect in [(0, 0, w, h), (130, 70, 400, 200), (999, 5, 2, 300), (3, 331, 700, 2)]:
        x0, y0, rw, rh = rect
        for pitch, lead, extra in ((rw, 0, 0), (rw + 1, 1, 5), (rw + 33, 7, 1000)):
            span = (rh - 1) * pitch + rw
            got = region_dev(ctx, g, w, h, levels, rect, pitch=pitch, ostride=span + extra, lead=lead, frame_stride=fs)
            for f in range(3):
                assert_same(got[f], wants[f][y0:y0 + rh, x0:x0 + rw], "batch frame %d %r pitch %d" % (f, rect, pitch))
    assert (g.cpu().numpy() == host).all()


def test_c4_frame_windows_against_the_full_decode(ctx, oracle):
    """BASELINE C4: a 16384^2 level-8 High frame; 20 random windows against the crop of the library's full decode."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w = h = 16384
    src = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
    _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_RAMP, SEED0 + 4, 0, w, h, src.data_ptr(), 1, w * h))
    lut = oracle.linear_lut(3)[0]
    grid = torch.empty_like(src)
    full = torch.empty_like(src)
    _ffi.check(L.hgi_encode_u8_dev(ctx.handle, src.data_ptr(), w, h, 8, 1, lut.ctypes.data, grid.data_ptr(), 1, w * h))
    _ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, 8, 1, full.data_ptr(), 1, w * h))
    torch.cuda.synchronize()
    rng = np.random.default_rng(SEED0 + 4)
    rects = [(5001, 7003, 1920, 1080), (w - 1920, h - 1080, 1920, 1080)]
    for _ in range(18):
        rw, rh = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
        rects.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    for i, (x0, y0, rw, rh) in enumerate(rects):
        out = torch.full((rh, rw + i % 3), SENT, dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_decode_region_u8_dev(ctx.handle, grid.data_ptr(), w, h, 8, 1, x0, y0, rw, rh, out.data_ptr(), rw + i % 3, 1, w * h, 0))
        want = full[0, y0:y0 + rh, x0:x0 + rw]
        assert torch.equal(out[:, :rw], want), "C4 window %r" % ((x0, y0, rw, rh),)
        if i % 3:
            assert (out[:, rw:] == SENT).all()


def test_error_cases(H, ctx):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h = 300, 200
    g = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    o = torch.full((2 * w * h,), SENT, dtype=torch.uint8, device="cuda")
    gp, op = g.data_ptr(), o.data_ptr()

    def call(*a, **k):
        args = dict(grid=gp, w=w, h=h, levels=4, interp=1, x0=0, y0=0, rw=10, rh=10, out=op, pitch=10, batch=1, fs=w * h, ofs=100, c=ctx.handle)
        args.update(k)
        return L.hgi_decode_region_u8_dev(args["c"], args["grid"], args["w"], args["h"], args["levels"], args["interp"], args["x0"],
                                          args["y0"], args["rw"], args["rh"], args["out"], args["pitch"], args["batch"], args["fs"], args["ofs"])
    E = _ffi.EINVAL
    assert call() == _ffi.OK
    assert call(x0=291) == E and call(y0=191) == E and call(x0=2 ** 32 - 1) == E and call(y0=2 ** 32 - 5, rh=10) == E
    assert call(rw=2 ** 32 - 1, x0=1) == E
    assert call(pitch=9) == E
    assert call(batch=2, fs=w * h - 1) == E
    assert call(batch=2, ofs=9 * 10 + 9) == E and call(batch=2, ofs=9 * 10 + 10) == _ffi.OK
    assert call(out=gp + 5) == E                               # output inside the grid
    assert call(out=gp - 50) == E                              # output span runs into the grid
    assert call(batch=2, out=gp + 2 * w * h - 50, ofs=100) == E
    assert call(grid=0) == E and call(out=0) == E
    assert call(levels=32) == E
    assert call(interp=7) == _ffi.EUNSUPPORTED
    assert call(c=None) == E
    torch.cuda.synchronize()
    o.fill_(SENT)
    torch.cuda.synchronize()
    # empty calls succeed and write nothing
    assert call(rw=0) == _ffi.OK and call(rh=0) == _ffi.OK and call(batch=0) == _ffi.OK and call(w=0) == _ffi.OK and call(h=0) == _ffi.OK
    assert call(rw=0, x0=300) == _ffi.OK
    torch.cuda.synchronize()
    assert (o == SENT).all()
    lw = H.Context(0)
    lw.set_path(_ffi.PATH_LEVELWISE)
    assert call(c=lw.handle) == _ffi.EUNSUPPORTED and b"LEVELWISE" in L.hgi_last_error()
    lw.close()
    gh = np.zeros((h, w), np.uint8)
    oh = np.zeros(100, np.uint8)
    assert L.hgi_decode_region_u8(ctx.handle, gh.ctypes.data, w, h, 4, 1, 295, 0, 10, 10, oh.ctypes.data, 10) == E
    assert L.hgi_decode_region_u8(ctx.handle, gh.ctypes.data, w, h, 4, 1, 0, 0, 10, 10, oh.ctypes.data, 9) == E
    assert L.hgi_decode_region_u8(ctx.handle, gh.ctypes.data, w, h, 4, 9, 0, 0, 10, 10, oh.ctypes.data, 10) == _ffi.EUNSUPPORTED


def test_reserved_ctx_does_not_grow_and_graph_replay(H, oracle):
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    w, h, B = 1300, 700, 2
    for levels in (4, 8, 12):
        c = H.Context(0)
        _ffi.check(L.hgi_ctx_reserve(c.handle, w, h, levels, B))
        before = c.scratch_bytes()
        grids = np.stack([grid_of(oracle, w, h, levels, 2, oracle.SYNTH_NOISE, frame=f) for f in range(B)])
        g = torch.from_numpy(grids).cuda()
        out = torch.empty((B, 300, 500), dtype=torch.uint8, device="cuda")
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        for rect in [(0, 0, 500, 300), (799, 399, 500, 300), (131, 67, 500, 300)]:
            _ffi.check(L.hgi_decode_region_u8_dev(c.handle, g.data_ptr(), w, h, levels, 1, *rect, out.data_ptr(), 500, B, w * h, 500 * 300))
        torch.cuda.synchronize()
        assert c.scratch_bytes() == before, "L%d: %d -> %d" % (levels, before, c.scratch_bytes())
        want = [oracle.decode(grids[f], levels) for f in range(B)]
        for f in range(B):
            assert_same(out[f].cpu().numpy(), want[f][67:367, 131:631], "reserved L%d frame %d" % (levels, f))
        if levels == 12:       # captured into a graph and replayed on new grids
            side = torch.cuda.Stream()
            out.zero_()
            with torch.cuda.stream(side):
                c.set_stream(side.cuda_stream)
                gr = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(gr, stream=side):
                    _ffi.check(L.hgi_decode_region_u8_dev(c.handle, g.data_ptr(), w, h, levels, 1, 257, 129, 500, 300, out.data_ptr(), 500,
                                                          B, w * h, 500 * 300))
            grids2 = np.stack([grid_of(oracle, w, h, levels, 3, oracle.SYNTH_RAMP, frame=f, seed=SEED0 + 77) for f in range(B)])
            g.copy_(torch.from_numpy(grids2).cuda())
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            for f in range(B):
                assert_same(out[f].cpu().numpy(), oracle.decode(grids2[f], levels)[129:429, 257:757], "graph replay frame %d" % f)
            assert c.scratch_bytes() == before
        c.close()


def test_python_numpy_torch_and_batch_surfaces(H, oracle, lena):
    import torch
    from rustyhgi_amd.interpolator import Crossed, LeftTop
    for interp, I in ((1, Crossed), (0, LeftTop)):
        dec = H.Decoder(I())
        for levels in (4, 7, 10):
            grid = oracle.encode(lena, levels, oracle.linear_lut(1)[0], interp)
            full = oracle.decode(grid, levels, interp)
            rect = (37, 101, 150, 77)
            got = dec.decode_region((256, 256), levels, grid, rect)
            assert isinstance(got, np.ndarray) and got.shape == (77, 150)
            assert_same(got, full[101:178, 37:187], "numpy L%d" % levels)
            tg = torch.from_numpy(grid).cuda()
            got = dec.decode_region((256, 256), levels, tg, rect)
            assert torch.is_tensor(got) and got.is_cuda and tuple(got.shape) == (77, 150)
            assert_same(got.cpu().numpy(), full[101:178, 37:187], "torch L%d" % levels)
            stack = torch.stack([tg, torch.from_numpy(oracle.encode(lena[::-1].copy(), levels, oracle.linear_lut(1)[0], interp)).cuda()])
            out = torch.full((2, 77, 150), SENT, dtype=torch.uint8, device="cuda")
            r = dec.decode_region_batch(stack, levels, rect, out=out)
            torch.cuda.synchronize()
            assert r is out
            assert_same(out[0].cpu().numpy(), full[101:178, 37:187], "batch frame 0")
            assert_same(out[1].cpu().numpy(), oracle.decode(stack[1].cpu().numpy(), levels, interp)[101:178, 37:187], "batch frame 1")
            nb = dec.decode_region_batch(stack.cpu().numpy(), levels, rect)
            assert (nb == out.cpu().numpy()).all()


def test_cli_region_is_the_crop_of_the_full_decode(H, oracle, lena, tmp_path):
    from rustyhgi_amd import Archive, Grid, Metadata
    exe = str(tmp_path / "hgi")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "cli", "hgi_cli.cpp"),
                           "-L", os.path.join(ROOT, "rustyhgi_amd"), "-lhgi_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "rustyhgi_amd"),
                           "-o", exe])
    g = oracle.encode(lena, 6, oracle.linear_lut(2)[0])
    with open(str(tmp_path / "a.hgi"), "wb") as f:
        Archive(Metadata(2, 0, 256, 256, 6), Grid(g, 256)).serialize_to_writer(f)
    run = lambda *a: subprocess.run([exe, "decode", "-i", "a.hgi"] + list(a), cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert run("-o", "full.pgm").returncode == 0
    full = np.frombuffer(open(str(tmp_path / "full.pgm"), "rb").read()[15:], np.uint8).reshape(256, 256)
    assert_same(full, oracle.decode(g, 6), "cli full decode")
    for rect in ((10, 20, 100, 50), (255, 255, 1, 1), (0, 0, 256, 256), (129, 3, 127, 61)):
        r = run("-o", "w.pgm", "--region", ",".join(map(str, rect)))
        assert r.returncode == 0, r.stderr
        x0, y0, rw, rh = rect
        data = open(str(tmp_path / "w.pgm"), "rb").read()
        head = ("P5\n%d %d\n255\n" % (rw, rh)).encode()
        assert data.startswith(head)
        assert_same(np.frombuffer(data[len(head):], np.uint8).reshape(rh, rw), full[y0:y0 + rh, x0:x0 + rw], "cli %r" % (rect,))
    for bad in ("1,2,3", "a,b,c,d", "250,0,10,10", "0,0,0,5", "-1,0,2,2", "1,2,3,4,5", "4294967295,0,1,1"):
        r = run("-o", "bad.pgm", "--region", bad)
        assert r.returncode != 0 and "region" in r.stderr, (bad, r.stderr)


FORCED_MODES = ["HGI_FORCE_CHECKED=1", "HGI_NO_LATTICE_KERNEL=1", "HGI_NO_LATTICE_KERNEL=1,HGI_FORCE_CHECKED=1"]


@pytest.mark.parametrize("mode", FORCED_MODES)
def test_forced_code_paths_in_a_child_process(mode):
    """The knobs build re-runs the shape-heavy region cases with the byte-checked path and / or the host recursion for the
    lattice plane forced: the bytes must not change."""
    from rustyhgi_amd import _ffi
    knobs = os.path.join(os.path.dirname(_ffi.LIB_PATH), "libhgi_hip_knobs.so")
    assert os.path.exists(knobs)
    env = dict(os.environ, HGI_LIB_PATH=knobs, **dict(kv.split("=") for kv in mode.split(",")))
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_region_gpu.py"), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "lena_all_depths or ragged_and_deep or batch_layouts"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, mode + "\n" + r.stdout[-3000:] + r.stderr[-1000:]


def _time(ctx, fn, reps=20):
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
def test_region_cost_follows_the_window(ctx):
    """Loose guards (targets: DESIGN.md 4.6, profiles/r05_region.txt): a 1080p window of a resident 16384^2 L8 grid <= 0.2 x the
    whole-frame decode; a 1024^2 window of each frame of a 64 x 4096^2 L4 batch <= 0.25 x the full batch decode."""
    import torch
    from rustyhgi_amd import _ffi
    L = _ffi.lib()
    for (w, h, B, levels, rect, bound) in ((16384, 16384, 1, 8, (5001, 7003, 1920, 1080), 0.2), (4096, 4096, 64, 4, (1000, 2000, 1024, 1024), 0.25)):
        grid = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED0, 0, w, h, grid.data_ptr(), B, w * h))
        full = torch.empty_like(grid)
        x0, y0, rw, rh = rect
        win = torch.empty((B, rh, rw), dtype=torch.uint8, device="cuda")
        t_full = _time(ctx, lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, full.data_ptr(), B, w * h)))
        t_win = _time(ctx, lambda: _ffi.check(L.hgi_decode_region_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, x0, y0, rw, rh,
                                                                        win.data_ptr(), rw, B, w * h, rw * rh)))
        torch.cuda.synchronize()
        assert torch.equal(win, full[:, y0:y0 + rh, x0:x0 + rw])
        print("%d x %dx%d L%d window %r: %.1f us of %.1f us (%.3f)" % (B, w, h, levels, rect, t_win * 1e3, t_full * 1e3, t_win / t_full))
        assert t_win <= bound * t_full, (rect, t_win, t_full)
        del grid, full, win
        torch.cuda.empty_cache()
