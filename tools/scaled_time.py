"""Scaled decode (hgi_decode_scaled_u8_dev / hgi_decode_scaled_u8) against the whole-frame decode, device-resident grids, HIP
events, one process: writes profiles/r06_scaled.txt (or the path given as argv[1]).
  * 64 x 4096^2 L4 at s = 1, 2, 3 against the whole-batch decode, and the composed route at s = 1, 2 (torch's strided
    .contiguous() gather of grid[:, ::S, ::S], then hgi_decode_u8_dev on levels - s);
  * C4 (16384^2 L8) at s = 1, 4 against the whole C4 decode;
  * one 1920 x 1080 L8 frame at s = 1 against its whole decode;
  * the host call on a C4 frame at s = 2 against hgi_decode_u8 on the same frame.
Every output is checked against the sliced full decode before it is timed.  Targets are printed beside each
figure; a miss is recorded as a miss."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi  # noqa: E402

L = _ffi.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=50, rounds=5):
    for _ in range(10):
        fn()
    best = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(best)), float(min(best))


def make_grid(w, h, B, levels, q=3):
    img = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
    _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_RAMP, 0x48474934, 0, w, h, img.data_ptr(), B, w * h))
    lut = np.zeros(256, np.uint8)
    _ffi.check(L.hgi_linear_lut(q, lut.ctypes.data, None))
    grid = torch.empty_like(img)
    _ffi.check(L.hgi_encode_u8_dev(ctx.handle, img.data_ptr(), w, h, levels, 1, lut.ctypes.data, grid.data_ptr(), B, w * h))
    del img
    return grid


def ssize(w, h, s):
    return -(-w >> s), -(-h >> s)


def verdict(x, target):
    return "met" if x <= target else "MISSED"


def case(w, h, B, levels, ss, label, targets, composed=()):
    grid = make_grid(w, h, B, levels)
    full = torch.empty_like(grid)
    ff = lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, full.data_ptr(), B, w * h))
    ff()
    torch.cuda.synchronize()
    t_full, t_full_min = timed(ff)
    say("%s: %d x %dx%d L%d whole decode %.1f us (min %.1f)" % (label, B, w, h, levels, t_full, t_full_min))
    res = {}
    for s in ss:
        sw, sh = ssize(w, h, s)
        out = torch.empty((B, sh, sw), dtype=torch.uint8, device="cuda")
        sf = lambda: _ffi.check(L.hgi_decode_scaled_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B, w * h,
                                                           sw * sh))
        sf()
        torch.cuda.synchronize()
        S = 1 << s
        assert torch.equal(out, full[:, ::S, ::S]), (label, s)
        t, tmin = timed(sf)
        res[s] = t
        tg = targets.get(s)
        say("  s = %d (%dx%d): %8.1f us (min %8.1f)  %.3f x whole%s" % (s, sw, sh, t, tmin, t / t_full,
                                                                       "  (target <= %.2f: %s)" % (tg, verdict(t / t_full, tg)) if tg else ""))
        if s in composed:
            comp = torch.empty((B, sh, sw), dtype=torch.uint8, device="cuda")
            holder = {}

            def cf():
                sub = grid[:, ::S, ::S].contiguous()
                holder["sub"] = sub
                _ffi.check(L.hgi_decode_u8_dev(ctx.handle, sub.data_ptr(), sw, sh, max(levels - s, 0), 1, comp.data_ptr(), B, sw * sh))
            cf()
            torch.cuda.synchronize()
            assert torch.equal(comp, full[:, ::S, ::S]), ("composed", label, s)
            tc, tcmin = timed(cf)
            say("  composed route s = %d (strided gather + whole decode of L%d): %8.1f us (min %8.1f)  %.3f x whole; fused / composed %.3f%s"
                % (s, levels - s, tc, tcmin, tc / t_full, t / tc, "  (target <= 0.75: %s)" % verdict(t / tc, 0.75) if s == 1 else ""))
            del comp, holder
        del out
    del grid, full
    torch.cuda.empty_cache()
    return t_full, res


say("# scaled decode vs whole-frame decode (tools/scaled_time.py; medians of 5 rounds x 50 launches, HIP events)")
say("# device: %s" % torch.cuda.get_device_name(0))
say("# byte floors (1/2^s + 1/4^s of the 2 B/px full decode): s = 1 0.375 x, s = 2 0.156 x, s = 3 0.070 x")
case(4096, 4096, 64, 4, (1, 2, 3), "C3 batch", {1: 0.45, 2: 0.22, 3: 0.12}, composed=(1, 2))
case(16384, 16384, 1, 8, (1, 4), "C4", {1: 0.5})
case(1920, 1080, 1, 8, (1,), "1080p", {})

# the host call: a C4 frame at s = 2 (uploads a quarter of the rows) against hgi_decode_u8 on the same frame
w = h = 16384
g = make_grid(w, h, 1, 8)[0].cpu().numpy()
full = np.empty_like(g)
sw, sh = ssize(w, h, 2)
small = np.empty((sh, sw), np.uint8)


def host_t(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


t_hf = host_t(lambda: _ffi.check(L.hgi_decode_u8(ctx.handle, g.ctypes.data, w, h, 8, 1, full.ctypes.data)))
t_hs = host_t(lambda: _ffi.check(L.hgi_decode_scaled_u8(ctx.handle, g.ctypes.data, w, h, 8, 1, 2, small.ctypes.data, sw)))
assert (small == full[::4, ::4]).all()
say("host call, C4 frame: hgi_decode_u8 %.2f ms, hgi_decode_scaled_u8 s = 2 %.2f ms (%.3f x)" % (t_hf, t_hs, t_hs / t_hf))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_scaled.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
ctx.close()
