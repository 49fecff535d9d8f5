"""Region decode (hgi_decode_region_u8_dev) against the whole-frame decode, device-resident, HIP events, one process: writes
profiles/r05_region.txt (or the path given as argv[1]).
  * C4: a 1920 x 1080 window at (5001, 7003) of a 16384^2 level-8 grid, against the whole C4 decode;
  * a 1024^2 window at (1000, 2000) of every frame of a 64 x 4096^2 level-4 batch, against the full batch decode;
  * the yardstick: a whole 1920 x 1080 level-8 frame decoded by hgi_decode_u8_dev;
  * windows from 64^2 up to the whole 16384^2 frame: time against the area of the cover (tiles of 128 x 64 that intersect it).
Every window is checked against the crop of the full decode before it is timed."""
import os
import sys

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


def full_fn(grid, w, h, B, levels, out):
    return lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, out.data_ptr(), B, w * h))


def region_fn(grid, w, h, B, levels, rect, win):
    x0, y0, rw, rh = rect
    return lambda: _ffi.check(L.hgi_decode_region_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, x0, y0, rw, rh, win.data_ptr(),
                                                         rw, B, w * h, rw * rh))


def cover(rect):
    x0, y0, rw, rh = rect
    return ((x0 + rw - 1) // 128 - x0 // 128 + 1) * ((y0 + rh - 1) // 64 - y0 // 64 + 1)


def case(w, h, B, levels, rects, label):
    grid = make_grid(w, h, B, levels)
    full = torch.empty_like(grid)
    ff = full_fn(grid, w, h, B, levels, full)
    ff()
    torch.cuda.synchronize()
    t_full, t_full_min = timed(ff)
    say("%s: %d x %dx%d L%d whole decode %.1f us (min %.1f)" % (label, B, w, h, levels, t_full, t_full_min))
    res = []
    for rect in rects:
        x0, y0, rw, rh = rect
        win = torch.empty((B, rh, rw), dtype=torch.uint8, device="cuda")
        rf = region_fn(grid, w, h, B, levels, rect, win)
        rf()
        torch.cuda.synchronize()
        assert torch.equal(win, full[:, y0:y0 + rh, x0:x0 + rw]), rect
        t, tmin = timed(rf)
        say("  window %-24s cover %6d tiles (%5.1f %% of the frame's)  %8.1f us (min %8.1f)  %.3f x whole"
            % ("%d,%d %dx%d" % rect, cover(rect) * B, 100.0 * cover(rect) / (((w + 127) // 128) * ((h + 63) // 64)), t, tmin, t / t_full))
        res.append((rect, t))
        del win
    del grid, full
    torch.cuda.empty_cache()
    return t_full, res


say("# region decode vs whole-frame decode (tools/region_time.py; medians of 5 rounds x 50 launches, HIP events)")
say("# device: %s" % torch.cuda.get_device_name(0))
t_yard, _ = case(1920, 1080, 1, 8, [], "yardstick")
t_c4, r = case(16384, 16384, 1, 8, [(5001, 7003, 1920, 1080)], "C4")
t_c4w = r[0][1]
say("C4 1080p window: %.1f us = %.2f x the 1080p L8 yardstick (target <= 2), %.3f x the whole C4 decode (target <= 0.1)"
    % (t_c4w, t_c4w / t_yard, t_c4w / t_c4))
t_b, r = case(4096, 4096, 64, 4, [(1000, 2000, 1024, 1024)], "batch")
say("batch 1024^2 window: %.1f us = %.3f x the full batch decode (target <= 0.12; the cover is %.1f %% of the frame)"
    % (r[0][1], r[0][1] / t_b, 100.0 * cover((1000, 2000, 1024, 1024)) / (32 * 64)))
sizes = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
rects = [(0, 0, s, s) if s == 16384 else (1000, 3000, s, s) for s in sizes]
_, res = case(16384, 16384, 1, 8, rects, "sizes (C4 grid)")
say("# us per cover tile, by window size: " + "  ".join("%d^2 %.4f" % (s, t / cover(rc)) for s, (rc, t) in zip(sizes, res)))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r05_region.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
ctx.close()
