"""Frame lists (hgi_encode_u8_list_dev / hgi_decode_u8_list_dev) against the per-frame loop of the uniform calls and against the
uniform 64 x 4096^2 call, device-resident, HIP events, one process: writes profiles/r07_framelist.txt (or the path in argv[1]).
All workloads at level 4, Medium, Crossed; each list's frames lie in one buffer at 256-B offsets; the pointer and size arrays are
built once, outside the timed loops.
  * W1 mixed: 1024 frames, widths and heights drawn independently and uniformly from [64, 2048] (seed printed), ~1.1 Gpx;
  * W2 thumbnails: 8192 frames, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard passed as 64 pointers.
Every list result is checked against the per-frame uniform call before it is timed.  The enqueue (host) time of a list call is
the host clock around the call with the device queue drained first.
`--prof`: the workload of the counter passes instead -- W1's list encode and decode, five launches each after the check, nothing
timed (rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE, one counter per pass: bytes = 2 * FETCH_SIZE * 1024 and
WRITE_SIZE * 1024, gfx950's FETCH correction as in tools/profile.sh)."""
import ctypes
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
LEVELS, INTERP, SEED = 4, 1, 0x48474937
LUT = np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(2, LUT.ctypes.data, None))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps, rounds=5):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms)), float(min(ms))


def enqueue_us(fn, reps=20):
    """Host time of one call (the device queue drained first, so that nothing blocks it)."""
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    torch.cuda.synchronize()
    return best * 1e6


class Workload:
    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.offs, at = [], 0
        for w, h in shapes:
            self.offs.append(at)
            at += (w * h + 255) // 256 * 256
        self.bytes = at
        self.px = sum(w * h for w, h in shapes)
        self.img = torch.empty(at, dtype=torch.uint8, device="cuda")
        for i, ((w, h), o) in enumerate(zip(shapes, self.offs)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_RAMP if i % 2 else _ffi.SYNTH_NOISE, SEED, i, w, h,
                                          self.img.data_ptr() + o, 1, w * h))
        self.grid = torch.empty_like(self.img)
        self.out = torch.empty_like(self.img)
        P, U = ctypes.c_void_p * self.n, ctypes.c_uint32 * self.n
        self.p_img = P(*[self.img.data_ptr() + o for o in self.offs])
        self.p_grid = P(*[self.grid.data_ptr() + o for o in self.offs])
        self.p_out = P(*[self.out.data_ptr() + o for o in self.offs])
        self.ws = U(*[w for w, h in shapes])
        self.hs = U(*[h for w, h in shapes])
        self.loop_args = [(self.p_img[i], self.p_grid[i], self.p_out[i], w, h) for i, (w, h) in enumerate(shapes)]

    def enc_list(self):
        _ffi.check(L.hgi_encode_u8_list_dev(ctx.handle, self.p_img, self.ws, self.hs, LEVELS, INTERP, LUT.ctypes.data, self.p_grid, self.n))

    def dec_list(self):
        _ffi.check(L.hgi_decode_u8_list_dev(ctx.handle, self.p_grid, self.ws, self.hs, LEVELS, INTERP, self.p_out, self.n))

    def enc_loop(self):
        for pi, pg, _, w, h in self.loop_args:
            _ffi.check(L.hgi_encode_u8_dev(ctx.handle, pi, w, h, LEVELS, INTERP, LUT.ctypes.data, pg, 1, w * h))

    def dec_loop(self):
        for _, pg, po, w, h in self.loop_args:
            _ffi.check(L.hgi_decode_u8_dev(ctx.handle, pg, w, h, LEVELS, INTERP, po, 1, w * h))

    def check(self):
        """The list's bytes against the per-frame loop's."""
        self.enc_list()
        self.dec_list()
        torch.cuda.synchronize()
        g, o = self.grid.clone(), self.out.clone()
        self.enc_loop()
        self.dec_loop()
        torch.cuda.synchronize()
        assert torch.equal(g, self.grid) and torch.equal(o, self.out), "%s: list and per-frame loop differ" % self.name

    def free(self):
        del self.img, self.grid, self.out
        torch.cuda.empty_cache()


def main(path):
    rng = np.random.default_rng(SEED)
    say("# tools/framelist_time.py: frame lists against the per-frame loop and the uniform call; L%d Medium Crossed, device-resident,"
        % LEVELS)
    say("# HIP events, median (min) of 5 rounds; seed 0x%x; %s; torch %s" % (SEED, L.hgi_version().decode(), torch.__version__))
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    w3 = [(4096, 4096)] * 64
    # the uniform 64 x 4096^2 call: the yardstick of W1's pixel rate and of W3
    uni = Workload("U", w3)
    t_uni = {}
    for d, fn in (("encode", lambda: _ffi.check(L.hgi_encode_u8_dev(ctx.handle, uni.img.data_ptr(), 4096, 4096, LEVELS, INTERP,
                                                                   LUT.ctypes.data, uni.grid.data_ptr(), 64, 4096 * 4096))),
                  ("decode", lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, uni.grid.data_ptr(), 4096, 4096, LEVELS, INTERP,
                                                                   uni.out.data_ptr(), 64, 4096 * 4096)))):
        t_uni[d] = timed(fn, 20)
        say("uniform 64 x 4096^2 %s: %.1f us (min %.1f), %.2f Gpx/s" % (d, t_uni[d][0] * 1e3, t_uni[d][1] * 1e3,
                                                                       uni.px / t_uni[d][0] / 1e6))
    uni.free()
    targets = {"W1": ("loop", 6.0), "W2": ("loop", 30.0), "W3": ("uniform", 1.15)}
    for name, shapes in (("W1", w1), ("W2", w2), ("W3", w3)):
        wl = Workload(name, shapes)
        wl.check()
        say("")
        say("%s: %d frames, %.3f Gpx%s" % (name, wl.n, wl.px / 1e9, "" if name == "W3" else
                                           ", sides %d..%d" % (min(min(s) for s in shapes), max(max(s) for s in shapes))))
        for d in ("encode", "decode"):
            lst = wl.enc_list if d == "encode" else wl.dec_list
            loop = wl.enc_loop if d == "encode" else wl.dec_loop
            t_list = timed(lst, 20 if wl.px > 3e8 else 50)
            t_loop = timed(loop, 2 if wl.n > 2000 else 3, rounds=3)
            host = enqueue_us(lst)
            rate = wl.px / t_list[0] / 1e6
            say("  %s list %.1f us (min %.1f), %.2f Gpx/s; per-frame loop %.1f us: loop / list = %.1fx; enqueue %.1f us per call, "
                "%.3f us per frame" % (d, t_list[0] * 1e3, t_list[1] * 1e3, rate, t_loop[0] * 1e3, t_loop[0] / t_list[0], host,
                                      host / wl.n))
            kind, target = targets[name]
            if kind == "loop":
                ok = t_loop[0] / t_list[0] >= target
                say("    target: list >= %.0fx faster than the loop -> %.1fx %s" % (target, t_loop[0] / t_list[0], "met" if ok else "MISSED"))
                if name == "W1":
                    r = rate / (uni.px / t_uni[d][0] / 1e6)
                    say("    target: pixel rate >= 0.7x the uniform 64 x 4096^2 call -> %.2fx %s" % (r, "met" if r >= 0.7 else "MISSED"))
            else:
                r = t_list[0] / t_uni[d][0]
                say("    target: list <= %.2fx the uniform call -> %.3fx %s" % (target, r, "met" if r <= target else "MISSED"))
        wl.free()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    rng = np.random.default_rng(SEED)
    wl = Workload("W1", [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)])
    wl.check()
    for _ in range(5):
        wl.enc_list()
    for _ in range(5):
        wl.dec_list()
    torch.cuda.synchronize()
    print("W1: %d frames, %d px, %d bytes in the buffer" % (wl.n, wl.px, wl.bytes))


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_framelist.txt"))
