"""Mapped decode (hgi_map_decode_dev, libhgi_map.so) against the route it replaces -- hgi_decode_u8_dev of libhgi_hip.so, then one
elementwise conversion -- device-resident, one process, on the same planes: writes profiles/r10_mapped.txt (or the path in
argv[1]).  Clocks are settled by a burst of the uniform decode first; every figure is the median (min) of 5 rounds timed with
the ctx's own event pair (hgi_timer_start / hgi_timer_stop) on the one stream all calls run on, around `reps` back-to-back calls.
For 64 x 4096^2 at level 4 and for C4 (one 16384^2 at level 8), at E = 2 (float16) and E = 4 (float32), noise grids:
  (a) the composed route: hgi_decode_u8_dev, then one tensor.to(dtype) -- (3 + E) B/px, two launches, the cheapest form of the
      two-launch route (the conversion writes into a preallocated frame, `out.copy_(image)`: the same kernel without the
      allocation of a fresh result per call); its table is the plain conversion;
  (b) hgi_map_decode_dev, packed, with that table -- (1 + E) B/px, one launch;
  (c) (b) with rows 4224 (C4: 16512) elements apart on both sides;
  (d) hgi_copy_u8_dev moving the same (1 + E) B/px, the same run's streaming yardstick;
  (e) hgi_decode_u8_pitched_dev alone (packed), against the uniform hgi_decode_u8_dev: the cost of the simple tile walk the
      mapped launch inherits.
The mapped results are checked against the composed route's before they are timed.  Condition: (b) < (a) everywhere.
Expectation reported next to it: (b) / (a) against the byte ratios (1 + E) / (3 + E) = 0.60 and 0.71, and against those times
(e) / (uniform decode).
`--prof`: the launches of (a) and (b) alone, five times each after the check, nothing timed (for a counter pass of its own:
rocprofv3 --pmc, never combined with tracing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_map  # noqa: E402
from rustyhgi_amd.planes import Planes  # noqa: E402

L = _ffi.lib()
M = _ffi_map.lib()
ctx = H.Context(0)
STREAM = torch.cuda.current_stream().cuda_stream
ctx.set_stream(STREAM)
INTERP, SEED = 1, 0x48474939
DTYPES = {2: torch.float16, 4: torch.float32}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps, rounds=5):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps):
            fn()
        ms.append(ctx.timer_stop() / reps)
    return float(np.median(ms)), float(min(ms))


def us(t):
    return "%.1f us (min %.1f)" % (t[0] * 1e3, t[1] * 1e3)


def mark(ratio, target):
    return "%.3fx (expectation <= %.3fx: %s)" % (ratio, target, "met" if ratio <= target else "MISSED by %.1f %%" % (100 * (ratio / target - 1)))


class Case:
    """`batch` grids of w x h: the grid and the uint8 image in two planes placed by the library, each large enough for rows
    `pitch` bytes apart; the typed output and the copy yardstick's buffers from torch."""

    def __init__(self, w, h, batch, levels, pitch):
        self.w, self.h, self.B, self.levels, self.pitch = w, h, batch, levels, pitch
        self.planes = Planes(ctx, batch * h * pitch, 2)
        self.p = self.planes.pointers
        # a noise plane is a valid grid, and the table's worst case: neighbouring lanes look up unrelated entries
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, w, h, self.p[0], batch, w * h))
        self.out = torch.empty((batch * h * pitch * 4,), dtype=torch.uint8, device="cuda")
        n = batch * w * h
        self.cp = torch.empty((2, (5 * n + 1) // 2), dtype=torch.uint8, device="cuda")
        self.tables = dict((e, torch.arange(256, dtype=torch.float32, device="cuda").to(dt)) for e, dt in DTYPES.items())
        self.conv = dict((e, torch.empty((batch, h, w), dtype=dt, device="cuda")) for e, dt in DTYPES.items())

    def grid(self, pitch):
        return self.planes.torch(0, (self.B, self.h, pitch))[:, :, :self.w]

    def image(self):
        return self.planes.torch(1, (self.B, self.h, self.w))

    def typed(self, e, pitch):
        n = self.B * self.h * pitch
        return self.out[:n * e].view(DTYPES[e]).view(self.B, self.h, pitch)[:, :, :self.w]

    def decode(self):
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, self.p[0], self.w, self.h, self.levels, INTERP, self.p[1], self.B, self.w * self.h))

    def decode_pitched(self):
        _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, self.p[0], self.w, self.w, self.h, self.levels, INTERP, self.p[1], self.w, self.B,
                                               self.w * self.h, self.w * self.h))

    def composed(self, e):
        self.decode()
        self.conv[e].copy_(self.image())      # tensor.to(dtype)'s conversion kernel into a preallocated frame: no allocator work

    def mapped(self, e, pitch=None):
        pitch = pitch or self.w
        _ffi_map.check(M.hgi_map_decode_dev(STREAM or None, self.p[0], pitch, self.w, self.h, self.levels, INTERP, self.tables[e].data_ptr(), e,
                                            self.out.data_ptr(), pitch * e, self.B, pitch * self.h, pitch * self.h * e))

    def copy(self, e):
        """(1 + E) B/px of traffic: (1 + E) / 2 bytes per pixel read and as many written."""
        n = self.B * self.w * self.h * (1 + e) // 2
        _ffi.check(L.hgi_copy_u8_dev(ctx.handle, self.cp[0].data_ptr(), self.cp[1].data_ptr(), n))

    def check(self):
        """The mapped launch's output against the composed route's, packed and (if the planes hold it) pitched."""
        for e in DTYPES:
            self.composed(e)
            torch.cuda.synchronize()
            want = self.conv[e].clone()
            self.out.zero_()
            self.mapped(e)
            torch.cuda.synchronize()
            assert torch.equal(self.typed(e, self.w), want), "mapped output differs from decode + conversion (E = %d)" % e
            if self.pitch != self.w:
                g = self.grid(self.w).clone()
                self.grid(self.pitch).copy_(g)
                self.out.zero_()
                self.mapped(e, self.pitch)
                torch.cuda.synchronize()
                assert torch.equal(self.typed(e, self.pitch), want), "pitched mapped output differs (E = %d)" % e
                self.grid(self.w).copy_(g)
                del g
            del want
        torch.cuda.empty_cache()

    def to_pitch(self):
        g = self.grid(self.w).clone()
        self.grid(self.pitch).copy_(g)
        del g
        torch.cuda.synchronize()

    def free(self):
        self.planes.close()
        del self.out, self.cp, self.conv
        torch.cuda.empty_cache()


def settle(c):
    for _ in range(400):
        c.decode()
    torch.cuda.synchronize()


def legs(c, title, reps):
    px = c.B * c.w * c.h
    say("")
    say(title)
    t_u, t_e = timed(c.decode, reps), timed(c.decode_pitched, reps)
    walk = t_e[0] / t_u[0]
    say("  hgi_decode_u8_dev alone        %s  %.2f Gpx/s" % (us(t_u), px / t_u[0] / 1e6))
    say("  (e) hgi_decode_u8_pitched_dev  %s  %.2f Gpx/s; (e) / uniform = %.3fx (the simple tile walk)" % (us(t_e), px / t_e[0] / 1e6, walk))
    res = {}
    for e in DTYPES:
        t_a = timed(lambda: c.composed(e), reps)
        t_b = timed(lambda: c.mapped(e), reps)
        t_d = timed(lambda: c.copy(e), reps)
        res[e] = (t_a, t_b, t_d)
        bytes_ratio = (1 + e) / (3 + e)
        say("  E = %d (%s)" % (e, str(DTYPES[e]).replace("torch.", "")))
        say("    (a) decode + tensor.to        %s  %.2f Gpx/s" % (us(t_a), px / t_a[0] / 1e6))
        say("    (b) mapped decode, packed     %s  %.2f Gpx/s  %.0f GB/s" % (us(t_b), px / t_b[0] / 1e6, (1 + e) * px / t_b[0] / 1e6))
        say("    (d) hgi_copy_u8_dev, %d B/px   %s  %.0f GB/s" % (1 + e, us(t_d), (1 + e) * px / t_d[0] / 1e6))
        say("    condition (b) < (a): %s" % ("met" if t_b[0] < t_a[0] else "MISSED"))
        say("    (b) / (a) = %s" % mark(t_b[0] / t_a[0], bytes_ratio))
        say("    (b) / (a) against the walk-adjusted ratio: %s" % mark(t_b[0] / t_a[0], bytes_ratio * walk))
        say("    (b) / (d) = %.3fx; (b) / uniform decode = %.3fx" % (t_b[0] / t_d[0], t_b[0] / t_u[0]))
    c.to_pitch()
    for e in DTYPES:
        t_c = timed(lambda: c.mapped(e, c.pitch), reps)
        say("  E = %d (c) mapped decode, pitch %d elements  %s  %.2f Gpx/s; (c) / (b) = %.3fx; (c) / (a) = %.3fx"
            % (e, c.pitch, us(t_c), px / t_c[0] / 1e6, t_c[0] / res[e][1][0], t_c[0] / res[e][0][0]))


def main(path):
    say("# tools/mapped_time.py: mapped decode (one launch, 1 + E B/px) against decode + conversion (two launches, 3 + E B/px);")
    say("# device-resident, same planes (hgi_planes_alloc), hgi_timer_* events on one stream, median (min) of 5 rounds; noise grids")
    say("# %s; %s; torch %s" % (L.hgi_version().decode(), M.hgi_map_version().decode(), torch.__version__))
    c = Case(4096, 4096, 64, 4, 4224)
    say("# planes: %s (separated: %s)" % (c.planes.report, c.planes.separated))
    c.check()
    settle(c)
    legs(c, "64 x 4096^2, level 4, Crossed", 20)
    c.free()
    e = Case(16384, 16384, 1, 8, 16512)
    e.check()
    legs(e, "one 16384^2, level 8, Crossed (C4)", 20)
    e.free()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    c = Case(4096, 4096, 64, 4, 4096)
    c.check()
    for _ in range(5):
        c.decode()
    for e in DTYPES:
        for _ in range(5):
            c.conv[e].copy_(c.image())
        for _ in range(5):
            c.mapped(e)
    torch.cuda.synchronize()
    print("64 x 4096^2: %d pixels; 5 x hgi_decode_u8_dev, then per E in (2, 4): 5 x tensor.to, 5 x hgi_map_decode_dev" % (c.B * c.w * c.h))
    c.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_mapped.txt"))
