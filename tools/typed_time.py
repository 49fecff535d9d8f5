"""Typed encode (hgi_typed_encode_dev, libhgi_typed.so) against the route it replaces -- one torch conversion of the float frame to
uint8, then hgi_encode_u8_pitched_dev of libhgi_hip.so -- device-resident, one process, on the same planes: writes
profiles/r13_typed.txt (or the path in argv[1]).  Clocks are settled by a burst of the uniform encode first; every figure is the
median (min) of 5 rounds timed with the ctx's own event pair (hgi_timer_start / hgi_timer_stop) on the one stream all calls run
on, around `reps` back-to-back calls.  For 64 x 4096^2 at level 4, Medium, and for C4 (one 16384^2 at level 8, High), Crossed, at
float16 and float32, on frames x = affine_table(dtype)[noise image] -- the converted image is the noise input of the other records:
  (a) the two-step route a pipeline has today: clamp(round(x * 255), 0, 255) -> uint8 by torch, into preallocated buffers (a
      float32 temporary and the uint8 frame: no allocator work; the bias is 0, so its add is left out -- the cheapest form of the
      composition), then hgi_encode_u8_pitched_dev -- (E + 3) B/px of codec traffic plus torch's temporaries;
  (b) hgi_typed_encode_dev, packed -- (E + 1) B/px, one launch;
  (c) (b) with rows 4224 (C4: 16512) elements apart on both sides;
  (d) hgi_copy_u8_dev moving the same (E + 1) B/px, the same run's streaming yardstick;
  (e) hgi_encode_u8_pitched_dev alone (packed).
The typed grids are checked against the two-step route's before they are timed.  Condition: (b) < (a) everywhere.  Reported next
to it: (b) / (a) against the byte ratios (E + 1) / (E + 3) = 0.60 and 0.71, and (b) / (d) beside what the neighbouring launches
reached against the copy of their own bytes (mapped decode 1.04-1.16x, encode with reconstruction 1.07x).
`--prof`: the launches of (a) and (b) alone, five times each after the check, nothing timed (for a counter pass of its own:
rocprofv3 --pmc, never combined with tracing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_typed  # noqa: E402
from rustyhgi_amd.planes import Planes  # noqa: E402
from rustyhgi_amd.quantizator import Linear, QuantizationLevel  # noqa: E402

L = _ffi.lib()
T = _ffi_typed.lib()
ctx = H.Context(0)
STREAM = torch.cuda.current_stream().cuda_stream
ctx.set_stream(STREAM)
INTERP, SEED = 1, 0x48474939
DTYPES = {2: torch.float16, 4: torch.float32}
NP_DTYPES = {2: np.float16, 4: np.float32}
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
    """`batch` frames of w x h: the uint8 image and the grid in two planes placed by the library, each large enough for rows
    `pitch` bytes apart; the float frames, the conversion's temporary and the copy yardstick's buffers from torch."""

    def __init__(self, w, h, batch, levels, quant, pitch):
        self.w, self.h, self.B, self.levels, self.pitch = w, h, batch, levels, pitch
        self.lut = np.ascontiguousarray(Linear(quant).table(), dtype=np.uint8)
        self.planes = Planes(ctx, batch * h * pitch, 2)
        self.p = self.planes.pointers
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, w, h, self.p[0], batch, w * h))
        n = batch * w * h
        self.frame = torch.empty((batch * h * pitch * 4,), dtype=torch.uint8, device="cuda")
        self.tmp = torch.empty((batch, h, w), dtype=torch.float32, device="cuda")
        self.cp = torch.empty((2, (5 * n + 1) // 2), dtype=torch.uint8, device="cuda")
        self.want = None

    def image(self):
        return self.planes.torch(0, (self.B, self.h, self.w))

    def grid(self, pitch):
        return self.planes.torch(1, (self.B, self.h, pitch))[:, :, :self.w]

    def typed(self, e, pitch):
        n = self.B * self.h * pitch
        return self.frame[:n * e].view(DTYPES[e]).view(self.B, self.h, pitch)[:, :, :self.w]

    def fill(self, e, pitch):
        """x = affine_table(dtype)[noise image], rows `pitch` elements apart; the image plane keeps the noise."""
        table = H.affine_table(NP_DTYPES[e], device="cuda")
        x = self.typed(e, pitch)
        for f in range(self.B):      # frame by frame: the index tensor of a whole batch is 8 B/px
            x[f].copy_(table[self.image()[f].long()])
        torch.cuda.synchronize()

    def encode(self):
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.p[0], self.w, self.h, self.levels, INTERP, self.lut.ctypes.data, self.p[1], self.B,
                                       self.w * self.h))

    def encode_pitched(self):
        _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, self.p[0], self.w, self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                               self.p[1], self.w, self.B, self.w * self.h, self.w * self.h))

    def convert(self, e):
        """clamp(round(x * 255), 0, 255) -> uint8, every result into a preallocated buffer"""
        x = self.typed(e, self.w)
        if e == 4:
            torch.mul(x, 255.0, out=self.tmp)
        else:
            self.tmp.copy_(x)
            self.tmp.mul_(255.0)
        self.tmp.round_().clamp_(0, 255)
        self.image().copy_(self.tmp)

    def two_step(self, e):
        self.convert(e)
        self.encode_pitched()

    def fused(self, e, pitch=None):
        pitch = pitch or self.w
        _ffi_typed.check(T.hgi_typed_encode_dev(STREAM or None, self.frame.data_ptr(), pitch * e, e, 0, 255.0, 0.0, self.w, self.h, self.levels,
                                                INTERP, self.lut.ctypes.data, self.p[1], pitch, self.B, pitch * self.h * e, pitch * self.h))

    def copy(self, e):
        """(E + 1) B/px of traffic: (E + 1) / 2 bytes per pixel read and as many written."""
        n = self.B * self.w * self.h * (1 + e) // 2
        _ffi.check(L.hgi_copy_u8_dev(ctx.handle, self.cp[0].data_ptr(), self.cp[1].data_ptr(), n))

    def check(self, e, pitch):
        """The typed launch's grid against the two-step route's (packed frames), or against that grid kept from the packed
        check (pitched frames)."""
        if pitch == self.w:
            noise = self.image().clone()
            self.two_step(e)
            torch.cuda.synchronize()
            assert torch.equal(self.image(), noise), "the torch conversion does not give the noise image back (E = %d)" % e
            self.want = self.grid(self.w).clone()
            del noise
        self.planes.torch(1, (self.B * self.h * self.pitch,)).zero_()
        self.fused(e, pitch)
        torch.cuda.synchronize()
        assert torch.equal(self.grid(pitch), self.want), "typed encode differs from conversion + encode (E = %d, pitch %d)" % (e, pitch)

    def free(self):
        self.planes.close()
        del self.frame, self.cp, self.tmp, self.want
        torch.cuda.empty_cache()


def settle(c):
    for _ in range(400):
        c.encode()
    torch.cuda.synchronize()


def legs(c, title, reps):
    px = c.B * c.w * c.h
    say("")
    say(title)
    t_u, t_e = timed(c.encode, reps), timed(c.encode_pitched, reps)
    say("  hgi_encode_u8_dev alone        %s  %.2f Gpx/s" % (us(t_u), px / t_u[0] / 1e6))
    say("  (e) hgi_encode_u8_pitched_dev  %s  %.2f Gpx/s; (e) / uniform = %.3fx" % (us(t_e), px / t_e[0] / 1e6, t_e[0] / t_u[0]))
    for e in DTYPES:
        c.fill(e, c.w)
        c.check(e, c.w)
        t_a = timed(lambda: c.two_step(e), reps)
        t_v = timed(lambda: c.convert(e), reps)
        t_b = timed(lambda: c.fused(e), reps)
        t_d = timed(lambda: c.copy(e), reps)
        say("  E = %d (%s)" % (e, str(DTYPES[e]).replace("torch.", "")))
        say("    (a) torch conversion + encode %s  %.2f Gpx/s (the conversion alone %s)" % (us(t_a), px / t_a[0] / 1e6, us(t_v)))
        say("    (b) typed encode, packed      %s  %.2f Gpx/s  %.0f GB/s" % (us(t_b), px / t_b[0] / 1e6, (1 + e) * px / t_b[0] / 1e6))
        say("    (d) hgi_copy_u8_dev, %d B/px   %s  %.0f GB/s" % (1 + e, us(t_d), (1 + e) * px / t_d[0] / 1e6))
        say("    condition (b) < (a): %s" % ("met" if t_b[0] < t_a[0] else "MISSED"))
        say("    (b) / (a) = %s" % mark(t_b[0] / t_a[0], (1 + e) / (3 + e)))
        say("    (b) / (d) = %.3fx (mapped decode 1.04-1.16x, encode with reconstruction 1.07x); (b) / (e) = %.3fx" % (t_b[0] / t_d[0], t_b[0] / t_e[0]))
        c.fill(e, c.pitch)
        c.check(e, c.pitch)
        t_c = timed(lambda: c.fused(e, c.pitch), reps)
        say("    (c) typed encode, pitch %d elements  %s  %.2f Gpx/s; (c) / (b) = %.3fx; (c) / (a) = %.3fx"
            % (c.pitch, us(t_c), px / t_c[0] / 1e6, t_c[0] / t_b[0], t_c[0] / t_a[0]))
        # the noise image back into its plane for the next element size
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, c.w, c.h, c.p[0], c.B, c.w * c.h))


def main(path):
    say("# tools/typed_time.py: typed encode (one launch, E + 1 B/px) against torch conversion + encode (E + 3 B/px and torch's temporaries);")
    say("# device-resident, same planes (hgi_planes_alloc), hgi_timer_* events on one stream, median (min) of 5 rounds; noise images")
    say("# load layout of the typed kernels: each lane loads the 16 * E contiguous bytes of its own 16 pixels (E b128 loads)")
    say("# %s; %s; torch %s" % (L.hgi_version().decode(), T.hgi_typed_version().decode(), torch.__version__))
    c = Case(4096, 4096, 64, 4, QuantizationLevel.Medium, 4224)
    say("# planes: %s (separated: %s)" % (c.planes.report, c.planes.separated))
    settle(c)
    legs(c, "64 x 4096^2, level 4, Medium, Crossed", 20)
    c.free()
    e = Case(16384, 16384, 1, 8, QuantizationLevel.High, 16512)
    legs(e, "one 16384^2, level 8, High, Crossed (C4)", 20)
    e.free()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    c = Case(4096, 4096, 64, 4, QuantizationLevel.Medium, 4096)
    for e in DTYPES:
        c.fill(e, c.w)
        c.check(e, c.w)
        for _ in range(5):
            c.two_step(e)
        for _ in range(5):
            c.fused(e)
    torch.cuda.synchronize()
    print("64 x 4096^2: %d pixels; per E in (2, 4): 5 x (torch conversion, hgi_encode_u8_pitched_dev), 5 x hgi_typed_encode_dev" % (c.B * c.w * c.h))
    c.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_typed.txt"))
