"""Encode with reconstruction (hgi_recon_encode_u8_dev, libhgi_recon.so) against the route it replaces -- hgi_encode_u8_dev then
hgi_decode_u8_dev of libhgi_hip.so -- device-resident, one process, on the same planes (hgi_planes_alloc): writes
profiles/r09_recon.txt (or the path in argv[1]).  Clocks are settled by a burst of the uniform decode first; every figure is the
median (min) of 5 rounds timed with the ctx's own event pair (hgi_timer_start / hgi_timer_stop) on the one stream all calls run
on, around `reps` back-to-back calls.
  (a) the composed route: encode, then decode of the grid -- 4 B/px, two launches;
  (b) hgi_recon_encode_u8_dev, packed (all three pitches == width) -- 3 B/px, one launch;
  (c) (b) with 4224-byte pitches on all three sides;
  (d) hgi_copy_u8_dev moving 3 B/px (one copy of the frames and one of half of them), the same run's streaming yardstick;
  (e) C4's 16384^2 at level 8 High, (a) and (b).
64 x 4096^2, level 4, Medium, Crossed unless noted.  The fused results are checked against the composed route's before they are
timed.  Expectation reported against: (b) <= 0.80 x (a) -- the bytes are 3/4, times the 1.07 that profiles/r08_pitched.txt
records for the simple 64-row tile walk this launch inherits on the encode side.
`--prof`: the launches of (a) and (b) alone, five times each after the check, nothing timed (for a counter pass of its own:
rocprofv3 --pmc FETCH_SIZE WRITE_SIZE, never combined with tracing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_recon  # noqa: E402
from rustyhgi_amd.planes import Planes  # noqa: E402

L = _ffi.lib()
R = _ffi_recon.lib()
ctx = H.Context(0)
STREAM = torch.cuda.current_stream().cuda_stream
ctx.set_stream(STREAM)
INTERP, SEED = 1, 0x48474939
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def lut_of(level):
    lut = np.zeros(256, np.uint8)
    _ffi.check(L.hgi_linear_lut(level, lut.ctypes.data, None))
    return lut


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
    return "%.3fx (expectation <= %.2fx: %s)" % (ratio, target, "met" if ratio <= target else "MISSED by %.1f %%" % (100 * (ratio / target - 1)))


class Case:
    """`batch` frames of w x h in three planes placed by the library (image, grid, reconstruction), each large enough for
    rows `pitch` bytes apart."""

    def __init__(self, w, h, batch, levels, quant, pitch):
        self.w, self.h, self.B, self.levels, self.pitch = w, h, batch, levels, pitch
        self.lut = lut_of(quant)
        self.planes = Planes(ctx, batch * h * pitch, 3)
        self.p = self.planes.pointers
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, w, h, self.p[0], batch, w * h))

    def view(self, i, pitch):
        t = self.planes.torch(i, (self.B, self.h, pitch))
        return t[:, :, :self.w]

    def encode(self):
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.p[0], self.w, self.h, self.levels, INTERP, self.lut.ctypes.data, self.p[1], self.B,
                                       self.w * self.h))

    def decode(self):
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, self.p[1], self.w, self.h, self.levels, INTERP, self.p[2], self.B, self.w * self.h))

    def composed(self):
        self.encode()
        self.decode()

    def fused(self, pitch=None):
        pitch = pitch or self.w
        _ffi_recon.check(R.hgi_recon_encode_u8_dev(STREAM or None, self.p[0], pitch, self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                                   self.p[1], pitch, self.p[2], pitch, self.B, pitch * self.h, pitch * self.h, pitch * self.h))

    def copy3(self):
        n = self.B * self.w * self.h
        _ffi.check(L.hgi_copy_u8_dev(ctx.handle, self.p[0], self.p[1], n))
        _ffi.check(L.hgi_copy_u8_dev(ctx.handle, self.p[1], self.p[2], n // 2))

    def check(self):
        """The fused launch's two outputs against the composed route's, packed and (if the planes hold it) pitched."""
        self.composed()
        torch.cuda.synchronize()
        grid, rec = self.view(1, self.w).clone(), self.view(2, self.w).clone()
        img = self.view(0, self.w).clone()
        self.view(1, self.w).zero_()
        self.view(2, self.w).zero_()
        self.fused()
        torch.cuda.synchronize()
        assert torch.equal(self.view(1, self.w), grid), "fused grid differs from hgi_encode_u8_dev"
        assert torch.equal(self.view(2, self.w), rec), "fused reconstruction differs from hgi_decode_u8_dev"
        if self.pitch != self.w:
            self.view(0, self.pitch).copy_(img)
            self.view(1, self.pitch).zero_()
            self.view(2, self.pitch).zero_()
            self.fused(self.pitch)
            torch.cuda.synchronize()
            assert torch.equal(self.view(1, self.pitch), grid) and torch.equal(self.view(2, self.pitch), rec), "pitched fused launch differs"
            self.view(0, self.w).copy_(img)
        del grid, rec, img
        torch.cuda.empty_cache()

    def free(self):
        self.planes.close()
        torch.cuda.empty_cache()


def settle(c):
    for _ in range(400):
        c.decode()
    torch.cuda.synchronize()


def main(path):
    say("# tools/recon_time.py: encode with reconstruction (one launch, 3 B/px) against encode + decode (two launches, 4 B/px);")
    say("# device-resident, same planes (hgi_planes_alloc), hgi_timer_* events on one stream, median (min) of 5 rounds;")
    say("# %s; %s; torch %s" % (L.hgi_version().decode(), R.hgi_recon_version().decode(), torch.__version__))
    c = Case(4096, 4096, 64, 4, 2, 4224)
    say("# planes: %s (separated: %s)" % (c.planes.report, c.planes.separated))
    c.check()
    settle(c)
    px, reps = c.B * c.w * c.h, 20
    say("")
    say("64 x 4096^2, level 4, Medium, Crossed")
    t_e, t_d = timed(c.encode, reps), timed(c.decode, reps)
    t_a = timed(c.composed, reps)
    t_b = timed(c.fused, reps)
    t_d3 = timed(c.copy3, reps)
    say("  hgi_encode_u8_dev alone %s, hgi_decode_u8_dev alone %s" % (us(t_e), us(t_d)))
    say("  (a) encode + decode            %s  %.2f Gpx/s" % (us(t_a), px / t_a[0] / 1e6))
    say("  (b) recon encode, packed       %s  %.2f Gpx/s" % (us(t_b), px / t_b[0] / 1e6))
    say("  (d) hgi_copy_u8_dev of 3 B/px  %s  %.0f GB/s" % (us(t_d3), 3 * px / t_d3[0] / 1e6))
    say("  (b) / (a) = %s; (b) / (d) = %.3fx; (b) / encode alone = %.3fx" % (mark(t_b[0] / t_a[0], 0.80), t_b[0] / t_d3[0], t_b[0] / t_e[0]))
    # (c): the same frames at pitch 4224 on all three sides (the image is laid out again; the composed route is not re-timed there)
    img = c.view(0, c.w).clone()
    c.view(0, c.pitch).copy_(img)
    del img
    torch.cuda.synchronize()
    t_c = timed(lambda: c.fused(c.pitch), reps)
    say("  (c) recon encode, pitch 4224   %s  %.2f Gpx/s; (c) / (b) = %.3fx; (c) / (a) = %.3fx"
        % (us(t_c), px / t_c[0] / 1e6, t_c[0] / t_b[0], t_c[0] / t_a[0]))
    c.free()
    e = Case(16384, 16384, 1, 8, 3, 16384)
    e.check()
    px = e.w * e.h
    say("")
    say("(e) one 16384^2, level 8, High, Crossed (C4)")
    t_a, t_b = timed(e.composed, reps), timed(e.fused, reps)
    say("  (a) encode + decode            %s  %.2f Gpx/s" % (us(t_a), px / t_a[0] / 1e6))
    say("  (b) recon encode, packed       %s  %.2f Gpx/s" % (us(t_b), px / t_b[0] / 1e6))
    say("  (b) / (a) = %s" % mark(t_b[0] / t_a[0], 0.80))
    e.free()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    c = Case(4096, 4096, 64, 4, 2, 4096)
    c.check()
    for fn in (c.encode, c.decode, c.fused):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("64 x 4096^2: %d image bytes; 5 x hgi_encode_u8_dev, 5 x hgi_decode_u8_dev, 5 x hgi_recon_encode_u8_dev" % (c.B * c.w * c.h))
    c.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_recon.txt"))
