"""Requantize (hgi_requant_dev, libhgi_requant.so) against the route it replaces -- hgi_decode_u8_dev then hgi_encode_u8_dev of
libhgi_hip.so with the new table -- device-resident, one process, on the same planes (hgi_planes_alloc): writes
profiles/r15_requant.txt (or the path in argv[1]).  Clocks are settled by a burst of the uniform decode first; every figure is
the median (min) of 5 rounds timed with the ctx's own event pair (hgi_timer_start / hgi_timer_stop) on the one stream all calls
run on, around `reps` back-to-back calls.
  (a) the composed route: decode of the source grid, then encode of the image -- 4 B/px, two launches;
  (b) hgi_requant_dev, packed (both pitches == width) -- 2 B/px, one launch;
  (c) (b) with 4224-byte pitches on both sides;
  (d) hgi_copy_u8_dev moving the same 2 B/px, the same run's streaming yardstick;
  (e) C4's 16384^2 at level 8 High, (a) and (b).
64 x 4096^2, level 4, Medium, Crossed unless noted; the source grid is the Lossless encode of noise.  The fused result is
checked against the composed route's before it is timed.  FOUR planes, so that every launch reads one memory class and
writes another (hgi_planes_alloc separates neighbours): plane 1 the source grid, plane 2 the composed route's image, plane 3 its
grid, plane 0 the fused launch's grid and the copy's destination.  By bytes the expectation is (b) = 0.50 x (a); the record states the
ratio, nothing asserts it.
`--prof`: the launches of (a) and (b) alone, five times each after the check, nothing timed (for a counter pass of its own:
rocprofv3 --pmc FETCH_SIZE WRITE_SIZE, never combined with tracing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_requant  # noqa: E402
from rustyhgi_amd.planes import Planes  # noqa: E402

L = _ffi.lib()
R = _ffi_requant.lib()
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


class Case:
    """`batch` frames of w x h in four planes placed by the library -- plane 1 the source grid (the Lossless encode of noise),
    plane 2 the decoded image of the composed route, plane 3 its grid, plane 0 the fused launch's grid -- each large enough for
    rows `pitch` bytes apart.  Every launch timed here goes from a plane to a neighbour of it: 1 -> 2, 2 -> 3, 1 -> 0."""

    def __init__(self, w, h, batch, levels, quant, pitch):
        self.w, self.h, self.B, self.levels, self.pitch = w, h, batch, levels, pitch
        self.lut = lut_of(quant)
        self.planes = Planes(ctx, batch * h * pitch, 4)
        self.p = self.planes.pointers
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, w, h, self.p[0], batch, w * h))
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.p[0], w, h, levels, INTERP, lut_of(0).ctypes.data, self.p[1], batch, w * h))
        torch.cuda.synchronize()

    def view(self, i, pitch):
        t = self.planes.torch(i, (self.B, self.h, pitch))
        return t[:, :, :self.w]

    def decode(self):
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, self.p[1], self.w, self.h, self.levels, INTERP, self.p[2], self.B, self.w * self.h))

    def encode(self):
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.p[2], self.w, self.h, self.levels, INTERP, self.lut.ctypes.data, self.p[3], self.B,
                                       self.w * self.h))

    def composed(self):
        self.decode()
        self.encode()

    def fused(self, pitch=None):
        pitch = pitch or self.w
        _ffi_requant.check(R.hgi_requant_dev(STREAM or None, self.p[1], pitch, self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                             self.p[0], pitch, self.B, pitch * self.h, pitch * self.h))

    def copy2(self):
        _ffi.check(L.hgi_copy_u8_dev(ctx.handle, self.p[1], self.p[0], self.B * self.w * self.h))

    def check(self):
        """The fused launch's grid against the composed route's, packed and (if the planes hold it) pitched; the source grid
        must come back unchanged.  Leaves the planes packed."""
        src = self.view(1, self.w).clone()
        self.composed()
        torch.cuda.synchronize()
        want = self.view(3, self.w).clone()
        self.view(0, self.w).zero_()
        self.fused()
        torch.cuda.synchronize()
        assert torch.equal(self.view(0, self.w), want), "the fused grid differs from decode + encode"
        assert torch.equal(self.view(1, self.w), src), "the source grid was modified"
        if self.pitch != self.w:
            self.to_pitch(src)
            self.view(0, self.pitch).zero_()
            self.fused(self.pitch)
            torch.cuda.synchronize()
            assert torch.equal(self.view(0, self.pitch), want), "the pitched fused launch differs"
            self.view(1, self.w).copy_(src)
        del src, want
        torch.cuda.empty_cache()

    def to_pitch(self, src=None):
        """Lay the source grid out again at the padded pitch (back to front is not needed: `src` is a copy)."""
        src = self.view(1, self.w).clone() if src is None else src
        self.view(1, self.pitch).copy_(src)
        torch.cuda.synchronize()

    def free(self):
        self.planes.close()
        torch.cuda.empty_cache()


def settle(c):
    for _ in range(400):
        c.decode()
    torch.cuda.synchronize()


def main(path):
    say("# tools/requant_time.py: requantize (one launch, 2 B/px) against decode + encode (two launches, 4 B/px);")
    say("# device-resident, same planes (hgi_planes_alloc), hgi_timer_* events on one stream, median (min) of 5 rounds;")
    say("# %s; %s; torch %s" % (L.hgi_version().decode(), R.hgi_requant_version().decode(), torch.__version__))
    c = Case(4096, 4096, 64, 4, 2, 4224)
    say("# planes: %s (separated: %s); source = plane 1, image = plane 2, composed grid = plane 3, fused grid = plane 0"
        % (c.planes.report, c.planes.separated))
    c.check()
    settle(c)
    px, reps = c.B * c.w * c.h, 20
    say("")
    say("64 x 4096^2, level 4, Lossless-encoded noise -> Medium, Crossed")
    t_d, t_e = timed(c.decode, reps), timed(c.encode, reps)
    t_a = timed(c.composed, reps)
    t_b = timed(c.fused, reps)
    t_d2 = timed(c.copy2, reps)
    say("  hgi_decode_u8_dev alone %s, hgi_encode_u8_dev alone %s" % (us(t_d), us(t_e)))
    say("  (a) decode + encode            %s  %.2f Gpx/s" % (us(t_a), px / t_a[0] / 1e6))
    say("  (b) requantize, packed         %s  %.2f Gpx/s" % (us(t_b), px / t_b[0] / 1e6))
    say("  (d) hgi_copy_u8_dev of 2 B/px  %s  %.0f GB/s" % (us(t_d2), 2 * px / t_d2[0] / 1e6))
    say("  (b) / (a) = %.3fx (by bytes 0.50x); (b) / (d) = %.3fx; (b) / encode alone = %.3fx" % (t_b[0] / t_a[0], t_b[0] / t_d2[0], t_b[0] / t_e[0]))
    # (c): the same grids at pitch 4224 on both sides (the composed route is not re-timed there)
    c.to_pitch()
    t_c = timed(lambda: c.fused(c.pitch), reps)
    say("  (c) requantize, pitch 4224     %s  %.2f Gpx/s; (c) / (b) = %.3fx; (c) / (a) = %.3fx"
        % (us(t_c), px / t_c[0] / 1e6, t_c[0] / t_b[0], t_c[0] / t_a[0]))
    c.free()
    e = Case(16384, 16384, 1, 8, 3, 16384)
    say("")
    say("# planes: %s (separated: %s)" % (e.planes.report, e.planes.separated))
    e.check()
    px = e.w * e.h
    say("(e) one 16384^2, level 8, Lossless-encoded noise -> High, Crossed (C4)")
    t_a, t_b = timed(e.composed, reps), timed(e.fused, reps)
    say("  (a) decode + encode            %s  %.2f Gpx/s" % (us(t_a), px / t_a[0] / 1e6))
    say("  (b) requantize, packed         %s  %.2f Gpx/s" % (us(t_b), px / t_b[0] / 1e6))
    say("  (b) / (a) = %.3fx (by bytes 0.50x)" % (t_b[0] / t_a[0]))
    e.free()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    c = Case(4096, 4096, 64, 4, 2, 4096)
    c.check()
    for fn in (c.decode, c.encode, c.fused):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("64 x 4096^2: %d grid bytes; 5 x hgi_decode_u8_dev, 5 x hgi_encode_u8_dev, 5 x hgi_requant_dev" % (c.B * c.w * c.h))
    c.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_requant.txt"))
