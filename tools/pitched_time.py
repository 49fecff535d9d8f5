"""Pitched frames (hgi_encode_u8_pitched_dev / hgi_decode_u8_pitched_dev) against the composed route of the uniform calls -- a
2-D packing copy in front of the encode or behind the decode -- and against the uniform call itself, device-resident, one
process, the comparison route timed on the same planes: writes profiles/r08_pitched.txt (or the path in argv[1]).
Clocks are settled by a burst of the uniform call first; every figure is the median (min) of 5 rounds timed with the ctx's own
event pair (hgi_timer_start / hgi_timer_stop) around `reps` back-to-back calls.  Level 4, Medium, Crossed unless noted.
  * P1: 64 windows of 4096^2 inside 64 parents of 4224 x 4160 (pitch 4224; at (128, 32): rows start on a 128-B line, and again
        at (64, 32), the centred window, whose rows start mid-line), each direction, packed on the other side, against
        hipMemcpy2DAsync (one per frame) + the uniform call; torch's strided copy and the hgi_copy_u8_dev rate (the copy's floor,
        one linear stream of the same bytes) beside it;
  * P2: the same frames pitched on BOTH sides (window -> window) against the uniform 64 x 4096^2 call;
  * P3: pitch == width through the pitched entry points against the uniform call (the forward);
  * P4: 64 x (4090 wide x 4096 high) packed -- rows start mid-line; at the allocation's start and 16 bytes into it, which decides
        whether the uniform call keeps its buffer path -- against the same frames at pitch 4096 on a 256-B aligned base (no
        target: reported);
  * P5: one 16384^2 window of a 16512 x 16448 parent, level 8 High, against the uniform call;
  * P6: a 1920 x 1080 crop of a 3840 x 2160 frame, encode, and decode into the same window, against the lone 1080p frame.
Every pitched result is checked against the uniform call on the packed copy before it is timed.
`--prof`: P4's buffer-path launches (packed + 16 B and pitched, both directions) alone, five times each after the check,
nothing timed (rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE, one counter per pass, as tools/profile.sh does)."""
import ctypes
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
STREAM = torch.cuda.current_stream().cuda_stream
ctx.set_stream(STREAM)
INTERP, SEED = 1, 0x48474938
lines = []


def hip_runtime():
    """The HIP runtime this process already holds (torch's copy when torch ships one): hipMemcpy2DAsync for the composed route."""
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    lib = ctypes.CDLL(rt if os.path.exists(rt) else "libamdhip64.so")
    lib.hipMemcpy2DAsync.restype = ctypes.c_int
    lib.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    return lib


HIP = hip_runtime()
D2D = 3


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


def copy2d(dst, dpitch, dfs, src, spitch, sfs, w, h, batch):
    for f in range(batch):
        rc = HIP.hipMemcpy2DAsync(dst + f * dfs, dpitch, src + f * sfs, spitch, w, h, D2D, STREAM)
        assert rc == 0, rc


class Case:
    """`batch` windows of w x h at (x0, y0) of parents pw x ph: an input parent, a grid parent, an output parent (noise or
    zeros), and packed planes beside them."""

    def __init__(self, w, h, pw, ph, batch, levels, quant, x0=64, y0=32):
        self.w, self.h, self.pw, self.ph, self.B, self.levels = w, h, pw, ph, batch, levels
        self.lut = lut_of(quant)
        self.off = y0 * pw + x0
        self.pin = torch.empty((batch, ph, pw), dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, 0, pw, ph, self.pin.data_ptr(), batch, pw * ph))
        self.pgrid = torch.zeros_like(self.pin)
        self.pout = torch.zeros_like(self.pin)
        self.img = self.pin[:, y0:y0 + h, x0:x0 + w].contiguous()
        self.grid = torch.empty_like(self.img)
        self.out = torch.empty_like(self.img)
        self.tmp = torch.empty_like(self.img)
        self.x0, self.y0 = x0, y0

    def win(self, t):
        return t[:, self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]

    # the uniform calls on the packed planes
    def enc_uniform(self, src=None, dst=None):
        src, dst = self.img if src is None else src, self.grid if dst is None else dst
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, src.data_ptr(), self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                       dst.data_ptr(), self.B, self.w * self.h))

    def dec_uniform(self, src=None, dst=None):
        src, dst = self.grid if src is None else src, self.out if dst is None else dst
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, src.data_ptr(), self.w, self.h, self.levels, INTERP, dst.data_ptr(), self.B,
                                       self.w * self.h))

    # the pitched calls: (pointer, pitch, frame stride) per side
    def side(self, t, pitched):
        return (t.data_ptr() + self.off, self.pw, self.pw * self.ph) if pitched else (t.data_ptr(), self.w, self.w * self.h)

    def enc_pitched(self, src, dst):
        (s, sp, sfs), (d, dp, dfs) = src, dst
        _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, s, sp, self.w, self.h, self.levels, INTERP, self.lut.ctypes.data, d, dp, self.B,
                                               sfs, dfs))

    def dec_pitched(self, src, dst):
        (s, sp, sfs), (d, dp, dfs) = src, dst
        _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, s, sp, self.w, self.h, self.levels, INTERP, d, dp, self.B, sfs, dfs))

    def pack(self, parent, packed):          # parent window -> packed plane
        copy2d(packed.data_ptr(), self.w, self.w * self.h, parent.data_ptr() + self.off, self.pw, self.pw * self.ph, self.w, self.h, self.B)

    def unpack(self, packed, parent):        # packed plane -> parent window
        copy2d(parent.data_ptr() + self.off, self.pw, self.pw * self.ph, packed.data_ptr(), self.w, self.w * self.h, self.w, self.h, self.B)

    def check(self):
        """The pitched calls' bytes (each layout that is timed) against the uniform calls on the packed copy."""
        self.enc_uniform()
        self.dec_uniform()
        pi, pg, po = self.side(self.pin, True), self.side(self.pgrid, True), self.side(self.pout, True)
        self.enc_pitched(pi, self.side(self.tmp, False))
        torch.cuda.synchronize()
        assert torch.equal(self.tmp, self.grid), "pitched -> packed encode differs"
        self.enc_pitched(pi, pg)
        self.dec_pitched(pg, po)
        torch.cuda.synchronize()
        assert torch.equal(self.win(self.pgrid), self.grid) and torch.equal(self.win(self.pout), self.out), "window -> window differs"
        self.pout.zero_()
        self.dec_pitched(self.side(self.grid, False), po)
        torch.cuda.synchronize()
        assert torch.equal(self.win(self.pout), self.out), "packed -> pitched decode differs"

    def free(self):
        del self.pin, self.pgrid, self.pout, self.img, self.grid, self.out, self.tmp
        torch.cuda.empty_cache()


def mark(ratio, target):
    return "%.3fx (target <= %.2fx: %s)" % (ratio, target, "met" if ratio <= target else "MISSED")


def settle(c):
    for _ in range(400):
        c.dec_uniform()
    torch.cuda.synchronize()


def p1_p2_p3(x0, y0, first, reps=20):
    c = Case(4096, 4096, 4224, 4160, 64, 4, 2, x0=x0, y0=y0)
    c.check()
    settle(c)
    say("")
    say("== windows at (%d, %d) of their parents: rows start %s ==" % (x0, y0, "on a 128-B line" if x0 % 128 == 0 else "mid-line (%d B into one)" % (x0 % 128)))
    px = c.B * c.w * c.h
    pi, pg, po = c.side(c.pin, True), c.side(c.pgrid, True), c.side(c.pout, True)
    ki, kg, ko = c.side(c.img, False), c.side(c.grid, False), c.side(c.out, False)
    t_ue, t_ud = timed(c.enc_uniform, reps), timed(c.dec_uniform, reps)
    say("uniform 64 x 4096^2: encode %s, decode %s  (%.2f / %.2f Gpx/s)" % (us(t_ue), us(t_ud), px / t_ue[0] / 1e6, px / t_ud[0] / 1e6))
    t_pack = timed(lambda: c.pack(c.pin, c.tmp), reps)
    t_unpack = timed(lambda: c.unpack(c.tmp, c.pout), reps)
    t_tpack = timed(lambda: c.tmp.copy_(c.win(c.pin)), reps)
    t_tunpack = timed(lambda: c.win(c.pout).copy_(c.tmp), reps)
    t_lin = timed(lambda: _ffi.check(L.hgi_copy_u8_dev(ctx.handle, c.img.data_ptr(), c.tmp.data_ptr(), px)), reps)
    say("packing copy of the 64 windows: hipMemcpy2DAsync x 64 %s in, %s out; torch strided copy %s in, %s out; hgi_copy_u8_dev of the "
        "same bytes (linear: the floor) %s" % (us(t_pack), us(t_unpack), us(t_tpack), us(t_tunpack), us(t_lin)))
    say("")
    say("P1: 64 windows of 4096^2 in parents of 4224 x 4160, the other side packed")
    t_pe = timed(lambda: c.enc_pitched(pi, kg), reps)

    def comp_enc():
        c.pack(c.pin, c.tmp)
        c.enc_uniform(src=c.tmp)

    def comp_enc_t():
        c.tmp.copy_(c.win(c.pin))
        c.enc_uniform(src=c.tmp)
    t_ce, t_cet = timed(comp_enc, reps), timed(comp_enc_t, reps)
    best = min(t_ce[0], t_cet[0])
    say("  encode pitched -> packed %s; composed: hipMemcpy2DAsync + uniform %s, torch copy + uniform %s" % (us(t_pe), us(t_ce), us(t_cet)))
    say("    pitched / composed (hipMemcpy2DAsync) = %s; / the faster composed route = %s; / copy floor + uniform (%.1f us) = %.3fx"
        % (mark(t_pe[0] / t_ce[0], 0.60), mark(t_pe[0] / best, 0.60), (t_lin[0] + t_ue[0]) * 1e3, t_pe[0] / (t_lin[0] + t_ue[0])))
    t_pd = timed(lambda: c.dec_pitched(kg, po), reps)

    def comp_dec():
        c.dec_uniform(dst=c.tmp)
        c.unpack(c.tmp, c.pout)

    def comp_dec_t():
        c.dec_uniform(dst=c.tmp)
        c.win(c.pout).copy_(c.tmp)
    t_cd, t_cdt = timed(comp_dec, reps), timed(comp_dec_t, reps)
    best = min(t_cd[0], t_cdt[0])
    say("  decode packed -> pitched %s; composed: uniform + hipMemcpy2DAsync %s, uniform + torch copy %s" % (us(t_pd), us(t_cd), us(t_cdt)))
    say("    pitched / composed (hipMemcpy2DAsync) = %s; / the faster composed route = %s; / uniform + copy floor (%.1f us) = %.3fx"
        % (mark(t_pd[0] / t_cd[0], 0.60), mark(t_pd[0] / best, 0.60), (t_lin[0] + t_ud[0]) * 1e3, t_pd[0] / (t_lin[0] + t_ud[0])))
    say("")
    say("P2: the same frames pitched on both sides (window -> window) against the uniform call, same run")
    t_e2, t_d2 = timed(lambda: c.enc_pitched(pi, pg), reps), timed(lambda: c.dec_pitched(pg, po), reps)
    t_ue2, t_ud2 = timed(c.enc_uniform, reps), timed(c.dec_uniform, reps)
    say("  encode %s against %s: %s" % (us(t_e2), us(t_ue2), mark(t_e2[0] / t_ue2[0], 1.15)))
    say("  decode %s against %s: %s" % (us(t_d2), us(t_ud2), mark(t_d2[0] / t_ud2[0], 1.15)))
    if not first:
        c.free()
        return
    say("")
    say("P3: pitch == width through the pitched entry points (the call forwards to the uniform call)")
    t_e3, t_d3 = timed(lambda: c.enc_pitched(ki, kg), reps), timed(lambda: c.dec_pitched(kg, ko), reps)
    t_ue3, t_ud3 = timed(c.enc_uniform, reps), timed(c.dec_uniform, reps)
    say("  encode %s against %s: %.3fx; decode %s against %s: %.3fx (target: equal within run-to-run noise)"
        % (us(t_e3), us(t_ue3), t_e3[0] / t_ue3[0], us(t_d3), us(t_ud3), t_d3[0] / t_ud3[0]))
    c.free()


class P4:
    """64 x (4090 x 4096): packed (rows start mid-line; the uniform call) and at pitch 4096 on an aligned base (the pitched call)."""

    def __init__(self):
        self.w, self.h, self.B, self.levels, self.p = 4090, 4096, 64, 4, 4096
        self.lut = lut_of(2)
        w, h, B, p = self.w, self.h, self.B, self.p
        self.pin = torch.empty((B, h, p), dtype=torch.uint8, device="cuda")
        _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED + 4, 0, p, h, self.pin.data_ptr(), B, p * h))
        self.pgrid, self.pout = torch.zeros_like(self.pin), torch.zeros_like(self.pin)
        self.img = self.pin[:, :, :w].contiguous()
        self.grid, self.out = torch.empty_like(self.img), torch.empty_like(self.img)
        # the same packed frames 16 bytes into their allocations: the batch then does not end on a page boundary, so the uniform call
        # may read the three bytes behind its last row (fused_geom) and keeps its buffer path on these 4090-byte rows
        n = B * w * h
        self.flat = [torch.empty(n + 4096, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.off16 = [t[16:16 + n] for t in self.flat]
        self.off16[0].copy_(self.img.reshape(-1))

    def enc_packed(self):
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.img.data_ptr(), self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                       self.grid.data_ptr(), self.B, self.w * self.h))

    def dec_packed(self):
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, self.grid.data_ptr(), self.w, self.h, self.levels, INTERP, self.out.data_ptr(), self.B,
                                       self.w * self.h))

    def enc_packed16(self):
        _ffi.check(L.hgi_encode_u8_dev(ctx.handle, self.off16[0].data_ptr(), self.w, self.h, self.levels, INTERP, self.lut.ctypes.data,
                                       self.off16[1].data_ptr(), self.B, self.w * self.h))

    def dec_packed16(self):
        _ffi.check(L.hgi_decode_u8_dev(ctx.handle, self.off16[1].data_ptr(), self.w, self.h, self.levels, INTERP, self.off16[2].data_ptr(),
                                       self.B, self.w * self.h))

    def enc_pitched(self):
        _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, self.pin.data_ptr(), self.p, self.w, self.h, self.levels, INTERP,
                                               self.lut.ctypes.data, self.pgrid.data_ptr(), self.p, self.B, self.p * self.h, self.p * self.h))

    def dec_pitched(self):
        _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, self.pgrid.data_ptr(), self.p, self.w, self.h, self.levels, INTERP,
                                               self.pout.data_ptr(), self.p, self.B, self.p * self.h, self.p * self.h))

    def check(self):
        self.enc_packed()
        self.dec_packed()
        self.enc_pitched()
        self.dec_pitched()
        self.enc_packed16()
        self.dec_packed16()
        torch.cuda.synchronize()
        assert torch.equal(self.pgrid[:, :, :self.w], self.grid) and torch.equal(self.pout[:, :, :self.w], self.out), "P4 differs"
        assert torch.equal(self.off16[1], self.grid.reshape(-1)) and torch.equal(self.off16[2], self.out.reshape(-1)), "P4 (+16) differs"


def p4(reps=20):
    c = P4()
    c.check()
    say("")
    say("P4: 64 x (4090 wide x 4096 high): packed (rows start mid-line), the uniform call, against pitch 4096 on a 256-B aligned base")
    say("    (packed at the allocation's start the batch ends on a page boundary: the three-byte tail cannot be granted and the uniform")
    say("     call takes its byte-checked path; 16 bytes in it keeps the buffer path -- that pair is the cost of the mid-line rows alone)")
    t_ep, t_dp = timed(c.enc_packed, reps), timed(c.dec_packed, reps)
    t_e16, t_d16 = timed(c.enc_packed16, reps), timed(c.dec_packed16, reps)
    t_ea, t_da = timed(c.enc_pitched, reps), timed(c.dec_pitched, reps)
    say("  encode packed %s, packed + 16 B %s, pitched %s: pitched / packed = %.3fx, pitched / packed + 16 B = %.3fx (no target: reported)"
        % (us(t_ep), us(t_e16), us(t_ea), t_ea[0] / t_ep[0], t_ea[0] / t_e16[0]))
    say("  decode packed %s, packed + 16 B %s, pitched %s: pitched / packed = %.3fx, pitched / packed + 16 B = %.3fx (no target: reported)"
        % (us(t_dp), us(t_d16), us(t_da), t_da[0] / t_dp[0], t_da[0] / t_d16[0]))
    del c
    torch.cuda.empty_cache()


def p5(reps=20):
    c = Case(16384, 16384, 16512, 16448, 1, 8, 3, x0=128, y0=32)
    c.check()
    pi, pg, po = c.side(c.pin, True), c.side(c.pgrid, True), c.side(c.pout, True)
    say("")
    say("P5: one 16384^2 window at (128, 32) of a 16512 x 16448 parent, level 8 High, pitched on both sides against the uniform call")
    t_e, t_d = timed(lambda: c.enc_pitched(pi, pg), reps), timed(lambda: c.dec_pitched(pg, po), reps)
    t_ue, t_ud = timed(c.enc_uniform, reps), timed(c.dec_uniform, reps)
    say("  encode %s against %s: %s" % (us(t_e), us(t_ue), mark(t_e[0] / t_ue[0], 1.15)))
    say("  decode %s against %s: %s" % (us(t_d), us(t_ud), mark(t_d[0] / t_ud[0], 1.15)))
    c.free()


def p6(reps=200):
    c = Case(1920, 1080, 3840, 2160, 1, 4, 2, x0=960, y0=540)
    c.check()
    pi, pg, po = c.side(c.pin, True), c.side(c.pgrid, True), c.side(c.pout, True)
    say("")
    say("P6: a 1920 x 1080 crop at (960, 540) of a 3840 x 2160 frame, encode, and decode into the same window, against the lone "
        "1080p frame (launch-bound: reported)")
    t_e, t_d = timed(lambda: c.enc_pitched(pi, pg), reps), timed(lambda: c.dec_pitched(pg, po), reps)
    t_ue, t_ud = timed(c.enc_uniform, reps), timed(c.dec_uniform, reps)
    say("  encode %s against %s: %.3fx; decode %s against %s: %.3fx"
        % (us(t_e), us(t_ue), t_e[0] / t_ue[0], us(t_d), us(t_ud), t_d[0] / t_ud[0]))
    c.free()


def main(path):
    say("# tools/pitched_time.py: pitched frames against the composed route (packing copy + uniform call) and the uniform call;")
    say("# device-resident, hgi_timer_* events on the ctx stream, median (min) of 5 rounds; %s; torch %s"
        % (L.hgi_version().decode(), torch.__version__))
    p1_p2_p3(128, 32, True)
    p1_p2_p3(64, 32, False)
    p4()
    p5()
    p6()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    c = P4()
    c.check()
    for fn in (c.enc_packed16, c.enc_pitched, c.dec_packed16, c.dec_pitched):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("P4: 64 x 4090 x 4096, %d image bytes per direction and side" % (c.B * c.w * c.h))


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_pitched.txt"))
