"""Requantize view lists (libhgi_qviews.so: hgi_qviews_requant_dev) against the two routes a list of mixed-size stored grids has
without them, device-resident, HIP events, one process, the legs of a comparison alternating within every round: writes
profiles/r24_requant_views.txt (or the path in argv[1]).  All workloads at level 4, Crossed, Lossless-encoded noise re-coded to
Medium; r07's workloads with r07's seed (tools/framelist_time.py, tools/views_time.py, tools/mviews_time.py, tools/tviews_time.py):
  * W1 mixed: 1024 grids, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 grids, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard as 64 views.
Sources and destinations lie in aligned_arena(shapes, 128): every row start of both sides on a 128-byte line.  Legs:
  (a) one hgi_requant_dev call per view;
  (b) hgi_views_decode_dev into a uint8 arena of the same layout plus hgi_views_encode_dev out of it: two launches, 4 B/px;
  (c) the one hgi_qviews_requant_dev launch, 2 B/px;
  (d) W3 only: the single hgi_requant_dev batch call on the same planes.
Every (c) result is checked against (a)'s bytes, arena against arena, before anything is timed, and (b)'s grids against (c)'s.
The plan of (c) is hgi_views_plan's: its host time (the best of five calls) is recorded, and is no new cost.  Nothing here
gates a test.
`--prof`: the workload of the counter passes instead -- W1 (b) and (c), five launches each after the check, nothing timed
(rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE in a pass of its own, never combined with tracing)."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_qviews as FQ, _ffi_requant as FR, _ffi_views as FV  # noqa: E402

L, LQ, LR, LV = _ffi.lib(), FQ.lib(), FR.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED = 4, 1, 0x48474937
LUT, LOSSLESS = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(2, LUT.ctypes.data, None))
_ffi.check(L.hgi_linear_lut(0, LOSSLESS.ctypes.data, None))
assert (LOSSLESS == np.arange(256)).all() and not (LUT == np.arange(256)).all()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps, rounds=5):
    """Median and minimum ms per call of each leg (reps[k] calls of leg k in a window); the legs take turns inside every round."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps[k]):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / reps[k])
    return [(float(np.median(m)), float(min(m))) for m in ms]


def stream():
    return _ffi._vp(torch.cuda.current_stream().cuda_stream or 0)


def plan_of(pairs):
    """hgi_views_plan of [(src, dst, w, h, sp, dp), ...]: (info, device blob, host microseconds: the best of five calls)."""
    n = len(pairs)
    arr = (FV.ViewPair * n)(*[FV.ViewPair(*p) for p in pairs])
    size = LV.hgi_views_plan_bytes(n)
    host = np.zeros(size, np.uint8)
    info = FV.ViewsInfo()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        st = LV.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
        best = min(best, (time.perf_counter() - t0) * 1e6)
        FV.check(st)
    return info, torch.from_numpy(host[:int(info.plan_bytes)].copy()).cuda(), best


class Grids:
    """The stored grids of a workload -- noise images encoded with the Lossless table at L4 Crossed -- in aligned_arena(shapes,
    128), the uint8 arena of (b), the three destination arenas of the same layout, and the plans."""

    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.px = sum(w * h for w, h in shapes)
        self.bytes, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        arena = lambda fill: torch.full((self.bytes,), fill, dtype=torch.uint8, device="cuda")      # noqa: E731
        self.src, self.tmp = arena(0), arena(0)
        self.out_a, self.out_b, self.out_c = arena(0xA5), arena(0xA5), arena(0xA5)
        assert all(t.data_ptr() % 128 == 0 for t in (self.src, self.tmp, self.out_a, self.out_b, self.out_c))
        # the noise images into (b)'s arena, frame by frame, then one view-list encode under the Lossless table: the stored grids
        packed = torch.empty(max(w * h for w, h in shapes), dtype=torch.uint8, device="cuda")
        for i, ((w, h), (o, p)) in enumerate(zip(shapes, self.places)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, i, w, h, packed.data_ptr(), 1, w * h))
            self.tmp[o:o + h * p].view(h, p)[:, :w].copy_(packed[:w * h].view(h, w))
        ptr = lambda t: [t.data_ptr() + o for o, _ in self.places]      # noqa: E731
        pairs = lambda a, b: [(s, d, w, h, p, p) for s, d, (w, h), (_, p) in zip(ptr(a), ptr(b), shapes, self.places)]      # noqa: E731
        info, blob, _ = plan_of(pairs(self.tmp, self.src))
        FV.check(LV.hgi_views_encode_dev(stream(), blob.data_ptr(), ctypes.addressof(info), LEVELS, INTERP, LOSSLESS.ctypes.data))
        torch.cuda.synchronize()
        self.tmp.zero_()
        self.plan_dec = plan_of(pairs(self.src, self.tmp))
        self.plan_enc = plan_of(pairs(self.tmp, self.out_b))
        self.plan_c = plan_of(pairs(self.src, self.out_c))
        self.host_us = self.plan_c[2]
        self.calls = [(s, p, w, h, d, p) for s, d, (w, h), (_, p) in zip(ptr(self.src), ptr(self.out_a), shapes, self.places)]
        torch.cuda.synchronize()

    def leg_a(self):
        s, f, lut = stream(), LR.hgi_requant_dev, LUT.ctypes.data
        for src, sp, w, h, dst, dp in self.calls:
            st = f(s, src, sp, w, h, LEVELS, INTERP, lut, dst, dp, 1, 0, 0)
            if st:
                FR.check(st)

    def leg_b(self):
        FV.check(LV.hgi_views_decode_dev(stream(), self.plan_dec[1].data_ptr(), ctypes.addressof(self.plan_dec[0]), LEVELS, INTERP))
        FV.check(LV.hgi_views_encode_dev(stream(), self.plan_enc[1].data_ptr(), ctypes.addressof(self.plan_enc[0]), LEVELS, INTERP, LUT.ctypes.data))

    def leg_c(self):
        FQ.check(LQ.hgi_qviews_requant_dev(stream(), self.plan_c[1].data_ptr(), ctypes.addressof(self.plan_c[0]), LEVELS, INTERP, LUT.ctypes.data))

    def leg_d(self):      # W3: one batch call on the same planes, into (a)'s arena
        n = 4096 * 4096
        FR.check(LR.hgi_requant_dev(stream(), self.src.data_ptr(), 4096, 4096, 4096, LEVELS, INTERP, LUT.ctypes.data, self.out_a.data_ptr(), 4096,
                                    self.n, n, n))

    def check(self):
        """(c) against (a), arena against arena (both filled with one sentinel first); then (b)'s arena against (c)'s."""
        before = self.src.clone() if self.bytes < (1 << 29) else None
        self.leg_a()
        self.leg_c()
        self.leg_b()
        torch.cuda.synchronize()
        assert torch.equal(self.out_c, self.out_a), "%s: the one launch differs from one requantize per view" % self.name
        assert int((self.out_c != 0xA5).sum()) >= self.px // 2, "nothing was written"
        assert torch.equal(self.out_b, self.out_c), "%s: decode + encode differs" % self.name
        assert before is None or torch.equal(before, self.src), "the sources were modified"
        if self.name == "W3":
            self.out_a.fill_(0xA5)
            self.leg_d()
            torch.cuda.synchronize()
            assert torch.equal(self.out_c, self.out_a), "W3: the one launch differs from the batch call"


def shapes_of():
    rng = np.random.default_rng(SEED)
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    return w1, w2, [(4096, 4096)] * 64


def main(path):
    say("# tools/qviews_time.py: requantize view lists against one requantize per view and against view-list decode + view-list encode;")
    say("# L%d Crossed, Lossless-encoded noise -> Medium, device-resident, HIP events, median (min) of 5 rounds," % LEVELS)
    say("# the legs alternating inside every round; seed 0x%x; %s; %s; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LQ.hgi_qviews_version().decode(), LR.hgi_requant_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) one hgi_requant_dev per view; (b) hgi_views_decode_dev into a uint8 arena + hgi_views_encode_dev, two launches; (c) the one")
    say("# hgi_qviews_requant_dev launch; (d) W3: the single hgi_requant_dev batch call on the same planes.  Both sides on 128-byte rows.")
    say("# Conditions, stated before measuring: (c)'s bytes equal (a)'s, checked first; W1, W2: (c) < (a) and (c) < (b); W3: (c) <= 1.15 x (d).")
    w1, w2, w3 = shapes_of()
    missed = []
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        g = Grids(name, shapes)
        g.check()
        say("")
        say("%s: %d grids, %.3f Gpx; arena %.3f GB a side; (c)'s bytes equal (a)'s and (b)'s; hgi_views_plan on the host: %.0f us (%d entries, blob %d bytes; the"
            % (name, g.n, g.px / 1e9, g.bytes / 1e9, g.host_us, g.n, g.plan_c[0].plan_bytes))
        say("  view lists' plan as it stands: no new plan cost)")
        legs = [g.leg_a, g.leg_b, g.leg_c] + ([g.leg_d] if name == "W3" else [])
        # windows of 10 ms and more: the per-view leg is thousands of launches a call, the one-launch legs get 20 calls
        t = timed(legs, [3 if g.n > 4096 else 5] + [20] * (len(legs) - 1))
        say("  (a) per view %.1f us (min %.1f); (b) decode + encode %.1f us (min %.1f); (c) one launch %.1f us (min %.1f), %.2f Gpx/s, %.2f GB/s at 2 B/px"
            % (t[0][0] * 1e3, t[0][1] * 1e3, t[1][0] * 1e3, t[1][1] * 1e3, t[2][0] * 1e3, t[2][1] * 1e3, g.px / t[2][0] / 1e6, g.px * 2 / t[2][0] / 1e6))
        say("    (a) / (c) = %.2fx; (b) / (c) = %.2fx; (c) / (b) = %.3fx (bytes predict 0.50x; the uniform launch stands at 0.671x, DESIGN 4.13)"
            % (t[0][0] / t[2][0], t[1][0] / t[2][0], t[2][0] / t[1][0]))
        if name == "W3":
            r = t[2][0] / t[3][0]
            say("    (d) batch call %.1f us (min %.1f); condition (c) <= 1.15x (d) -> %.3fx %s" % (t[3][0] * 1e3, t[3][1] * 1e3, r, "met" if r <= 1.15 else "MISSED"))
            if r > 1.15:
                missed.append("%s (c) <= 1.15x (d): %.3fx" % (name, r))
        else:
            for leg, k in (("(a)", 0), ("(b)", 1)):
                ok = t[2][0] < t[k][0]
                say("    condition (c) < %s on %s -> %s" % (leg, name, "met" if ok else "MISSED"))
                if not ok:
                    missed.append("%s (c) < %s" % (name, leg))
        del g
        torch.cuda.empty_cache()
    say("")
    say("conditions missed: %s" % ("; ".join(missed) if missed else "none"))
    say("FETCH_SIZE / WRITE_SIZE of W1 (b) and (c): not counted in this run (qviews_time.py --prof under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def prof():
    g = Grids("W1", shapes_of()[0])
    g.check()
    for fn in (g.leg_b, g.leg_c):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1: %d grids, %d px, arena %d bytes a side" % (g.n, g.px, g.bytes))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--prof":
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_requant_views.txt"))
