"""Recon view lists (libhgi_rviews.so: hgi_rviews_encode_dev) against the two routes a list of mixed-size frames has to its grids
and reconstructions without them, device-resident, HIP events, one process, the legs of a comparison alternating within every
round: writes profiles/r26_recon_views.txt (or the path in argv[1]).  All workloads at level 4, Crossed, noise encoded with the
Medium table; r07's workloads with r07's seed (tools/framelist_time.py, tools/views_time.py, tools/qviews_time.py):
  * W1 mixed: 1024 frames, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 frames, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard as 64 views.
Sources, grids and reconstructions lie in aligned_arena(shapes, 128): every row start of all three sides on a 128-byte line.
Legs:
  (a) one hgi_recon_encode_u8_dev call per view;
  (b) hgi_views_encode_dev plus hgi_views_decode_dev of the grids it wrote: two launches, 4 B/px;
  (c) the one hgi_rviews_encode_dev launch, 3 B/px;
  (d) W3 only: the single hgi_recon_encode_u8_dev batch call on the same planes.
Every (c) result is checked against (a)'s bytes, arena against arena on both outputs, before anything is timed, and (b)'s arenas
against (c)'s.  The host time of hgi_rviews_plan (the best of five calls) is recorded.  Nothing here gates a test.
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
from rustyhgi_amd import _ffi, _ffi_recon as FR, _ffi_rviews as FX, _ffi_views as FV  # noqa: E402

L, LX, LR, LV = _ffi.lib(), FX.lib(), FR.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED = 4, 1, 0x48474937
LUT = np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(2, LUT.ctypes.data, None))
assert not (LUT == np.arange(256)).all()
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


def views_plan_of(pairs):
    """hgi_views_plan of [(src, dst, w, h, sp, dp), ...]: (info, device blob)."""
    n = len(pairs)
    arr = (FV.ViewPair * n)(*[FV.ViewPair(*p) for p in pairs])
    size = LV.hgi_views_plan_bytes(n)
    host = np.zeros(size, np.uint8)
    info = FV.ViewsInfo()
    FV.check(LV.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info)))
    return info, torch.from_numpy(host[:int(info.plan_bytes)].copy()).cuda()


def rviews_plan_of(triples):
    """hgi_rviews_plan of [(src, grid, recon, w, h, sp, gp, rp), ...]: (info, device blob, host microseconds: the best of five calls)."""
    n = len(triples)
    arr = (FX.RViewTriple * n)(*[FX.RViewTriple(*t) for t in triples])
    size = LX.hgi_rviews_plan_bytes(n)
    host = np.zeros(size, np.uint8)
    info = FX.RViewsInfo()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        st = LX.hgi_rviews_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info))
        best = min(best, (time.perf_counter() - t0) * 1e6)
        FX.check(st)
    return info, torch.from_numpy(host[:int(info.plan_bytes)].copy()).cuda(), best


class Frames:
    """The frames of a workload -- noise -- in aligned_arena(shapes, 128), three pairs of output arenas of the same layout (grids
    and reconstructions of (a), (b) and (c)), and the plans."""

    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.px = sum(w * h for w, h in shapes)
        self.bytes, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        arena = lambda fill: torch.full((self.bytes,), fill, dtype=torch.uint8, device="cuda")      # noqa: E731
        self.src = arena(0)
        self.grid_a, self.recon_a, self.grid_b, self.recon_b, self.grid_c, self.recon_c = (arena(0xA5) for _ in range(6))
        assert all(t.data_ptr() % 128 == 0 for t in (self.src, self.grid_a, self.recon_a, self.grid_b, self.recon_b, self.grid_c, self.recon_c))
        packed = torch.empty(max(w * h for w, h in shapes), dtype=torch.uint8, device="cuda")
        for i, ((w, h), (o, p)) in enumerate(zip(shapes, self.places)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, i, w, h, packed.data_ptr(), 1, w * h))
            self.src[o:o + h * p].view(h, p)[:, :w].copy_(packed[:w * h].view(h, w))
        ptr = lambda t: [t.data_ptr() + o for o, _ in self.places]      # noqa: E731
        pairs = lambda a, b: [(s, d, w, h, p, p) for s, d, (w, h), (_, p) in zip(ptr(a), ptr(b), shapes, self.places)]      # noqa: E731
        self.plan_enc = views_plan_of(pairs(self.src, self.grid_b))
        self.plan_dec = views_plan_of(pairs(self.grid_b, self.recon_b))
        self.plan_c = rviews_plan_of([(s, g, r, w, h, p, p, p) for s, g, r, (w, h), (_, p) in zip(ptr(self.src), ptr(self.grid_c), ptr(self.recon_c), shapes, self.places)])
        self.host_us = self.plan_c[2]
        self.calls = [(s, p, w, h, g, r) for s, g, r, (w, h), (_, p) in zip(ptr(self.src), ptr(self.grid_a), ptr(self.recon_a), shapes, self.places)]
        torch.cuda.synchronize()

    def leg_a(self):
        s, f, lut = stream(), LR.hgi_recon_encode_u8_dev, LUT.ctypes.data
        for src, p, w, h, grid, recon in self.calls:
            st = f(s, src, p, w, h, LEVELS, INTERP, lut, grid, p, recon, p, 1, 0, 0, 0)
            if st:
                FR.check(st)

    def leg_b(self):
        FV.check(LV.hgi_views_encode_dev(stream(), self.plan_enc[1].data_ptr(), ctypes.addressof(self.plan_enc[0]), LEVELS, INTERP, LUT.ctypes.data))
        FV.check(LV.hgi_views_decode_dev(stream(), self.plan_dec[1].data_ptr(), ctypes.addressof(self.plan_dec[0]), LEVELS, INTERP))

    def leg_c(self):
        FX.check(LX.hgi_rviews_encode_dev(stream(), self.plan_c[1].data_ptr(), ctypes.addressof(self.plan_c[0]), LEVELS, INTERP, LUT.ctypes.data))

    def leg_d(self):      # W3: one batch call on the same planes, into (a)'s arenas
        n = 4096 * 4096
        FR.check(LR.hgi_recon_encode_u8_dev(stream(), self.src.data_ptr(), 4096, 4096, 4096, LEVELS, INTERP, LUT.ctypes.data, self.grid_a.data_ptr(), 4096,
                                            self.recon_a.data_ptr(), 4096, self.n, n, n, n))

    def check(self):
        """(c) against (a), arena against arena on both outputs (all filled with one sentinel first); then (b)'s arenas against (c)'s."""
        before = self.src.clone() if self.bytes < (1 << 29) else None
        self.leg_a()
        self.leg_c()
        self.leg_b()
        torch.cuda.synchronize()
        assert torch.equal(self.grid_c, self.grid_a), "%s: the one launch's grids differ from one call per view" % self.name
        assert torch.equal(self.recon_c, self.recon_a), "%s: the one launch's reconstructions differ from one call per view" % self.name
        assert int((self.grid_c != 0xA5).sum()) >= self.px // 2 and int((self.recon_c != 0xA5).sum()) >= self.px // 2, "nothing was written"
        assert torch.equal(self.grid_b, self.grid_c) and torch.equal(self.recon_b, self.recon_c), "%s: encode + decode differs" % self.name
        assert before is None or torch.equal(before, self.src), "the sources were modified"
        if self.name == "W3":
            self.grid_a.fill_(0xA5)
            self.recon_a.fill_(0xA5)
            self.leg_d()
            torch.cuda.synchronize()
            assert torch.equal(self.grid_c, self.grid_a) and torch.equal(self.recon_c, self.recon_a), "W3: the one launch differs from the batch call"


def shapes_of():
    rng = np.random.default_rng(SEED)
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    return w1, w2, [(4096, 4096)] * 64


def main(path):
    say("# tools/rviews_time.py: recon view lists against one encode with reconstruction per view and against view-list encode + view-list decode;")
    say("# L%d Crossed, noise under Medium, device-resident, HIP events, median (min) of 5 rounds," % LEVELS)
    say("# the legs alternating inside every round; seed 0x%x; %s; %s; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LX.hgi_rviews_version().decode(), LR.hgi_recon_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) one hgi_recon_encode_u8_dev per view; (b) hgi_views_encode_dev + hgi_views_decode_dev, two launches; (c) the one")
    say("# hgi_rviews_encode_dev launch; (d) W3: the single hgi_recon_encode_u8_dev batch call on the same planes.  All three sides on 128-byte rows.")
    say("# Conditions, stated before measuring: (c)'s bytes equal (a)'s, checked first; W1, W2: (c) < (a) and (c) < (b); W3: (c) <= 1.15 x (d).")
    w1, w2, w3 = shapes_of()
    missed = []
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        g = Frames(name, shapes)
        g.check()
        say("")
        say("%s: %d frames, %.3f Gpx; arena %.3f GB a side; (c)'s bytes equal (a)'s and (b)'s on both outputs; hgi_rviews_plan on the host: %.0f us (%d entries, blob %d bytes)"
            % (name, g.n, g.px / 1e9, g.bytes / 1e9, g.host_us, g.n, g.plan_c[0].plan_bytes))
        legs = [g.leg_a, g.leg_b, g.leg_c] + ([g.leg_d] if name == "W3" else [])
        # windows of 10 ms and more: the per-view leg is thousands of launches a call, the one-launch legs get 20 calls
        t = timed(legs, [3 if g.n > 4096 else 5] + [20] * (len(legs) - 1))
        say("  (a) per view %.1f us (min %.1f); (b) encode + decode %.1f us (min %.1f); (c) one launch %.1f us (min %.1f), %.2f Gpx/s, %.2f GB/s at 3 B/px"
            % (t[0][0] * 1e3, t[0][1] * 1e3, t[1][0] * 1e3, t[1][1] * 1e3, t[2][0] * 1e3, t[2][1] * 1e3, g.px / t[2][0] / 1e6, g.px * 3 / t[2][0] / 1e6))
        say("    (a) / (c) = %.2fx; (b) / (c) = %.2fx; (c) / (b) = %.3fx (bytes predict 0.75x; the uniform launch stands at 0.750x, DESIGN 4.10)"
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
    say("FETCH_SIZE / WRITE_SIZE of W1 (b) and (c): not counted in this run (rviews_time.py --prof under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def prof():
    g = Frames("W1", shapes_of()[0])
    g.check()
    for fn in (g.leg_b, g.leg_c):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1: %d frames, %d px, arena %d bytes a side" % (g.n, g.px, g.bytes))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--prof":
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r26_recon_views.txt"))
