"""Scaled view lists (libhgi_sviews.so: hgi_sviews_decode_dev) against the routes a list of mixed-size stored grids has without
them, device-resident, HIP events, one process, the legs of a comparison alternating within every round: writes
profiles/r25_scaled_views.txt (or the path in argv[1]).  All workloads at level 4, Crossed, Lossless-encoded noise, at shifts 1, 2
and 3; r07's workloads with r07's seed (tools/framelist_time.py, tools/views_time.py, tools/qviews_time.py):
  * W1 mixed: 1024 grids, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 grids, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard as 64 views.
Grids and images lie in aligned_arena(shapes, 128): every row start of both sides on a 128-byte line.  Legs, per shift:
  (a) one hgi_decode_scaled_u8_dev per grid -- that call takes packed grids only, so it reads a packed copy of the same grids
      and writes into an arena of (c)'s layout;
  (b) hgi_views_decode_dev at full resolution alone, into a full-size arena: the floor of any decode-then-subsample route;
  (c) the one hgi_sviews_decode_dev launch;
  (d) W3 only: the uniform hgi_decode_scaled_u8_dev batch call on the same planes.
Every (c) result is checked against (a)'s bytes, arena against arena, before anything is timed.  The host time of
hgi_sviews_plan (the best of five calls) is recorded per list.  Nothing here gates a test.
`--prof`: the workload of the counter passes instead -- W1 (b) and (c) at shift 1, five launches each after the check, nothing
timed (rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE in a pass of its own, never combined with tracing)."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi, _ffi_sviews as FS, _ffi_views as FV  # noqa: E402

L, LS, LV = _ffi.lib(), FS.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED, SHIFTS = 4, 1, 0x48474937, (1, 2, 3)
BYTES = {1: 0.375, 2: 0.15625, 3: 0.0703125}      # (1 / 2^s + 1 / 4^s) / 2: (c)'s bytes over (b)'s 2 B/px
LOSSLESS = np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(0, LOSSLESS.ctypes.data, None))
assert (LOSSLESS == np.arange(256)).all()
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
    n = len(pairs)
    arr = (FV.ViewPair * n)(*[FV.ViewPair(*p) for p in pairs])
    size = LV.hgi_views_plan_bytes(n)
    host = np.zeros(size, np.uint8)
    info = FV.ViewsInfo()
    FV.check(LV.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(info)))
    return info, torch.from_numpy(host[:int(info.plan_bytes)].copy()).cuda()


def sviews_plan_of(pairs, shift):
    """hgi_sviews_plan of [(src, dst, w, h, sp, dp), ...]: (info, device blob, host microseconds: the best of five calls)."""
    n = len(pairs)
    arr = (FS.SViewPair * n)(*[FS.SViewPair(*p) for p in pairs])
    size = LS.hgi_sviews_plan_bytes(n)
    host = np.zeros(size, np.uint8)
    info = FS.SViewsInfo()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        st = LS.hgi_sviews_plan(ctypes.addressof(arr), n, shift, host.ctypes.data, size, ctypes.addressof(info))
        best = min(best, (time.perf_counter() - t0) * 1e6)
        FS.check(st)
    return info, torch.from_numpy(host[:int(info.plan_bytes)].copy()).cuda(), best


class Grids:
    """The stored grids of a workload -- noise images encoded with the Lossless table at L4 Crossed -- in aligned_arena(shapes,
    128) and once more packed, one behind the other, for (a); the full-size arena of (b); per shift the two image arenas of
    aligned_arena(scaled shapes, 128) and the plan of (c)."""

    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.px = sum(w * h for w, h in shapes)
        self.bytes, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        arena = lambda size, fill: torch.full((size,), fill, dtype=torch.uint8, device="cuda")      # noqa: E731
        self.src, self.full = arena(self.bytes, 0), arena(self.bytes, 0)
        self.packed = arena(self.px, 0)
        ptr = lambda t, places: [t.data_ptr() + o for o, _ in places]      # noqa: E731
        # the noise images into (b)'s arena, frame by frame, then one view-list encode under the Lossless table: the stored grids
        tmp = torch.empty(max(w * h for w, h in shapes), dtype=torch.uint8, device="cuda")
        for i, ((w, h), (o, p)) in enumerate(zip(shapes, self.places)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, i, w, h, tmp.data_ptr(), 1, w * h))
            self.full[o:o + h * p].view(h, p)[:, :w].copy_(tmp[:w * h].view(h, w))
        full_pairs = lambda a, b: [(s, d, w, h, p, p) for s, d, (w, h), (_, p) in zip(ptr(a, self.places), ptr(b, self.places), shapes, self.places)]      # noqa: E731
        info, blob = views_plan_of(full_pairs(self.full, self.src))
        FV.check(LV.hgi_views_encode_dev(stream(), blob.data_ptr(), ctypes.addressof(info), LEVELS, INTERP, LOSSLESS.ctypes.data))
        torch.cuda.synchronize()
        self.full.zero_()
        at, self.packed_at = 0, []
        for (w, h), (o, p) in zip(shapes, self.places):
            self.packed[at:at + w * h].view(h, w).copy_(self.src[o:o + h * p].view(h, p)[:, :w])
            self.packed_at.append(self.packed.data_ptr() + at)
            at += w * h
        self.plan_b = views_plan_of(full_pairs(self.src, self.full))
        self.at = {}
        for s in SHIFTS:
            sshapes = [(-(-w >> s), -(-h >> s)) for w, h in shapes]
            size, places = H.aligned_arena([(h, w) for w, h in sshapes], 128)
            out_a, out_c = arena(size, 0xA5), arena(size, 0xA5)
            pairs = [(a, d, w, h, p, dp) for a, d, (w, h), (_, p), (_, dp) in zip(ptr(self.src, self.places), ptr(out_c, places), shapes, self.places, places)]
            calls = [(a, w, h, d, dp) for a, d, (w, h), (_, dp) in zip(self.packed_at, ptr(out_a, places), shapes, places)]
            self.at[s] = dict(out_a=out_a, out_c=out_c, plan=sviews_plan_of(pairs, s), calls=calls, spx=sum(w * h for w, h in sshapes), places=places, sshapes=sshapes)
        torch.cuda.synchronize()

    def leg_a(self, s):
        f, c = L.hgi_decode_scaled_u8_dev, ctx.handle
        for src, w, h, dst, dp in self.at[s]["calls"]:
            st = f(c, src, w, h, LEVELS, INTERP, s, dst, dp, 1, 0, 0)
            if st:
                _ffi.check(st)

    def leg_b(self):
        FV.check(LV.hgi_views_decode_dev(stream(), self.plan_b[1].data_ptr(), ctypes.addressof(self.plan_b[0]), LEVELS, INTERP))

    def leg_c(self, s):
        info, blob, _ = self.at[s]["plan"]
        FS.check(LS.hgi_sviews_decode_dev(stream(), blob.data_ptr(), ctypes.addressof(info), LEVELS, INTERP))

    def leg_d(self, s):      # W3: the uniform batch call on the same planes (4096-byte rows are packed rows), into (a)'s arena
        n, m = 4096 * 4096, (4096 >> s) * (4096 >> s)
        _ffi.check(L.hgi_decode_scaled_u8_dev(ctx.handle, self.src.data_ptr(), 4096, 4096, LEVELS, INTERP, s, self.at[s]["out_a"].data_ptr(), 4096 >> s, self.n, n, m))

    def check(self, s):
        """(c) against (a), arena against arena (both filled with one sentinel first); on W1 also against (b)'s full decode,
        subsampled; on W3 against the batch call."""
        d = self.at[s]
        self.leg_a(s)
        self.leg_c(s)
        torch.cuda.synchronize()
        assert torch.equal(d["out_c"], d["out_a"]), "%s s%d: the one launch differs from one scaled decode per grid" % (self.name, s)
        assert int((d["out_c"] != 0xA5).sum()) >= d["spx"] // 2, "nothing was written"
        if self.name == "W1":
            self.leg_b()
            torch.cuda.synchronize()
            for (w, h), (o, p), (sw, sh), (so, sp) in list(zip(self.shapes, self.places, d["sshapes"], d["places"]))[:64]:
                want = self.full[o:o + h * p].view(h, p)[:, :w][::1 << s, ::1 << s]
                assert torch.equal(d["out_c"][so:so + sh * sp].view(sh, sp)[:, :sw], want), "%s s%d: differs from the full decode's lattice" % (self.name, s)
        if self.name == "W3":
            d["out_a"].fill_(0xA5)
            self.leg_d(s)
            torch.cuda.synchronize()
            assert torch.equal(d["out_c"], d["out_a"]), "W3 s%d: the one launch differs from the batch call" % s


def shapes_of():
    rng = np.random.default_rng(SEED)
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    return w1, w2, [(4096, 4096)] * 64


def main(path):
    say("# tools/sviews_time.py: scaled view lists against one scaled decode per grid and against the full-resolution view-list decode;")
    say("# L%d Crossed, Lossless-encoded noise, shifts 1, 2, 3, device-resident, HIP events, median (min) of 5 rounds," % LEVELS)
    say("# the legs alternating inside every round; seed 0x%x; %s; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LS.hgi_sviews_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) one hgi_decode_scaled_u8_dev per grid, from a packed copy; (b) hgi_views_decode_dev at full resolution alone; (c) the one")
    say("# hgi_sviews_decode_dev launch; (d) W3: the uniform hgi_decode_scaled_u8_dev batch call on the same planes.  Both sides on 128-byte rows.")
    say("# Conditions, stated before measuring: (c)'s bytes equal (a)'s, checked first; W1, W2: (c) < (a) and (c) < (b) at every shift (bytes predict")
    say("# (c) / (b) = 0.375x / 0.156x / 0.070x: recorded, not a condition); W3: (c) <= 1.15 x (d) at shifts 1 and 2.")
    w1, w2, w3 = shapes_of()
    missed = []
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        g = Grids(name, shapes)
        say("")
        say("%s: %d grids, %.3f Gpx; arena %.3f GB" % (name, g.n, g.px / 1e9, g.bytes / 1e9))
        for s in SHIFTS:
            g.check(s)
            d = g.at[s]
            info = d["plan"][0]
            say("  shift %d: %.4f Gpx out; (c)'s bytes equal (a)'s; hgi_sviews_plan on the host: %.0f us (%d entries, blob %d bytes, %d interior + %d ragged tiles)"
                % (s, d["spx"] / 1e9, d["plan"][2], g.n, info.plan_bytes, info.interior_tiles, info.edge_tiles))
            legs = [lambda: g.leg_a(s), g.leg_b, lambda: g.leg_c(s)] + ([lambda: g.leg_d(s)] if name == "W3" else [])
            # windows of 10 ms and more: the per-grid leg is thousands of launches a call, the one-launch legs get 20 calls
            t = timed(legs, [3 if g.n > 4096 else 5] + [20] * (len(legs) - 1))
            moved = g.px / (1 << s) + d["spx"]
            say("    (a) per grid %.1f us (min %.1f); (b) full decode %.1f us (min %.1f); (c) one launch %.1f us (min %.1f), %.2f Gpx/s out, %.2f GB/s at 1/2^s + 1/4^s B/px"
                % (t[0][0] * 1e3, t[0][1] * 1e3, t[1][0] * 1e3, t[1][1] * 1e3, t[2][0] * 1e3, t[2][1] * 1e3, d["spx"] / t[2][0] / 1e6, moved / t[2][0] / 1e6))
            say("    (a) / (c) = %.2fx; (b) / (c) = %.2fx; (c) / (b) = %.3fx (bytes predict %.3fx)" % (t[0][0] / t[2][0], t[1][0] / t[2][0], t[2][0] / t[1][0], BYTES[s]))
            if name == "W3":
                r = t[2][0] / t[3][0]
                if s <= 2:
                    say("    (d) batch call %.1f us (min %.1f); condition (c) <= 1.15x (d) -> %.3fx %s" % (t[3][0] * 1e3, t[3][1] * 1e3, r, "met" if r <= 1.15 else "MISSED"))
                    if r > 1.15:
                        missed.append("%s s%d (c) <= 1.15x (d): %.3fx" % (name, s, r))
                else:
                    say("    (d) batch call %.1f us (min %.1f); (c) / (d) = %.3fx (recorded: no condition at shift 3)" % (t[3][0] * 1e3, t[3][1] * 1e3, r))
            else:
                for leg, k in (("(a)", 0), ("(b)", 1)):
                    ok = t[2][0] < t[k][0]
                    say("    condition (c) < %s on %s at shift %d -> %s" % (leg, name, s, "met" if ok else "MISSED"))
                    if not ok:
                        missed.append("%s s%d (c) < %s" % (name, s, leg))
        del g
        torch.cuda.empty_cache()
    say("")
    say("conditions missed: %s" % ("; ".join(missed) if missed else "none"))
    say("FETCH_SIZE / WRITE_SIZE of W1 (b) and (c): not counted in this run (sviews_time.py --prof under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def prof():
    g = Grids("W1", shapes_of()[0])
    g.check(1)
    for fn in (g.leg_b, lambda: g.leg_c(1)):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1: %d grids, %d px, arena %d bytes" % (g.n, g.px, g.bytes))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--prof":
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_scaled_views.txt"))
