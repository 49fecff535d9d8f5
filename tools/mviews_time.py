"""Mapped view lists (libhgi_mviews.so: hgi_mviews_decode_dev) against the two routes a ragged batch of stored grids has without
them, device-resident, HIP events, one process, the legs of a comparison alternating within every round: writes
profiles/r22_mapped_views.txt (or the path in argv[1]).  All workloads at level 4, Crossed, grids coded with Medium; r07's
workloads with r07's seed (tools/framelist_time.py, tools/views_time.py), at E = 2 (float16) and E = 4 (float32), the table
affine_table(dtype):
  * W1 mixed: 1024 frames, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 frames, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard as 64 views.
The grids lie in aligned_arena(shapes, 128), the float frames in aligned_arena of their rows of w * E bytes: every row start of
both sides on a 128-byte line.  Legs:
  (a) one hgi_map_decode_dev call per frame;
  (b) hgi_views_decode_dev into a uint8 arena and one torch conversion of that arena per list (uint8 * scale -> dtype, one pass);
  (c) the one hgi_mviews_decode_dev launch;
  (d) W3 only: the single hgi_map_decode_dev batch call on the same planes.
Every (c) result is checked against (a)'s bytes, arena against arena, before anything is timed.  The host time of
hgi_mviews_plan is the best of five calls.  Nothing here gates a test.
`--prof E`: the workload of the counter passes instead -- W1 (b) and (c) at that E, five launches each after the check, nothing
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
from rustyhgi_amd import _ffi, _ffi_map as FM, _ffi_mviews as FMV, _ffi_views as FV  # noqa: E402

L, LM, LMV, LV = _ffi.lib(), FM.lib(), FMV.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED = 4, 1, 0x48474937
LUT = np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(2, LUT.ctypes.data, None))
DTYPE = {2: torch.float16, 4: torch.float32}
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


class Grids:
    """The stored grids of a workload in aligned_arena(shapes, 128): synthetic frames (r07's) coded with the core list call."""

    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.px = sum(w * h for w, h in shapes)
        offs, at = [], 0
        for w, h in shapes:
            offs.append(at)
            at += (w * h + 255) // 256 * 256
        img = torch.empty(at, dtype=torch.uint8, device="cuda")
        for i, ((w, h), o) in enumerate(zip(shapes, offs)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_RAMP if i % 2 else _ffi.SYNTH_NOISE, SEED, i, w, h, img.data_ptr() + o, 1, w * h))
        packed = torch.empty_like(img)
        P, U = ctypes.c_void_p * self.n, ctypes.c_uint32 * self.n
        _ffi.check(L.hgi_encode_u8_list_dev(ctx.handle, P(*[img.data_ptr() + o for o in offs]), U(*[w for w, h in shapes]), U(*[h for w, h in shapes]),
                                            LEVELS, INTERP, LUT.ctypes.data, P(*[packed.data_ptr() + o for o in offs]), self.n))
        self.bytes, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        self.grid = torch.zeros(self.bytes, dtype=torch.uint8, device="cuda")
        assert self.grid.data_ptr() % 4096 == 0, "the page rule of the layout assumes a page-aligned arena"
        for (w, h), o, (ao, ap) in zip(shapes, offs, self.places):
            self.grid[ao:ao + h * ap].view(h, ap)[:, :w].copy_(packed[o:o + w * h].view(h, w))
        self.u8 = torch.empty_like(self.grid)      # (b): the decoded bytes, the grids' layout
        n = self.n
        arr = (FV.ViewPair * n)(*[FV.ViewPair(self.grid.data_ptr() + ao, self.u8.data_ptr() + ao, w, h, ap, ap) for (w, h), (ao, ap) in zip(shapes, self.places)])
        size = LV.hgi_views_plan_bytes(n)
        host = np.zeros(size, np.uint8)
        self.vinfo = FV.ViewsInfo()
        FV.check(LV.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(self.vinfo)))
        self.vblob = torch.from_numpy(host[:int(self.vinfo.plan_bytes)].copy()).cuda()
        torch.cuda.synchronize()


class Floats:
    """The float side of a workload at one element size: the arena of (c), the arena of (a), the arena of (b), the plan."""

    def __init__(self, g, E):
        self.g, self.E, self.dtype = g, E, DTYPE[E]
        self.bytes, self.places = H.aligned_arena([(h, w * E) for w, h in g.shapes], 128)
        self.out_c = torch.full((self.bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_a = torch.full((self.bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_b = torch.empty((g.bytes,), dtype=self.dtype, device="cuda")      # the uint8 arena's layout, in elements
        self.table = H.affine_table(self.dtype, device="cuda")
        self.scale = torch.tensor(1.0 / 255.0, dtype=self.dtype, device="cuda")
        n = g.n
        arr = (FMV.MViewPair * n)(*[FMV.MViewPair(g.grid.data_ptr() + ao, self.out_c.data_ptr() + fo, w, h, ap, fp)
                                    for (w, h), (ao, ap), (fo, fp) in zip(g.shapes, g.places, self.places)])
        size = LMV.hgi_mviews_plan_bytes(n)
        host = np.zeros(size, np.uint8)
        self.info = FMV.MViewsInfo()
        self.host_us = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            st = LMV.hgi_mviews_plan(ctypes.addressof(arr), n, E, host.ctypes.data, size, ctypes.addressof(self.info))
            self.host_us = min(self.host_us, (time.perf_counter() - t0) * 1e6)
            FMV.check(st)
        self.blob = torch.from_numpy(host[:int(self.info.plan_bytes)].copy()).cuda()
        self.calls = [(g.grid.data_ptr() + ao, ap, w, h, self.out_a.data_ptr() + fo, fp) for (w, h), (ao, ap), (fo, fp) in zip(g.shapes, g.places, self.places)]

    def leg_a(self):
        s, t, E, f = stream(), self.table.data_ptr(), self.E, LM.hgi_map_decode_dev
        for src, sp, w, h, dst, dp in self.calls:
            st = f(s, src, sp, w, h, LEVELS, INTERP, t, E, dst, dp, 1, 0, 0)
            if st:
                FM.check(st)

    def leg_b(self):
        g = self.g
        FV.check(LV.hgi_views_decode_dev(stream(), g.vblob.data_ptr(), ctypes.addressof(g.vinfo), LEVELS, INTERP))
        torch.mul(g.u8, self.scale, out=self.out_b)

    def leg_c(self):
        FMV.check(LMV.hgi_mviews_decode_dev(stream(), self.blob.data_ptr(), ctypes.addressof(self.info), LEVELS, INTERP, self.table.data_ptr()))

    def leg_d(self):      # W3: one batch call on the same planes, into (a)'s arena
        g, E, n = self.g, self.E, 4096 * 4096
        FM.check(LM.hgi_map_decode_dev(stream(), g.grid.data_ptr(), 4096, 4096, 4096, LEVELS, INTERP, self.table.data_ptr(), E, self.out_a.data_ptr(), 4096 * E,
                                       g.n, n, n * E))

    def check(self):
        """(c) against (a), arena against arena (both filled with one sentinel first); (b)'s values against (c)'s on a sample."""
        self.leg_a()
        self.leg_c()
        self.leg_b()
        torch.cuda.synchronize()
        assert torch.equal(self.out_c, self.out_a), "%s E%d: the fused launch differs from one mapped decode per frame" % (self.g.name, self.E)
        assert int((self.out_c != 0xA5).sum()) >= self.g.px * self.E // 2, "nothing was written"
        for i in sorted(set(list(range(0, self.g.n, 97)) + [self.g.n - 1])):
            (w, h), (ao, ap), (fo, fp) = self.g.shapes[i], self.g.places[i], self.places[i]
            c = self.out_c[fo:fo + h * fp].view(h, fp).view(self.dtype)[:, :w]
            b = self.out_b[ao:ao + h * ap].view(h, ap)[:, :w]
            assert torch.allclose(b.float(), c.float(), rtol=2e-3, atol=1e-6), "%s E%d frame %d: the conversion route differs" % (self.g.name, self.E, i)
        if self.g.name == "W3":
            self.out_a.fill_(0xA5)
            self.leg_d()
            torch.cuda.synchronize()
            assert torch.equal(self.out_c, self.out_a), "W3 E%d: the fused launch differs from the batch call" % self.E


def shapes_of():
    rng = np.random.default_rng(SEED)
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    return w1, w2, [(4096, 4096)] * 64


def main(path):
    say("# tools/mviews_time.py: mapped view lists against one mapped decode per frame and against view-list decode + conversion;")
    say("# L%d Crossed, table affine_table(dtype), device-resident, HIP events, median (min) of 5 rounds, the legs alternating inside" % LEVELS)
    say("# every round; seed 0x%x; %s; %s; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LMV.hgi_mviews_version().decode(), LM.hgi_map_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) one hgi_map_decode_dev per frame; (b) hgi_views_decode_dev to a uint8 arena + one torch conversion per list; (c) the one")
    say("# hgi_mviews_decode_dev launch; (d) W3: the single hgi_map_decode_dev batch call on the same planes.  Both sides on 128-byte rows.")
    w1, w2, w3 = shapes_of()
    missed = []
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        g = Grids(name, shapes)
        for E in (2, 4):
            f = Floats(g, E)
            f.check()
            say("")
            say("%s E = %d: %d frames, %.3f Gpx; grid arena %.3f GB, float arena %.3f GB; hgi_mviews_plan on the host: %.0f us (%d entries, blob %d bytes)"
                % (name, E, g.n, g.px / 1e9, g.bytes / 1e9, f.bytes / 1e9, f.host_us, g.n, f.info.plan_bytes))
            legs = [f.leg_a, f.leg_b, f.leg_c] + ([f.leg_d] if name == "W3" else [])
            # windows of 10 ms and more: the per-frame leg is thousands of launches a call, the one-launch legs get 20 calls
            t = timed(legs, [3 if g.n > 4096 else 5] + [20] * (len(legs) - 1))
            say("  (a) per frame %.1f us (min %.1f); (b) views + conversion %.1f us (min %.1f); (c) one launch %.1f us (min %.1f), %.2f Gpx/s, %.2f GB/s at %d B/px"
                % (t[0][0] * 1e3, t[0][1] * 1e3, t[1][0] * 1e3, t[1][1] * 1e3, t[2][0] * 1e3, t[2][1] * 1e3, g.px / t[2][0] / 1e6, g.px * (1 + E) / t[2][0] / 1e6, 1 + E))
            say("    (a) / (c) = %.2fx; (b) / (c) = %.2fx" % (t[0][0] / t[2][0], t[1][0] / t[2][0]))
            if name == "W3":
                r = t[2][0] / t[3][0]
                say("    (d) batch call %.1f us (min %.1f); condition (c) <= 1.15x (d) -> %.3fx %s" % (t[3][0] * 1e3, t[3][1] * 1e3, r, "met" if r <= 1.15 else "MISSED"))
                if r > 1.15:
                    missed.append("%s E%d (c) <= 1.15x (d): %.3fx" % (name, E, r))
            else:
                for leg, k in (("(a)", 0), ("(b)", 1)):
                    ok = t[2][0] < t[k][0]
                    say("    condition (c) < %s on %s E = %d -> %s" % (leg, name, E, "met" if ok else "MISSED"))
                    if not ok:
                        missed.append("%s E%d (c) < %s" % (name, E, leg))
            del f
            torch.cuda.empty_cache()
        del g
        torch.cuda.empty_cache()
    say("")
    say("conditions missed: %s" % ("; ".join(missed) if missed else "none"))
    say("FETCH_SIZE / WRITE_SIZE of W1 (b) and (c): not counted in this run (mviews_time.py --prof E under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def prof(E):
    g = Grids("W1", shapes_of()[0])
    f = Floats(g, E)
    f.check()
    for fn in (f.leg_b, f.leg_c):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1 E = %d: %d frames, %d px, grid arena %d bytes, float arena %d bytes" % (E, g.n, g.px, g.bytes, f.bytes))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--prof":
        prof(int(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_mapped_views.txt"))
