"""Typed view lists (libhgi_tviews.so: hgi_tviews_encode_dev) against the two routes a ragged batch of float frames has without
them, device-resident, HIP events, one process, the legs of a comparison alternating within every round: writes
profiles/r23_typed_views.txt (or the path in argv[1]).  All workloads at level 4, Crossed, Medium; r07's workloads with r07's
seed (tools/framelist_time.py, tools/views_time.py, tools/mviews_time.py), at E = 2 (float16) and E = 4 (float32), the frames
x = affine_table(dtype)[noise image], scale 255, bias 0:
  * W1 mixed: 1024 frames, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 frames, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard as 64 views.
The float frames lie in aligned_arena of their rows of w * E bytes, the grids in aligned_arena(shapes, 128): every row start of
both sides on a 128-byte line.  Legs:
  (a) one hgi_typed_encode_dev call per frame;
  (b) one torch conversion of a float arena into a uint8 arena per list plus hgi_views_encode_dev.  The conversion is elementwise
      over the whole arena, so leg (b) reads a float arena of its own in the uint8 arena's layout (rows pitch * E bytes: on
      128-byte lines too).  It is the cheapest torch composition that gives the library's bytes on these frames: t = 0.5 + 255 * x
      in one pass (torch.add with alpha), the truncating cast to uint8 in a second -- the frames are table entries, so t is
      never a tie and never out of range; the general conversion (NaN, clamp, ties to even) takes more passes;
  (c) the one hgi_tviews_encode_dev launch;
  (d) W3 only: the single hgi_typed_encode_dev batch call on the same planes.
Every (c) result is checked against (a)'s bytes, arena against arena, before anything is timed, and (b)'s grids against (c)'s.
The host time of hgi_tviews_plan is the best of five calls.  Nothing here gates a test.
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
from rustyhgi_amd import _ffi, _ffi_tviews as FTV, _ffi_typed as FT, _ffi_views as FV  # noqa: E402

L, LT, LTV, LV = _ffi.lib(), FT.lib(), FTV.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED = 4, 1, 0x48474937
SCALE, BIAS = 255.0, 0.0
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


class Images:
    """The uint8 noise images of a workload, packed, and the layout of the grids: aligned_arena(shapes, 128)."""

    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.px = sum(w * h for w, h in shapes)
        self.offs, at = [], 0
        for w, h in shapes:
            self.offs.append(at)
            at += (w * h + 255) // 256 * 256
        self.img = torch.empty(at, dtype=torch.uint8, device="cuda")
        for i, ((w, h), o) in enumerate(zip(shapes, self.offs)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, SEED, i, w, h, self.img.data_ptr() + o, 1, w * h))
        self.bytes, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        torch.cuda.synchronize()


class Floats:
    """One element size of a workload: the float arena of (a), (c) and (d), the float and uint8 arenas of (b), the grid arenas,
    the two plans."""

    def __init__(self, g, E):
        self.g, self.E, self.dtype = g, E, DTYPE[E]
        self.bytes, self.places = H.aligned_arena([(h, w * E) for w, h in g.shapes], 128)
        table = H.affine_table(self.dtype, device="cuda")
        self.src = torch.zeros((self.bytes // E,), dtype=self.dtype, device="cuda")
        self.src_b = torch.zeros((g.bytes,), dtype=self.dtype, device="cuda")      # the uint8 arena's layout, in elements
        assert self.src.data_ptr() % 128 == 0 and self.src_b.data_ptr() % 128 == 0
        raw = self.src.view(torch.uint8)
        for (w, h), o, (ao, ap), (fo, fp) in zip(g.shapes, g.offs, g.places, self.places):
            x = table[g.img[o:o + w * h].view(h, w).long()]
            raw[fo:fo + h * fp].view(h, fp).view(self.dtype)[:, :w].copy_(x)
            self.src_b[ao:ao + h * ap].view(h, ap)[:, :w].copy_(x)
        self.tmp_b = torch.empty_like(self.src_b)
        self.u8_b = torch.zeros((g.bytes,), dtype=torch.uint8, device="cuda")
        self.half = torch.tensor(0.5, dtype=self.dtype, device="cuda")
        self.out_a = torch.full((g.bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_b = torch.full((g.bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_c = torch.full((g.bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        n = g.n
        arr = (FTV.TViewPair * n)(*[FTV.TViewPair(self.src.data_ptr() + fo, self.out_c.data_ptr() + ao, w, h, fp, ap)
                                    for (w, h), (ao, ap), (fo, fp) in zip(g.shapes, g.places, self.places)])
        size = LTV.hgi_tviews_plan_bytes(n)
        host = np.zeros(size, np.uint8)
        self.info = FTV.TViewsInfo()
        self.host_us = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            st = LTV.hgi_tviews_plan(ctypes.addressof(arr), n, E, host.ctypes.data, size, ctypes.addressof(self.info))
            self.host_us = min(self.host_us, (time.perf_counter() - t0) * 1e6)
            FTV.check(st)
        self.blob = torch.from_numpy(host[:int(self.info.plan_bytes)].copy()).cuda()
        varr = (FV.ViewPair * n)(*[FV.ViewPair(self.u8_b.data_ptr() + ao, self.out_b.data_ptr() + ao, w, h, ap, ap) for (w, h), (ao, ap) in zip(g.shapes, g.places)])
        size = LV.hgi_views_plan_bytes(n)
        host = np.zeros(size, np.uint8)
        self.vinfo = FV.ViewsInfo()
        FV.check(LV.hgi_views_plan(ctypes.addressof(varr), n, host.ctypes.data, size, ctypes.addressof(self.vinfo)))
        self.vblob = torch.from_numpy(host[:int(self.vinfo.plan_bytes)].copy()).cuda()
        self.calls = [(self.src.data_ptr() + fo, fp, w, h, self.out_a.data_ptr() + ao, ap) for (w, h), (ao, ap), (fo, fp) in zip(g.shapes, g.places, self.places)]
        torch.cuda.synchronize()

    def leg_a(self):
        s, E, f, lut = stream(), self.E, LT.hgi_typed_encode_dev, LUT.ctypes.data
        for src, sp, w, h, dst, dp in self.calls:
            st = f(s, src, sp, E, 0, SCALE, BIAS, w, h, LEVELS, INTERP, lut, dst, dp, 1, 0, 0)
            if st:
                FT.check(st)

    def leg_b(self):
        torch.add(self.half, self.src_b, alpha=SCALE, out=self.tmp_b)
        self.u8_b.copy_(self.tmp_b)
        FV.check(LV.hgi_views_encode_dev(stream(), self.vblob.data_ptr(), ctypes.addressof(self.vinfo), LEVELS, INTERP, LUT.ctypes.data))

    def leg_c(self):
        FTV.check(LTV.hgi_tviews_encode_dev(stream(), self.blob.data_ptr(), ctypes.addressof(self.info), 0, SCALE, BIAS, LEVELS, INTERP, LUT.ctypes.data))

    def leg_d(self):      # W3: one batch call on the same planes, into (a)'s arena
        g, E, n = self.g, self.E, 4096 * 4096
        FT.check(LT.hgi_typed_encode_dev(stream(), self.src.data_ptr(), 4096 * E, E, 0, SCALE, BIAS, 4096, 4096, LEVELS, INTERP, LUT.ctypes.data,
                                         self.out_a.data_ptr(), 4096, g.n, n * E, n))

    def check(self):
        """(c) against (a), arena against arena (both filled with one sentinel first); then (b)'s arena against (c)'s."""
        self.leg_a()
        self.leg_c()
        self.leg_b()
        torch.cuda.synchronize()
        assert torch.equal(self.out_c, self.out_a), "%s E%d: the fused launch differs from one typed encode per frame" % (self.g.name, self.E)
        assert int((self.out_c != 0xA5).sum()) >= self.g.px // 2, "nothing was written"
        assert torch.equal(self.out_b, self.out_c), "%s E%d: the conversion route differs" % (self.g.name, self.E)
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
    say("# tools/tviews_time.py: typed view lists against one typed encode per frame and against conversion + view-list encode;")
    say("# L%d Crossed Medium, frames affine_table(dtype)[noise], scale 255, bias 0, device-resident, HIP events, median (min) of 5 rounds," % LEVELS)
    say("# the legs alternating inside every round; seed 0x%x; %s; %s; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LTV.hgi_tviews_version().decode(), LT.hgi_typed_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) one hgi_typed_encode_dev per frame; (b) a torch conversion of the float arena to a uint8 arena (two passes: 0.5 + 255 x, the cast)")
    say("# + hgi_views_encode_dev; (c) the one hgi_tviews_encode_dev launch; (d) W3: the single hgi_typed_encode_dev batch call on the same")
    say("# planes.  Both sides on 128-byte rows.  Conditions, stated before measuring: W1, W2: (c) < (a) and (c) < (b); W3: (c) <= 1.15 x (d).")
    w1, w2, w3 = shapes_of()
    missed = []
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        g = Images(name, shapes)
        for E in (2, 4):
            f = Floats(g, E)
            f.check()
            say("")
            say("%s E = %d: %d frames, %.3f Gpx; float arena %.3f GB, grid arena %.3f GB; hgi_tviews_plan on the host: %.0f us (%d entries, blob %d bytes)"
                % (name, E, g.n, g.px / 1e9, f.bytes / 1e9, g.bytes / 1e9, f.host_us, g.n, f.info.plan_bytes))
            legs = [f.leg_a, f.leg_b, f.leg_c] + ([f.leg_d] if name == "W3" else [])
            # windows of 10 ms and more: the per-frame leg is thousands of launches a call, the one-launch legs get 20 calls
            t = timed(legs, [3 if g.n > 4096 else 5] + [20] * (len(legs) - 1))
            say("  (a) per frame %.1f us (min %.1f); (b) conversion + views %.1f us (min %.1f); (c) one launch %.1f us (min %.1f), %.2f Gpx/s, %.2f GB/s at %d B/px"
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
    say("FETCH_SIZE / WRITE_SIZE of W1 (b) and (c): not counted in this run (tviews_time.py --prof E under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def prof(E):
    g = Images("W1", shapes_of()[0])
    f = Floats(g, E)
    f.check()
    for fn in (f.leg_b, f.leg_c):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1 E = %d: %d frames, %d px, float arena %d bytes, grid arena %d bytes" % (E, g.n, g.px, f.bytes, g.bytes))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--prof":
        prof(int(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_typed_views.txt"))
