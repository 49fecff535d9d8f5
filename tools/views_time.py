"""View lists (libhgi_views.so: hgi_views_encode_dev / hgi_views_decode_dev) against the core frame lists and the pitched call,
device-resident, HIP events, one process, the legs of a comparison alternating within every round: writes
profiles/r21_views.txt (or the path in argv[1]).  All workloads at level 4, Medium, Crossed; r07's workloads with r07's seed
(tools/framelist_time.py):
  * W1 mixed: 1024 frames, widths and heights drawn independently and uniformly from [64, 2048], ~1.1 Gpx;
  * W2 thumbnails: 8192 frames, sides from [96, 320];
  * W3 equal: the 64 x 4096^2 shard.
Legs:
  (a) the core list calls on the frames packed back to back at 256-B offsets -- the yardstick;
  (b) the view calls on the same packed frames (pitch == width): what the new kernels cost on the lists' own layout;
  (c) the view calls on aligned_arena(shapes, 128): every row start on a 128-byte line;
  (d) W3 as 64 views against hgi_*_u8_pitched_dev on the same planes.
Every view result is checked against the core list's bytes before it is timed.  The host time of hgi_views_plan is the best of
five calls.  Nothing here gates a test.
`--prof`: the workload of the counter passes instead -- W1 (a) and (c), five launches each after the check, nothing timed
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
from rustyhgi_amd import _ffi, _ffi_views as FV  # noqa: E402

L, LV = _ffi.lib(), FV.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
LEVELS, INTERP, SEED = 4, 1, 0x48474937
LUT = np.zeros(256, np.uint8)
_ffi.check(L.hgi_linear_lut(2, LUT.ctypes.data, None))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps, rounds=5):
    """Median and minimum ms per call of each leg; the legs take turns inside every round."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / reps)
    return [(float(np.median(m)), float(min(m))) for m in ms]


class Plan:
    """hgi_views_plan of (src, dst, w, h, src pitch, dst pitch) entries, uploaded; the host time of the plan call."""

    def __init__(self, entries):
        n = len(entries)
        arr = (FV.ViewPair * n)(*[FV.ViewPair(*e) for e in entries])
        size = LV.hgi_views_plan_bytes(n)
        host = np.zeros(size, np.uint8)
        self.info = FV.ViewsInfo()
        self.host_us = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            st = LV.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(self.info))
            self.host_us = min(self.host_us, (time.perf_counter() - t0) * 1e6)
            FV.check(st)
        self.blob = torch.from_numpy(host[:int(self.info.plan_bytes)].copy()).cuda()
        self.stream = _ffi._vp(torch.cuda.current_stream().cuda_stream or 0)

    def encode(self):
        FV.check(LV.hgi_views_encode_dev(self.stream, self.blob.data_ptr(), ctypes.addressof(self.info), LEVELS, INTERP, LUT.ctypes.data))

    def decode(self):
        FV.check(LV.hgi_views_decode_dev(self.stream, self.blob.data_ptr(), ctypes.addressof(self.info), LEVELS, INTERP))


class Workload:
    def __init__(self, name, shapes):
        self.name, self.shapes, self.n = name, shapes, len(shapes)
        self.offs, at = [], 0
        for w, h in shapes:      # r07's layout; a frame that would break the views' page rule (page-aligned base) moves on by 256 B
            while w % 4 and (at + w * h - 1) % 4096 > 4092:
                at += 256
            self.offs.append(at)
            at += (w * h + 255) // 256 * 256
        self.px = sum(w * h for w, h in shapes)
        self.img = torch.empty(at, dtype=torch.uint8, device="cuda")
        for i, ((w, h), o) in enumerate(zip(shapes, self.offs)):
            _ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_RAMP if i % 2 else _ffi.SYNTH_NOISE, SEED, i, w, h,
                                          self.img.data_ptr() + o, 1, w * h))
        self.grid, self.out = torch.empty_like(self.img), torch.empty_like(self.img)      # (a)
        assert all(t.data_ptr() % 4096 == 0 for t in (self.img, self.grid)), "the layouts assume page-aligned buffers"
        self.vgrid, self.vout = torch.empty_like(self.img), torch.empty_like(self.img)    # (b)
        P, U = ctypes.c_void_p * self.n, ctypes.c_uint32 * self.n
        self.p_img = P(*[self.img.data_ptr() + o for o in self.offs])
        self.p_grid = P(*[self.grid.data_ptr() + o for o in self.offs])
        self.p_out = P(*[self.out.data_ptr() + o for o in self.offs])
        self.ws, self.hs = U(*[w for w, h in shapes]), U(*[h for w, h in shapes])
        # (b): the packed layout through the view calls
        self.b_enc = Plan([(self.img.data_ptr() + o, self.vgrid.data_ptr() + o, w, h, w, w) for (w, h), o in zip(shapes, self.offs)])
        self.b_dec = Plan([(self.vgrid.data_ptr() + o, self.vout.data_ptr() + o, w, h, w, w) for (w, h), o in zip(shapes, self.offs)])
        # (c): every row start on a 128-byte line
        total, self.places = H.aligned_arena([(h, w) for w, h in shapes], 128)
        self.aimg = torch.empty(total, dtype=torch.uint8, device="cuda")
        self.agrid, self.aout = torch.empty_like(self.aimg), torch.empty_like(self.aimg)
        assert all(t.data_ptr() % 4096 == 0 for t in (self.vgrid, self.aimg, self.agrid))
        for (w, h), o, (ao, ap) in zip(shapes, self.offs, self.places):
            self.aimg[ao:ao + h * ap].view(h, ap)[:, :w].copy_(self.img[o:o + w * h].view(h, w))
        self.arena_bytes = total
        self.c_enc = Plan([(self.aimg.data_ptr() + ao, self.agrid.data_ptr() + ao, w, h, ap, ap) for (w, h), (ao, ap) in zip(shapes, self.places)])
        self.c_dec = Plan([(self.agrid.data_ptr() + ao, self.aout.data_ptr() + ao, w, h, ap, ap) for (w, h), (ao, ap) in zip(shapes, self.places)])

    def enc_list(self):
        _ffi.check(L.hgi_encode_u8_list_dev(ctx.handle, self.p_img, self.ws, self.hs, LEVELS, INTERP, LUT.ctypes.data, self.p_grid, self.n))

    def dec_list(self):
        _ffi.check(L.hgi_decode_u8_list_dev(ctx.handle, self.p_grid, self.ws, self.hs, LEVELS, INTERP, self.p_out, self.n))

    def check(self):
        """The view calls' bytes against the core list's, (b) and (c), on every 23rd frame and the last."""
        self.enc_list()
        self.dec_list()
        for p in (self.b_enc, self.c_enc):
            p.encode()
        for p in (self.b_dec, self.c_dec):
            p.decode()
        torch.cuda.synchronize()
        sample = sorted(set(list(range(0, self.n, 23)) + [self.n - 1]))
        for i in sample:
            (w, h), o, (ao, ap) = self.shapes[i], self.offs[i], self.places[i]
            for packed, view, arena in ((self.grid, self.vgrid, self.agrid), (self.out, self.vout, self.aout)):
                want = packed[o:o + w * h].view(h, w)
                assert torch.equal(view[o:o + w * h].view(h, w), want), "%s frame %d: packed views differ from the list" % (self.name, i)
                assert torch.equal(arena[ao:ao + h * ap].view(h, ap)[:, :w], want), "%s frame %d: arena views differ from the list" % (self.name, i)

    def free(self):
        for k in ("img", "grid", "out", "vgrid", "vout", "aimg", "agrid", "aout", "b_enc", "b_dec", "c_enc", "c_dec"):
            delattr(self, k)
        torch.cuda.empty_cache()


def shapes_of():
    rng = np.random.default_rng(SEED)
    w1 = [(int(rng.integers(64, 2049)), int(rng.integers(64, 2049))) for _ in range(1024)]
    w2 = [(int(rng.integers(96, 321)), int(rng.integers(96, 321))) for _ in range(8192)]
    return w1, w2, [(4096, 4096)] * 64


def main(path):
    say("# tools/views_time.py: view lists against the core frame lists and the pitched call; L%d Medium Crossed, device-resident," % LEVELS)
    say("# HIP events, median (min) of 5 rounds, the legs alternating inside every round; seed 0x%x; %s; %s; torch %s"
        % (SEED, L.hgi_version().decode(), LV.hgi_views_version().decode(), torch.__version__))
    say("# (a) core list calls, frames packed at 256-B offsets; (b) view calls, same layout (pitch == width); (c) view calls on")
    say("# aligned_arena(shapes, 128); (d) W3 as 64 views against hgi_*_u8_pitched_dev on the same planes")
    w1, w2, w3 = shapes_of()
    n = 4096 * 4096
    rate_uni, c_rate = {}, {}
    for name, shapes in (("W3", w3), ("W1", w1), ("W2", w2)):
        wl = Workload(name, shapes)
        wl.check()
        say("")
        say("%s: %d frames, %.3f Gpx; packed %.3f GB, arena %.3f GB; hgi_views_plan on the host: %.0f us (%d entries, blob %d bytes)"
            % (name, wl.n, wl.px / 1e9, wl.img.numel() / 1e9, wl.arena_bytes / 1e9, wl.c_enc.host_us, wl.n, wl.c_enc.info.plan_bytes))
        for d in ("encode", "decode"):
            enc = d == "encode"
            legs = [wl.enc_list if enc else wl.dec_list, (wl.b_enc.encode if enc else wl.b_dec.decode), (wl.c_enc.encode if enc else wl.c_dec.decode)]
            if name == "W3":      # the uniform call (the pixel-rate yardstick) and the pitched call on the same planes
                if enc:
                    legs.append(lambda: _ffi.check(L.hgi_encode_u8_dev(ctx.handle, wl.img.data_ptr(), 4096, 4096, LEVELS, INTERP, LUT.ctypes.data,
                                                                       wl.grid.data_ptr(), 64, n)))
                    legs.append(lambda: _ffi.check(L.hgi_encode_u8_pitched_dev(ctx.handle, wl.img.data_ptr(), 4096, 4096, 4096, LEVELS, INTERP,
                                                                               LUT.ctypes.data, wl.grid.data_ptr(), 4096, 64, n, n)))
                else:
                    legs.append(lambda: _ffi.check(L.hgi_decode_u8_dev(ctx.handle, wl.grid.data_ptr(), 4096, 4096, LEVELS, INTERP, wl.out.data_ptr(), 64, n)))
                    legs.append(lambda: _ffi.check(L.hgi_decode_u8_pitched_dev(ctx.handle, wl.grid.data_ptr(), 4096, 4096, 4096, LEVELS, INTERP,
                                                                               wl.out.data_ptr(), 4096, 64, n, n)))
            t = timed(legs, 20 if wl.px > 3e8 else 50)
            say("  %s (a) list %.1f us (min %.1f), %.2f Gpx/s; (b) views packed %.1f us (min %.1f), %.3fx (a); (c) views arena %.1f us (min %.1f), %.3fx (a), %.2f Gpx/s"
                % (d, t[0][0] * 1e3, t[0][1] * 1e3, wl.px / t[0][0] / 1e6, t[1][0] * 1e3, t[1][1] * 1e3, t[1][0] / t[0][0], t[2][0] * 1e3, t[2][1] * 1e3,
                   t[2][0] / t[0][0], wl.px / t[2][0] / 1e6))
            if name == "W3":
                rate_uni[d] = wl.px / t[3][0] / 1e6
                r = t[1][0] / t[4][0]
                say("    uniform call %.1f us, %.2f Gpx/s; pitched call %.1f us" % (t[3][0] * 1e3, rate_uni[d], t[4][0] * 1e3))
                say("    condition (d): 64 views <= 1.15x the pitched call on the same planes -> %.3fx %s (the lists measured 1.01x / 1.14x of the uniform call)"
                    % (r, "met" if r <= 1.15 else "MISSED"))
            else:
                ok = t[2][0] <= t[0][0]
                say("    condition (c) <= (a) on %s %s -> %.3fx %s" % (name, d, t[2][0] / t[0][0], "met" if ok else "MISSED"))
                c_rate[(name, d)] = (wl.px / t[2][0] / 1e6) / rate_uni[d], (wl.px / t[0][0] / 1e6) / rate_uni[d]
        wl.free()
    say("")
    for d, r07 in (("encode", 0.38), ("decode", 0.43)):
        say("W1 %s pixel rate against the uniform 64 x 4096^2 call of this run: (c) %.2fx, (a) %.2fx (r07 measured %.2fx for the lists)"
            % (d, c_rate[("W1", d)][0], c_rate[("W1", d)][1], r07))
    say("FETCH_SIZE / WRITE_SIZE of W1 (a) and (c): not counted in this run (views_time.py --prof under rocprofv3 --pmc is the workload for it)")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prof():
    wl = Workload("W1", shapes_of()[0])
    wl.check()
    for fn in (wl.enc_list, wl.dec_list, wl.c_enc.encode, wl.c_dec.decode):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print("W1: %d frames, %d px, packed %d bytes, arena %d bytes" % (wl.n, wl.px, wl.img.numel(), wl.arena_bytes))


if __name__ == "__main__":
    if sys.argv[1:] == ["--prof"]:
        prof()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_views.txt"))
