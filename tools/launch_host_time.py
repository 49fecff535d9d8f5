"""Host cost of the core library's tile launches, for two or more builds of libhgi_hip.so in ONE process on the same buffers:
what a change of the launchers' host code could move (the sibling of companion_host_time.py, with its counts of calls and rounds).  Usage:
    launch_host_time.py OUT.txt LABEL=DIR [LABEL=DIR ...]
DIR holds libhgi_hip.so.  Name a build twice to see the run's own spread: the passes of a row take turns round by round.
Rows: hgi_encode_u8_dev / hgi_decode_u8_dev on one 256 x 256 frame at levels 4 (the tile holds the pyramid) and 6 (the cone);
the region, scaled, pitched and list calls (four frames) at level 4; Crossed, a lossy table.  Per row: `calls` back-to-back
calls on torch's current stream, wall clock; `host` is the time until the last call returned, `done` until the stream drained,
per call, median (min .. max) of the rounds."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rustyhgi_amd import _ffi  # noqa: E402

W = H = 256
N = W * H
INTERP = 1
CALLS, ROUNDS = 2000, 15


def load(directory):
    L = ctypes.CDLL(os.path.join(directory, "libhgi_hip.so"))
    for sym, res, args in _ffi.SYMBOLS:
        fn = getattr(L, sym)
        fn.restype, fn.argtypes = res, args
    ctx = ctypes.c_void_p()
    assert L.hgi_ctx_create(0, ctypes.byref(ctx)) == _ffi.OK
    assert L.hgi_ctx_set_stream(ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or 0)) == _ffi.OK
    return L, ctx


def rows(L, ctx, buf, keep):
    """The calls on 256 x 256 frames: every side in a 1-MiB slice of `buf` of its own."""
    a, b = buf.data_ptr(), buf.data_ptr() + (1 << 20)
    lut = np.ascontiguousarray(np.arange(256) & 0xFC, dtype=np.uint8)
    lp, pitch = lut.ctypes.data, W + 64
    ins = (ctypes.c_void_p * 4)(*[a + i * N for i in range(4)])
    outs = (ctypes.c_void_p * 4)(*[b + i * N for i in range(4)])
    ws, hs = (ctypes.c_uint32 * 4)(*[W] * 4), (ctypes.c_uint32 * 4)(*[H] * 4)
    keep += [lut, ins, outs, ws, hs]
    return [
        ("encode L4", lambda: L.hgi_encode_u8_dev(ctx, a, W, H, 4, INTERP, lp, b, 1, N)),
        ("decode L4", lambda: L.hgi_decode_u8_dev(ctx, a, W, H, 4, INTERP, b, 1, N)),
        ("encode L6", lambda: L.hgi_encode_u8_dev(ctx, a, W, H, 6, INTERP, lp, b, 1, N)),
        ("decode L6", lambda: L.hgi_decode_u8_dev(ctx, a, W, H, 6, INTERP, b, 1, N)),
        ("region", lambda: L.hgi_decode_region_u8_dev(ctx, a, W, H, 4, INTERP, 37, 21, 200, 200, b, pitch, 1, N, 200 * pitch)),
        ("scaled s=1", lambda: L.hgi_decode_scaled_u8_dev(ctx, a, W, H, 5, INTERP, 1, b, pitch, 1, N, (H // 2) * pitch)),
        ("enc pitched", lambda: L.hgi_encode_u8_pitched_dev(ctx, a, pitch, W - 64, H, 4, INTERP, lp, b, pitch, 1, H * pitch, H * pitch)),
        ("dec pitched", lambda: L.hgi_decode_u8_pitched_dev(ctx, a, pitch, W - 64, H, 4, INTERP, b, pitch, 1, H * pitch, H * pitch)),
        ("enc list x4", lambda: L.hgi_encode_u8_list_dev(ctx, ins, ws, hs, 4, INTERP, lp, outs, 4)),
        ("dec list x4", lambda: L.hgi_decode_u8_list_dev(ctx, ins, ws, hs, 4, INTERP, outs, 4)),
    ]


def timed(fns):
    """companion_host_time.timed, with the spread of the rounds beside the median."""
    for fn in fns:
        for _ in range(200):
            assert fn() == _ffi.OK
    torch.cuda.synchronize()
    host, done = [[] for _ in fns], [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[i].append((t1 - t0) / CALLS * 1e6)
            done[i].append((t2 - t0) / CALLS * 1e6)
    return ["host %6.2f us (%6.2f .. %6.2f)   done %6.2f us (%6.2f .. %6.2f)" % (np.median(h), min(h), max(h), np.median(d), min(d), max(d))
            for h, d in zip(host, done)]


def main(out, passes):
    _ffi._share_torch_hip_runtime()
    buf = torch.randint(0, 256, (2 << 20,), dtype=torch.uint8, device="cuda")
    lines = ["# tools/launch_host_time.py: %d back-to-back calls per round, %d rounds per pass, the passes interleaved round by round;"
             % (CALLS, ROUNDS), "# one process, one buffer; torch %s, %s" % (torch.__version__, torch.cuda.get_device_name(0))]
    loaded, keep = [(label, load(directory)) for label, directory in passes], []
    for label, (L, _) in loaded:
        lines.append("# %s: %s" % (label, L.hgi_version().decode()))
    per_pass = [rows(L, ctx, buf, keep) for _, (L, ctx) in loaded]
    for r, (name, _) in enumerate(per_pass[0]):
        for (label, _), text in zip(loaded, timed([calls[r][1] for calls in per_pass])):
            lines.append("  %-12s %-9s %s" % (name, label, text))
            print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], [a.split("=", 1) for a in sys.argv[2:]])
