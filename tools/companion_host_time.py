"""Host cost of the smallest launches of the four companion libraries, for two or more builds of them in ONE process on the
same buffers: what a change of the entry points' host layer could move.  Usage:
    companion_host_time.py OUT.txt LABEL=DIR [LABEL=DIR ...]
DIR holds libhgi_recon.so, libhgi_map.so, libhgi_typed.so and libhgi_requant.so.  Name a build twice to see the run's own
spread: the passes of a row take turns round by round.  One 128 x 64 frame (one tile) and one 201 x 100 frame (ragged tiles,
the tail bytes), level 2, Crossed.  Per row: `calls` back-to-back calls on torch's current stream, wall clock; `host` is the
time until the last call returned, `done` until the stream drained, per call, median (min) of 15 rounds."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rustyhgi_amd import _ffi, _ffi_map, _ffi_recon, _ffi_requant, _ffi_typed  # noqa: E402

TABLES = {"recon": _ffi_recon.SYMBOLS, "map": _ffi_map.SYMBOLS, "typed": _ffi_typed.SYMBOLS, "requant": _ffi_requant.SYMBOLS}
CALLS, ROUNDS, LEVELS, INTERP = 2000, 15, 2, 1


def load(directory):
    libs = {}
    for name, table in TABLES.items():
        L = ctypes.CDLL(os.path.join(directory, "libhgi_%s.so" % name))
        for sym, res, args in table:
            fn = getattr(L, sym)
            fn.restype, fn.argtypes = res, args
        libs[name] = L
    return libs


def rows(libs, buf, w, h):
    """The four calls on one frame of w x h: every side in a 1-MiB slice of `buf` of its own, rows 4 * (w + 8) bytes apart."""
    a, b, c, t = (buf.data_ptr() + (i << 20) for i in range(4))
    pitch = 4 * (w + 8)
    lut = np.ascontiguousarray(255 - np.arange(256), dtype=np.uint8)      # not the identity: requantize refuses that one
    stream, lp = torch.cuda.current_stream().cuda_stream or None, lut.ctypes.data
    return lut, [
        ("recon", lambda: libs["recon"].hgi_recon_encode_u8_dev(stream, a, pitch, w, h, LEVELS, INTERP, lp, b, pitch, c, pitch, 1, 0, 0, 0)),
        ("map fp16", lambda: libs["map"].hgi_map_decode_dev(stream, a, pitch, w, h, LEVELS, INTERP, t, 2, b, pitch, 1, 0, 0)),
        ("typed fp32", lambda: libs["typed"].hgi_typed_encode_dev(stream, a, pitch, 4, 0, 255.0, 0.0, w, h, LEVELS, INTERP, lp, b, pitch, 1, 0, 0)),
        ("requant", lambda: libs["requant"].hgi_requant_dev(stream, a, pitch, w, h, LEVELS, INTERP, lp, b, pitch, 1, 0, 0)),
    ]


def timed(fns):
    """One row: the same call of every pass, the passes taking turns round by round, so that a drift of the host's clocks
    during the row falls on all of them alike.  Returns one text per pass."""
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
    return ["host %6.2f us (min %6.2f)   done %6.2f us (min %6.2f)" % (np.median(h), min(h), np.median(d), min(d)) for h, d in zip(host, done)]


def main(out, passes):
    _ffi._share_torch_hip_runtime()
    buf = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
    lines = ["# tools/companion_host_time.py: %d back-to-back calls per round, %d rounds per pass, the passes interleaved round by round;"
             % (CALLS, ROUNDS), "# one process, one buffer; torch %s, %s" % (torch.__version__, torch.cuda.get_device_name(0))]
    loaded = [(label, load(directory)) for label, directory in passes]
    for label, libs in loaded:
        lines.append("# %s: %s" % (label, "; ".join(getattr(libs[n], "hgi_%s_version" % n)().decode() for n in TABLES)))
    for w, h in ((128, 64), (201, 100)):
        per_pass = [rows(libs, buf, w, h) for _, libs in loaded]      # [(lut kept alive, [(name, call)])]
        for r, (name, _) in enumerate(per_pass[0][1]):
            texts = timed([calls[r][1] for _, calls in per_pass])
            for (label, _), text in zip(loaded, texts):
                lines.append("  %3d x %-3d  %-10s %-9s %s" % (w, h, name, label, text))
                print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], [a.split("=", 1) for a in sys.argv[2:]])
