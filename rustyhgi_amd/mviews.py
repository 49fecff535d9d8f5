"""Mapped view lists (libhgi_mviews.so, include/hgi_mviews.h): stored grids of different shapes, each with a row pitch of its
own, decoded straight into float16 / bfloat16 / float32 frames that each have a pitch of their own -- a ragged batch into a padded
float tensor, or into an aligned arena of float frames -- through a 256-entry table, in ONE launch.

    batch, views = padded_batch([(h, w), ...], torch.float16)       # [N, Hmax, Wp] and its (h, w) views, rows on 128-byte lines
    plan = MappedViewPlan(zip(grid_views, views), torch.float16)    # judged and planned on the host, uploaded once
    Decoder(...).decode_mapped_views(plan, levels, table)           # any number of launches, each capturable into a graph

`table` is as for Decoder.decode_mapped (rustyhgi_amd.affine_table).
"""
import ctypes

import numpy as np

from . import _ffi
from .views import _layout as _u8_layout


def _elem_size(dtype, what):
    if not type(dtype).__module__.startswith("torch"):
        raise ValueError("%s: dtype must be torch.float16, torch.bfloat16 or torch.float32, not %r" % (what, dtype))
    import torch
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError("%s: dtype must be torch.float16, torch.bfloat16 or torch.float32, not %s" % (what, dtype))
    return 2 if dtype != torch.float32 else 4


def padded_batch(shapes, dtype, align=128, device="cuda", fill=None):
    """The data-loader case in one call: for frames of the given (height, width) shapes, a tensor `[N, Hmax, Wp]` of `dtype`
    (torch.float16 / bfloat16 / float32) on `device` whose rows are `Wp` elements, Wmax rounded up so that `Wp * E` is a
    multiple of `align` bytes -- every row of every frame starts on an `align`-byte boundary, which is what the tile kernels
    write at their best rate -- and the list of its views `batch[i, :h, :w]`, the destinations of a MappedViewPlan.  `fill`:
    the value of the padding (None leaves the tensor uninitialised; a launch writes the views only).  Returns (batch, views)."""
    what = "padded_batch"
    e = _elem_size(dtype, what)
    align = int(align)
    if align < e or align & (align - 1):
        raise ValueError("%s: align must be a power of two of at least one element (%d bytes), not %r" % (what, e, align))
    shapes = [tuple(int(v) for v in s) for s in shapes]
    for s in shapes:
        if len(s) != 2 or min(s) < 0:
            raise ValueError("%s: shape %r is not a (height, width) of non-negative sides" % (what, s))
    hmax = max([h for h, w in shapes if h and w], default=0)
    wmax = max([w for h, w in shapes if h and w], default=0)
    wp = -(-wmax * e // align) * align // e
    import torch
    batch = torch.empty((len(shapes), hmax, wp), dtype=dtype, device=device) if fill is None else \
        torch.full((len(shapes), hmax, wp), fill, dtype=dtype, device=device)
    return batch, [batch[i, :h, :w] if h and w else batch.new_empty((h, w)) for i, (h, w) in enumerate(shapes)]


def _typed_layout(t, dtype, e, i):
    """(ptr, height, width, pitch in BYTES) of the destination of pair i: a 2-D CUDA tensor of `dtype` whose last dimension has
    stride 1 element."""
    what = "destination"
    if not type(t).__module__.startswith("torch"):
        raise ValueError("MappedViewPlan: pair %d: the %s must be a torch CUDA tensor" % (i, what))
    if t.dtype != dtype or t.dim() != 2:
        raise ValueError("MappedViewPlan: pair %d: the %s must be a 2-D (height, width) %s tensor" % (i, what, dtype))
    h, w = (int(v) for v in t.shape)
    if max(h, w) >= 2 ** 32:
        raise ValueError("MappedViewPlan: pair %d: the %s is too large" % (i, what))
    if h * w == 0:
        return 0, h, w, w * e
    sr, sc = (int(v) for v in t.stride())
    if w > 1 and sc != 1:
        raise ValueError("MappedViewPlan: pair %d: the last dimension of the %s must have stride 1, not %d" % (i, what, sc))
    if h > 1 and sr < w:
        raise ValueError("MappedViewPlan: pair %d: the row stride %d of the %s is smaller than the width %d" % (i, sr, what, w))
    return t.data_ptr(), h, w, (sr if h > 1 else w) * e


class MappedViewPlan:
    """The plan of a mapped view list: `pairs` is a list of (src, dst) pairs on one device -- `src` a 2-D uint8 CUDA view (a
    stored grid), `dst` a 2-D view of `dtype` (torch.float16 / bfloat16 / float32) of equal shape -- last stride 1, the pitch
    taken from stride(0).  Layouts are validated here (ValueError); the rules of the list -- aliasing on rectangles of bytes,
    the tile count -- by hgi_mviews_plan on the host (HgiError, the text names the pair).  The blob is uploaded once and the
    tensors are kept alive with it.  A list the one launch does not serve (HGI_EUNSUPPORTED: an entry beyond the 32-bit buffer
    path, or of a width that is no multiple of 4 with its last grid bytes at the end of a 4-KiB page) still makes a plan:
    `fused` is False, `reason` says why, and decode_mapped_views composes one decode_mapped call per view."""

    def __init__(self, pairs, dtype):
        from . import _ffi_mviews as F
        self.dtype, self.elem_size = dtype, _elem_size(dtype, "MappedViewPlan")
        pairs = list(pairs)
        self.srcs, self.dsts = [p[0] for p in pairs], [p[1] for p in pairs]
        n = len(pairs)
        self.layouts = []
        arr = (F.MViewPair * max(n, 1))()
        device = None
        for i, (s, d) in enumerate(pairs):
            try:
                sp_, h, w, sp = _u8_layout(s, "source", i)
            except ValueError as err:
                raise ValueError(str(err).replace("ViewPlan:", "MappedViewPlan:", 1)) from None
            dp_, dh, dw, dp = _typed_layout(d, dtype, self.elem_size, i)
            if (h, w) != (dh, dw):
                raise ValueError("MappedViewPlan: pair %d: the destination has shape %s, the source %s" % (i, (dh, dw), (h, w)))
            if s.device != d.device or (device is not None and s.device != device):
                raise ValueError("MappedViewPlan: pair %d lives on %s / %s: one device per list" % (i, s.device, d.device))
            device = s.device
            arr[i] = F.MViewPair(sp_, dp_, w, h, sp, dp)
            self.layouts.append((sp_, dp_, w, h, sp, dp))
        self.device = device
        if device is not None and device.type != "cuda":      # (layouts are judged first: their faults are the caller's to see on any machine)
            raise ValueError("MappedViewPlan: torch tensors must live on the GPU")
        self.info = F.MViewsInfo()
        L = F.lib()
        size = int(L.hgi_mviews_plan_bytes(n))
        host = np.zeros(max(size, 16), np.uint8)
        st = L.hgi_mviews_plan(ctypes.addressof(arr), n, self.elem_size, host.ctypes.data, size, ctypes.addressof(self.info))
        self.fused, self.reason, self.blob = True, "", None
        if st == _ffi.EUNSUPPORTED:
            self.fused, self.reason = False, F.last_error()
        else:
            F.check(st)
            if self.info.count:
                import torch
                self.blob = torch.from_numpy(host[:int(self.info.plan_bytes)].copy()).to(device)

    def __len__(self):
        return len(self.srcs)
