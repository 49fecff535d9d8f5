"""Typed view lists (libhgi_tviews.so, include/hgi_tviews.h): float16 / bfloat16 / float32 frames of different shapes, each with
a row pitch of its own -- the frames of a padded float tensor, an arena of float frames, float crops of one canvas -- converted
(v = clamp(rint(x * scale + bias), 0, 255), include/hgi_typed.h) and encoded straight into grids that each have a pitch of their
own, in ONE launch.

    batch, frames = padded_batch([(h, w), ...], torch.float16)      # [N, Hmax, Wp] and its (h, w) views
    total, places = aligned_arena([(h, w), ...])                    # where the grids go, rows on 128-byte lines
    grids = arena_views(torch.empty(total, dtype=torch.uint8, device="cuda"), shapes, places)
    plan = TypedViewPlan(zip(frames, grids), torch.float16)         # judged and planned on the host, uploaded once
    Encoder(...).encode_typed_views(plan)                           # any number of launches, each capturable into a graph

`scale` and `bias` are as for Encoder.encode_typed (rustyhgi_amd.affine_inverse).
"""
import ctypes

import numpy as np

from . import _ffi
from .mviews import _elem_size
from .views import _layout as _u8_layout


def _float_layout(t, dtype, e, i):
    """(ptr, height, width, pitch in BYTES) of the source of pair i: a 2-D CUDA tensor of `dtype` whose last dimension has
    stride 1 element."""
    what = "source"
    if not type(t).__module__.startswith("torch"):
        raise ValueError("TypedViewPlan: pair %d: the %s must be a torch CUDA tensor" % (i, what))
    if t.dtype != dtype or t.dim() != 2:
        raise ValueError("TypedViewPlan: pair %d: the %s must be a 2-D (height, width) %s tensor" % (i, what, dtype))
    h, w = (int(v) for v in t.shape)
    if max(h, w) >= 2 ** 32:
        raise ValueError("TypedViewPlan: pair %d: the %s is too large" % (i, what))
    if h * w == 0:
        return 0, h, w, w * e
    sr, sc = (int(v) for v in t.stride())
    if w > 1 and sc != 1:
        raise ValueError("TypedViewPlan: pair %d: the last dimension of the %s must have stride 1, not %d" % (i, what, sc))
    if h > 1 and sr < w:
        raise ValueError("TypedViewPlan: pair %d: the row stride %d of the %s is smaller than the width %d" % (i, sr, what, w))
    return t.data_ptr(), h, w, (sr if h > 1 else w) * e


class TypedViewPlan:
    """The plan of a typed view list: `pairs` is a list of (src, dst) pairs on one device -- `src` a 2-D view of `dtype`
    (torch.float16 / bfloat16 / float32), `dst` a 2-D uint8 CUDA view (where the grid goes) of equal shape -- last stride 1, the
    pitch taken from stride(0).  Layouts are validated here (ValueError); the rules of the list -- aliasing on rectangles of
    bytes, the tile count -- by hgi_tviews_plan on the host (HgiError, the text names the pair).  The blob is uploaded once and
    the tensors are kept alive with it.  A list the one launch does not serve (HGI_EUNSUPPORTED: an entry beyond the 32-bit
    buffer path, or of 2-byte elements and an odd width whose last frame byte ends a 4-KiB page) still makes a plan: `fused` is
    False, `reason` says why, and encode_typed_views composes one encode_typed call per view."""

    def __init__(self, pairs, dtype):
        from . import _ffi_tviews as F
        self.dtype, self.elem_size = dtype, _elem_size(dtype, "TypedViewPlan")
        pairs = list(pairs)
        self.srcs, self.dsts = [p[0] for p in pairs], [p[1] for p in pairs]
        n = len(pairs)
        self.layouts = []
        arr = (F.TViewPair * max(n, 1))()
        device = None
        for i, (s, d) in enumerate(pairs):
            sp_, h, w, sp = _float_layout(s, dtype, self.elem_size, i)
            try:
                dp_, dh, dw, dp = _u8_layout(d, "destination", i)
            except ValueError as err:
                raise ValueError(str(err).replace("ViewPlan:", "TypedViewPlan:", 1)) from None
            if (h, w) != (dh, dw):
                raise ValueError("TypedViewPlan: pair %d: the destination has shape %s, the source %s" % (i, (dh, dw), (h, w)))
            if s.device != d.device or (device is not None and s.device != device):
                raise ValueError("TypedViewPlan: pair %d lives on %s / %s: one device per list" % (i, s.device, d.device))
            device = s.device
            arr[i] = F.TViewPair(sp_, dp_, w, h, sp, dp)
            self.layouts.append((sp_, dp_, w, h, sp, dp))
        self.device = device
        if device is not None and device.type != "cuda":      # (layouts are judged first: their faults are the caller's to see on any machine)
            raise ValueError("TypedViewPlan: torch tensors must live on the GPU")
        self.info = F.TViewsInfo()
        L = F.lib()
        size = int(L.hgi_tviews_plan_bytes(n))
        host = np.zeros(max(size, 16), np.uint8)
        st = L.hgi_tviews_plan(ctypes.addressof(arr), n, self.elem_size, host.ctypes.data, size, ctypes.addressof(self.info))
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
