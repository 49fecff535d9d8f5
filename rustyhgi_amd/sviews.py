"""Scaled view lists (libhgi_sviews.so, include/hgi_sviews.h): stored grids of different shapes, each with a row pitch of its own,
decoded at 1 / 2**shift resolution into images that each have a pitch of their own -- every grid of a ragged store as a preview,
thumbnails side by side on one canvas -- in ONE launch, at the bytes of the stride-2**shift lattice.

    sizes = [scaled_shape(h, w, shift) for h, w in shapes]          # (sh, sw) = (ceil(h / 2**shift), ceil(w / 2**shift))
    plan = ScaledViewPlan(zip(grid_views, preview_views), shift)    # judged and planned on the host, uploaded once
    Decoder(...).decode_scaled_views(plan, levels)                  # any number of launches, each capturable into a graph
"""
import ctypes

import numpy as np

from . import _ffi
from .views import _layout


def scaled_shape(height, width, shift):
    """(sh, sw) = (ceil(height / 2**shift), ceil(width / 2**shift)): the image a grid of (height, width) decodes to at that shift."""
    return -(-int(height) >> int(shift)), -(-int(width) >> int(shift))


class ScaledViewPlan:
    """The plan of a scaled view list: `pairs` is a list of (src, dst) 2-D uint8 CUDA tensor views on one device -- `src` a stored
    grid of shape (h, w), `dst` the image of shape scaled_shape(h, w, shift) -- last stride 1, the pitch taken from stride(0);
    `shift` is an int from 0 to 31, one for the list.  Layouts are validated here (ValueError); the rules of the list -- aliasing
    on rectangles of bytes, the tile count -- by hgi_sviews_plan on the host (HgiError, the text names the pair).  The blob is
    uploaded once and the tensors are kept alive with it.  A list the one launch does not serve (HGI_EUNSUPPORTED: shift 0, or
    an entry beyond the 32-bit buffer path) still makes a plan: `fused` is False, `reason` says why, and decode_scaled_views
    composes one scaled decode per view."""

    def __init__(self, pairs, shift):
        from . import _ffi_sviews as F
        if isinstance(shift, (bool, np.bool_)) or not isinstance(shift, (int, np.integer)) or not 0 <= int(shift) <= 31:
            raise ValueError("ScaledViewPlan: shift must be an int from 0 to 31, not %r" % (shift,))
        self.shift = shift = int(shift)
        pairs = list(pairs)
        self.srcs, self.dsts = [p[0] for p in pairs], [p[1] for p in pairs]
        n = len(pairs)
        self.layouts = []
        arr = (F.SViewPair * max(n, 1))()
        device = None
        for i, (s, d) in enumerate(pairs):
            try:
                sp_, h, w, sp = _layout(s, "source", i)
                dp_, dh, dw, dp = _layout(d, "destination", i)
            except ValueError as err:
                raise ValueError(str(err).replace("ViewPlan:", "ScaledViewPlan:", 1)) from None
            want = scaled_shape(h, w, shift)
            if (dh, dw) != want:
                raise ValueError("ScaledViewPlan: pair %d: the destination has shape %s, the source %s at shift %d gives %s" % (i, (dh, dw), (h, w), shift, want))
            if s.device != d.device or (device is not None and s.device != device):
                raise ValueError("ScaledViewPlan: pair %d lives on %s / %s: one device per list" % (i, s.device, d.device))
            device = s.device
            arr[i] = F.SViewPair(sp_, dp_, w, h, sp, dp)
            self.layouts.append((sp_, dp_, w, h, sp, dp))
        self.device = device
        if device is not None and device.type != "cuda":      # (layouts are judged first: their faults are the caller's to see on any machine)
            raise ValueError("ScaledViewPlan: torch tensors must live on the GPU")
        self.info = F.SViewsInfo()
        L = F.lib()
        size = int(L.hgi_sviews_plan_bytes(n))
        host = np.zeros(max(size, 16), np.uint8)
        st = L.hgi_sviews_plan(ctypes.addressof(arr), n, shift, host.ctypes.data, size, ctypes.addressof(self.info))
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
