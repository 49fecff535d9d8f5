"""Recon view lists (libhgi_rviews.so, include/hgi_rviews.h): frames of different shapes, each with a row pitch of its own on the
image that is read, on the grid that is written and on the reconstruction that is written -- the sprites of an atlas, the tiles
of a mosaic, a ragged thumbnail store inside a rate/quality search -- encoded in ONE launch, which also writes the image the
decoder will make of every grid.

    arena_bytes, places = aligned_arena([(h, w), ...])                  # a layout with every row start on a 128-byte line
    plan = ReconViewPlan(zip(image_views, grid_views, recon_views))     # judged and planned on the host, uploaded once
    grids, recons = Encoder(...).encode_views_with_reconstruction(plan) # any number of launches, each capturable into a graph
"""
import ctypes

import numpy as np

from . import _ffi
from .views import _layout


class ReconViewPlan:
    """The plan of a recon view list: `triples` is a list of (src, grid, recon) 2-D uint8 CUDA tensor views of equal shape on one
    device, last stride 1, the pitch of each taken from stride(0).  Layouts are validated here (ValueError); the rules of the
    list -- aliasing on rectangles of bytes over all three sides, the tile count -- by hgi_rviews_plan on the host (HgiError, the
    text names the triple and the side).  The blob is uploaded once and the tensors are kept alive with it.  A list the one
    launch does not serve (HGI_EUNSUPPORTED: an entry beyond the 32-bit buffer path, or of a width that is no multiple of 4
    with its last source bytes at the end of a 4-KiB page) still makes a plan: `fused` is False, `reason` says why, and
    encode_views_with_reconstruction composes one encode with reconstruction per view."""

    def __init__(self, triples):
        from . import _ffi_rviews as F
        triples = list(triples)
        self.srcs, self.grids, self.recons = [t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples]
        n = len(triples)
        self.layouts = []
        arr = (F.RViewTriple * max(n, 1))()
        device = None
        for i, (s, g, r) in enumerate(triples):
            try:
                sp_, h, w, sp = _layout(s, "source", i)
                gp_, gh, gw, gp = _layout(g, "grid", i)
                rp_, rh, rw, rp = _layout(r, "reconstruction", i)
            except ValueError as err:
                raise ValueError(str(err).replace("ViewPlan: pair", "ReconViewPlan: triple", 1)) from None
            for what, shape in (("grid", (gh, gw)), ("reconstruction", (rh, rw))):
                if shape != (h, w):
                    raise ValueError("ReconViewPlan: triple %d: the %s has shape %s, the source %s" % (i, what, shape, (h, w)))
            if s.device != g.device or s.device != r.device or (device is not None and s.device != device):
                raise ValueError("ReconViewPlan: triple %d lives on %s / %s / %s: one device per list" % (i, s.device, g.device, r.device))
            device = s.device
            arr[i] = F.RViewTriple(sp_, gp_, rp_, w, h, sp, gp, rp)
            self.layouts.append((sp_, gp_, rp_, w, h, sp, gp, rp))
        self.device = device
        if device is not None and device.type != "cuda":      # (layouts are judged first: their faults are the caller's to see on any machine)
            raise ValueError("ReconViewPlan: torch tensors must live on the GPU")
        self.info = F.RViewsInfo()
        L = F.lib()
        size = int(L.hgi_rviews_plan_bytes(n))
        host = np.zeros(max(size, 16), np.uint8)
        st = L.hgi_rviews_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(self.info))
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
