"""View lists (libhgi_views.so, include/hgi_views.h): frames that each bring a shape and a row pitch of their own on the side that
is read and on the side that is written -- sprites in an atlas, mosaic tiles decoded into their places on one canvas, crops of
different sizes out of one device image, mixed-size planes with padded rows -- coded in ONE launch.

    arena_bytes, places = aligned_arena([(h, w), ...])         # a layout with every row start on a 128-byte line
    plan = ViewPlan([(src_view, dst_view), ...])               # judged and planned on the host, uploaded once
    Encoder(...).encode_views(plan)                            # any number of launches, each capturable into a graph
    Decoder(...).decode_views(plan, levels)

A plan depends on neither direction nor depth: the first view of a pair is always the one that is READ.
"""
import ctypes

import numpy as np

from . import _ffi


def aligned_arena(shapes, align=128):
    """A layout for frames of the given (height, width) shapes in one byte arena with EVERY ROW START on an `align`-byte
    boundary: `(total_bytes, [(offset, pitch), ...])`, frame i at `offset` with its rows `pitch` bytes apart -- pitch the
    width rounded up to `align`, offsets in list order.  Rows that start on a line are what the tile kernels read and write
    at their best rate.  The arena itself must start on an `align`-byte boundary (torch allocations do).
    A zero-size frame takes no room.  In an arena that starts on a 4-KiB page boundary no frame breaks the page rule of
    include/hgi_views.h: a frame whose width is no multiple of 4 and whose last byte would fall on the last three bytes of a
    page is moved on by `align` bytes."""
    align = int(align)
    if align < 1 or align & (align - 1):
        raise ValueError("aligned_arena: align must be a power of two, not %r" % (align,))
    places, total = [], 0
    for s in shapes:
        h, w = (int(v) for v in s)
        if h < 0 or w < 0:
            raise ValueError("aligned_arena: shape %r has a negative side" % (tuple(s),))
        pitch = -(-w // align) * align
        while h and w % 4 and (total + (h - 1) * pitch + w - 1) % 4096 > 4092:
            total += align
        places.append((total, pitch))
        total += h * pitch if h and w else 0
    return total, places


def arena_views(arena, shapes, places):
    """The (height, width) views of a 1-D uint8 tensor `arena` at the `places` aligned_arena returned."""
    return [arena[o:o + h * p].view(h, p)[:, :w] if h and w else arena.new_empty((h, w)) for (h, w), (o, p) in zip(shapes, places)]


def _layout(t, what, i):
    """(ptr, height, width, pitch) of one side of pair i: a 2-D uint8 CUDA tensor whose last dimension has stride 1."""
    if not type(t).__module__.startswith("torch"):
        raise ValueError("ViewPlan: pair %d: the %s must be a torch CUDA tensor" % (i, what))
    import torch
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError("ViewPlan: pair %d: the %s must be a 2-D (height, width) uint8 tensor" % (i, what))
    h, w = (int(v) for v in t.shape)
    if max(h, w) >= 2 ** 32:
        raise ValueError("ViewPlan: pair %d: the %s is too large" % (i, what))
    if h * w == 0:
        return 0, h, w, w
    sr, sc = (int(v) for v in t.stride())
    if w > 1 and sc != 1:
        raise ValueError("ViewPlan: pair %d: the last dimension of the %s must have stride 1, not %d" % (i, what, sc))
    if h > 1 and sr < w:
        raise ValueError("ViewPlan: pair %d: the row stride %d of the %s is smaller than the width %d" % (i, sr, what, w))
    return t.data_ptr(), h, w, (sr if h > 1 else w)


class ViewPlan:
    """The plan of a view list: `pairs` is a list of (src, dst) 2-D uint8 CUDA tensor views of equal shape on one device,
    last stride 1, the pitch taken from stride(0).  Layouts are validated here (ValueError); the rules of the list --
    aliasing on rectangles of bytes, the tile count -- by hgi_views_plan on the host (HgiError, the text names the pair).
    The blob is uploaded once and the tensors are kept alive with it.  A list the one launch does not serve
    (HGI_EUNSUPPORTED: an entry beyond the 32-bit buffer path, or of a width that is no multiple of 4 with its last source
    bytes at the end of a 4-KiB page) still makes a plan: `fused` is False, `reason` says why, and encode_views /
    decode_views compose one pitched call per view."""

    def __init__(self, pairs):
        from . import _ffi_views as F
        pairs = list(pairs)
        self.srcs, self.dsts = [p[0] for p in pairs], [p[1] for p in pairs]
        n = len(pairs)
        self.layouts = []
        arr = (F.ViewPair * max(n, 1))()
        device = None
        for i, (s, d) in enumerate(pairs):
            sp_, h, w, sp = _layout(s, "source", i)
            dp_, dh, dw, dp = _layout(d, "destination", i)
            if (h, w) != (dh, dw):
                raise ValueError("ViewPlan: pair %d: the destination has shape %s, the source %s" % (i, (dh, dw), (h, w)))
            if s.device != d.device or (device is not None and s.device != device):
                raise ValueError("ViewPlan: pair %d lives on %s / %s: one device per list" % (i, s.device, d.device))
            device = s.device
            arr[i] = F.ViewPair(sp_, dp_, w, h, sp, dp)
            self.layouts.append((sp_, dp_, w, h, sp, dp))
        self.device = device
        if device is not None and device.type != "cuda":      # (layouts are judged first: their faults are the caller's to see on any machine)
            raise ValueError("ViewPlan: torch tensors must live on the GPU")
        self.info = F.ViewsInfo()
        L = F.lib()
        size = int(L.hgi_views_plan_bytes(n))
        host = np.zeros(max(size, 16), np.uint8)
        st = L.hgi_views_plan(ctypes.addressof(arr), n, host.ctypes.data, size, ctypes.addressof(self.info))
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
