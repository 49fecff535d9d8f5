"""Mirror of `hgi::{Encoder, Decoder}` (reference src/encoder.rs, src/decoder.rs) over the C ABI.

numpy arrays take the host-pointer entry points (hgi_encode_u8 / hgi_decode_u8); torch CUDA
tensors take the device-pointer, asynchronous, batched entry points on torch's current stream.
Every path ends in the HIP kernels; there is no host implementation.
"""
import ctypes

import numpy as np

from . import _ffi
from .grid import Grid
from .interpolator import Interpolator
from .quantizator import Quantizator


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _interp_id(interpolator):
    kid = getattr(interpolator, "kernel_id", None)
    if kid is None:
        raise _ffi.HgiError(_ffi.EUNSUPPORTED,
                            "interpolator %r has no device predictor" % type(interpolator).__name__)
    return int(kid)


def _torch_ctx(t, ctx=None):
    """The context serving tensor `t`, bound to torch's current stream on t's device so that the
    launches are ordered with the torch ops around them."""
    import torch
    if not t.is_cuda:
        raise ValueError("torch tensors must live on the GPU (use numpy for host buffers)")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError("expected a contiguous uint8 tensor")
    return _bind_ctx(t, ctx)


def _bind_ctx(t, ctx=None):
    """The context of CUDA tensor `t`'s device, bound to torch's current stream there."""
    import torch
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    if ctx is None:
        ctx = _ffi.default_context(dev)
    elif ctx.device != dev:
        raise ValueError("tensor lives on cuda:%d but the context was created for cuda:%d" % (dev, ctx.device))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return ctx


def _check_out(out, like, what):
    """A caller-supplied output buffer goes to the C ABI as a raw pointer: it must be exactly what the call will write --
    uint8, C-contiguous, the input's shape, on the input's device -- and must not share memory with the input."""
    if _is_torch(like):
        import torch
        if not _is_torch(out) or out.dtype != torch.uint8 or not out.is_contiguous() or out.shape != like.shape \
                or out.device != like.device:
            raise ValueError("%s: `out` must be a contiguous uint8 tensor of shape %s on %s" % (what, tuple(like.shape), like.device))
        a0, b0, n = like.data_ptr(), out.data_ptr(), like.numel()
    else:
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] \
                or not out.flags["WRITEABLE"] or out.shape != like.shape:
            raise ValueError("%s: `out` must be a writable C-contiguous uint8 array of shape %s" % (what, like.shape))
        a0, b0, n = like.ctypes.data, out.ctypes.data, like.size
    if a0 < b0 + n and b0 < a0 + n:
        raise ValueError("%s: `out` overlaps the input" % what)
    return out


def _check_rect(rect, width, height, what):
    """(x0, y0, w, h) of a window that lies inside the (width, height) frame -- checked in Python integers, before any
    device call (the C ABI takes 32-bit coordinates: x0 = 2**32 - 1 must not wrap into the frame)."""
    try:
        x0, y0, w, h = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError("%s: the region is (x0, y0, width, height)" % what)
    if min(x0, y0, w, h) < 0:
        raise ValueError("%s: region %r has a negative coordinate or size" % (what, (x0, y0, w, h)))
    if x0 + w > width or y0 + h > height:
        raise ValueError("%s: region %r does not lie inside the %dx%d frame" % (what, (x0, y0, w, h), width, height))
    return x0, y0, w, h


def _check_region_out(out, like, shape, what):
    """`out=` of a region call: a C-contiguous uint8 buffer of the window stack's shape beside `like` (the grids), not
    overlapping them."""
    if _is_torch(like):
        import torch
        if not _is_torch(out) or out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != shape \
                or out.device != like.device:
            raise ValueError("%s: `out` must be a contiguous uint8 tensor of shape %s on %s" % (what, shape, like.device))
        a0, na, b0, nb = like.data_ptr(), like.numel(), out.data_ptr(), out.numel()
    else:
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] \
                or not out.flags["WRITEABLE"] or out.shape != shape:
            raise ValueError("%s: `out` must be a writable C-contiguous uint8 array of shape %s" % (what, shape))
        a0, na, b0, nb = like.ctypes.data, like.size, out.ctypes.data, out.size
    if a0 < b0 + nb and b0 < a0 + na:
        raise ValueError("%s: `out` overlaps the input" % what)
    return out


def _check_shift(shift, what):
    """The scale step: an int from 0 to 31 (bool, float and str are refused, before any device call)."""
    if isinstance(shift, (bool, np.bool_)) or not isinstance(shift, (int, np.integer)) or not 0 <= int(shift) <= 31:
        raise ValueError("%s: shift must be an int from 0 to 31, not %r" % (what, shift))
    return int(shift)


def scaled_size(width, height, shift):
    """(sw, sh) = (ceil(width / 2**shift), ceil(height / 2**shift)): the frame of a scaled decode."""
    return -(-int(width) >> int(shift)), -(-int(height) >> int(shift))


def _spans_meet(spans):
    """spans: (lo, hi, is_output) byte ranges.  True when two outputs meet or an output meets an input (inputs may overlap each
    other) -- include/hgi.h's rule for frame lists, by one sorted sweep."""
    hi_any = hi_out = 0
    for lo, hi, is_out in sorted(s for s in spans if s[1] > s[0]):
        if lo < hi_out or (is_out and lo < hi_any):
            return True
        hi_any = max(hi_any, hi)
        if is_out:
            hi_out = max(hi_out, hi)
    return False


def _check_list(frames, out, what):
    """A frame list -- 2-D uint8 arrays, all torch CUDA tensors on one device (contiguous) or all numpy arrays -- and its `out=`
    list: the same shapes, uint8, C-contiguous, beside the inputs, no output meeting another output or any input.  Everything is
    decided here, before any device call.  Returns (frames, is_torch)."""
    if not isinstance(frames, (list, tuple)):
        raise ValueError("%s: expected a list of (height, width) frames" % what)
    frames = list(frames)
    torch_in = [_is_torch(f) for f in frames]
    if any(torch_in) and not all(torch_in):
        raise ValueError("%s: the list mixes torch tensors and other arrays" % what)
    use_torch = bool(frames) and all(torch_in)
    if use_torch:
        import torch
        dev = frames[0].device
        for i, f in enumerate(frames):
            if f.dtype != torch.uint8 or f.dim() != 2 or not f.is_contiguous():
                raise ValueError("%s: frame %d must be a contiguous (height, width) uint8 tensor" % (what, i))
            if f.device != dev:
                raise ValueError("%s: frame %d lives on %s, frame 0 on %s: one device per list" % (what, i, f.device, dev))
            if max(f.shape) >= 2 ** 32:
                raise ValueError("%s: frame %d is too large" % (what, i))
        spans = [(f.data_ptr(), f.data_ptr() + f.numel(), False) for f in frames]
    else:
        for i, f in enumerate(frames):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 2:
                raise ValueError("%s: frame %d must be a (height, width) uint8 array" % (what, i))
        frames = [np.ascontiguousarray(f) for f in frames]
        spans = [(f.ctypes.data, f.ctypes.data + f.size, False) for f in frames]
    if use_torch and frames[0].device.type != "cuda":
        on_host = "torch tensors must live on the GPU (use numpy for host buffers)"
    else:
        on_host = None
    if out is None:
        if on_host:
            raise ValueError(on_host)
        return frames, use_torch
    if not isinstance(out, (list, tuple)) or len(out) != len(frames):
        raise ValueError("%s: `out` must be a list of %d frames" % (what, len(frames)))
    for i, (f, o) in enumerate(zip(frames, out)):
        if use_torch:
            import torch
            ok = _is_torch(o) and o.dtype == torch.uint8 and o.is_contiguous() and o.shape == f.shape and o.device == f.device
            lo = o.data_ptr() if ok else 0
        else:
            ok = isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.flags["C_CONTIGUOUS"] and o.flags["WRITEABLE"] \
                and o.shape == f.shape
            lo = o.ctypes.data if ok else 0
        if not ok:
            raise ValueError("%s: `out` frame %d must be a C-contiguous uint8 buffer of shape %s beside the input"
                             % (what, i, tuple(f.shape)))
        spans.append((lo, lo + int(np.prod(f.shape)), True))
    if _spans_meet(spans):
        raise ValueError("%s: `out` frames overlap each other or the input" % what)
    if on_host:
        raise ValueError(on_host)
    return frames, use_torch


def _list_out(frames):
    """Outputs of a torch frame list: (h, w) views into ONE allocation, each frame at a 256-B offset."""
    import torch
    offs, total = [], 0
    for f in frames:
        offs.append(total)
        total += (f.numel() + 255) // 256 * 256
    buf = torch.empty((total,), dtype=torch.uint8, device=frames[0].device)
    return [buf[o:o + f.numel()].view(f.shape) for o, f in zip(offs, frames)]


def _list_arrays(frames, outs):
    """The C ABI's host arrays of a list call: input pointers, widths, heights, output pointers."""
    n = len(frames)
    ptrs = ctypes.c_void_p * n
    u32s = ctypes.c_uint32 * n
    return (ptrs(*[f.data_ptr() for f in frames]), u32s(*[int(f.shape[1]) for f in frames]),
            u32s(*[int(f.shape[0]) for f in frames]), ptrs(*[o.data_ptr() for o in outs]))


def _view_layout(x, what):
    """The layout of a pitched view: a 2-D (height, width) or 3-D (batch, height, width) uint8 torch tensor or numpy array whose
    last dimension has stride 1, whose rows lie >= width bytes apart and whose frames lie uniformly >= one frame's span apart --
    any slice t[f0:f1, y0:y1, x0:x1] of a contiguous buffer.  Returns (ptr, batch, height, width, pitch, frame_stride, span) in
    bytes, span = (height - 1) * pitch + width.  Everything else -- other strides (steps, negative steps, expanded dimensions),
    dtypes, ranks -- raises ValueError; nothing here touches a device."""
    if _is_torch(x):
        import torch
        if x.dtype != torch.uint8:
            raise ValueError("%s: expected a uint8 tensor, not %s" % (what, x.dtype))
        shape, strides = tuple(int(v) for v in x.shape), tuple(int(v) for v in x.stride())
    elif isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise ValueError("%s: expected a uint8 array, not %s" % (what, x.dtype))
        shape, strides = tuple(int(v) for v in x.shape), tuple(int(v) for v in x.strides)
    else:
        raise ValueError("%s: expected a uint8 torch CUDA tensor or numpy array" % what)
    if len(shape) not in (2, 3):
        raise ValueError("%s: expected a (height, width) or (batch, height, width) view, not %d dimensions" % (what, len(shape)))
    if len(shape) == 2:
        shape, strides = (1,) + shape, (0,) + strides
    (b, h, w), (sf, sr, sc) = shape, strides
    if max(shape) >= 2 ** 32:
        raise ValueError("%s: the view is too large" % what)
    ptr = (x.data_ptr() if _is_torch(x) else x.ctypes.data) if b * h * w else 0
    if b * h * w == 0:
        return ptr, b, h, w, w, h * w, h * w
    if w > 1 and sc != 1:
        raise ValueError("%s: the last dimension must have stride 1, not %d" % (what, sc))
    if h > 1 and sr < w:
        raise ValueError("%s: the row stride %d is smaller than the width %d" % (what, sr, w))
    pitch = sr if h > 1 else w
    span = (h - 1) * pitch + w
    if b > 1 and sf < span:
        raise ValueError("%s: the frame stride %d is smaller than a frame's span %d" % (what, sf, span))
    return ptr, b, h, w, pitch, (sf if b > 1 else span), span


def _view_out(out, like, lay, what, name="out"):
    """`out=` of a view call (or the output argument called `name`): None (a packed buffer of the input's shape is allocated
    beside it) or a view of the input's kind, shape and device whose byte span does not meet the input's.  Returns (out, its
    layout)."""
    if out is None:
        if _is_torch(like):
            import torch
            out = torch.empty(tuple(like.shape), dtype=torch.uint8, device=like.device)
        else:
            out = np.empty(like.shape, np.uint8)
        return out, _view_layout(out, what)
    if _is_torch(like) != _is_torch(out):
        raise ValueError("%s: `%s` must be a %s like the input" % (what, name, "torch tensor" if _is_torch(like) else "numpy array"))
    olay = _view_layout(out, "%s (%s)" % (what, name))
    if tuple(out.shape) != tuple(like.shape):
        raise ValueError("%s: `%s` has shape %s, the input %s" % (what, name, tuple(out.shape), tuple(like.shape)))
    if _is_torch(like):
        if out.device != like.device:
            raise ValueError("%s: `%s` lives on %s, the input on %s" % (what, name, out.device, like.device))
    elif not out.flags["WRITEABLE"]:
        raise ValueError("%s: `%s` is not writable" % (what, name))
    (a0, ab, _, _, _, afs, aspan), (b0, bb, _, _, _, bfs, bspan) = lay, olay
    if ab and a0 < b0 + (bb - 1) * bfs + bspan and b0 < a0 + (ab - 1) * afs + aspan:
        raise ValueError("%s: `%s` shares memory with the input (byte spans, tested conservatively)" % (what, name))
    return out, olay


def _view_device(x, what):
    if _is_torch(x) and not x.is_cuda:
        raise ValueError("%s: torch tensors must live on the GPU (use numpy for host buffers)" % what)


def _typed_view_layout(x, what, dtype, esize):
    """_view_layout's sibling for the output of a mapped decode: a (height, width) or (batch, height, width) view of `dtype`
    elements, `esize` bytes each, whose last dimension has stride 1 ELEMENT, whose rows lie >= width elements apart and whose
    frames lie >= one frame's span apart.  Returns (ptr, batch, height, width, pitch, frame_stride, span) with pitch, stride and
    span in BYTES, span = (height - 1) * pitch + width * esize.  Nothing here touches a device."""
    if _is_torch(x):
        if x.dtype != dtype:
            raise ValueError("%s: expected a %s tensor, not %s" % (what, dtype, x.dtype))
        shape, strides = tuple(int(v) for v in x.shape), tuple(int(v) for v in x.stride())
    elif isinstance(x, np.ndarray):
        if x.dtype != dtype:
            raise ValueError("%s: expected a %s array, not %s" % (what, dtype, x.dtype))
        if any(int(v) % esize for v in x.strides):
            raise ValueError("%s: strides %s are not whole elements" % (what, x.strides))
        shape, strides = tuple(int(v) for v in x.shape), tuple(int(v) // esize for v in x.strides)
    else:
        raise ValueError("%s: expected a torch CUDA tensor or numpy array of %s" % (what, dtype))
    if len(shape) not in (2, 3):
        raise ValueError("%s: expected a (height, width) or (batch, height, width) view, not %d dimensions" % (what, len(shape)))
    if len(shape) == 2:
        shape, strides = (1,) + shape, (0,) + strides
    (b, h, w), (sf, sr, sc) = shape, strides
    if max(shape) >= 2 ** 32:
        raise ValueError("%s: the view is too large" % what)
    if b * h * w == 0:
        return 0, b, h, w, w * esize, h * w * esize, h * w * esize
    ptr = x.data_ptr() if _is_torch(x) else x.ctypes.data
    if w > 1 and sc != 1:
        raise ValueError("%s: the last dimension must have stride 1, not %d" % (what, sc))
    if h > 1 and sr < w:
        raise ValueError("%s: the row stride %d is smaller than the width %d" % (what, sr, w))
    pitch = sr if h > 1 else w
    span = (h - 1) * pitch + w
    if b > 1 and sf < span:
        raise ValueError("%s: the frame stride %d is smaller than a frame's span %d" % (what, sf, span))
    return ptr, b, h, w, pitch * esize, (sf if b > 1 else span) * esize, span * esize


def _map_table(table, grids, what):
    """The table of a mapped decode: 256 contiguous elements of 2 or 4 bytes -- a 1-D torch tensor on the grids' device, or a
    numpy array (torch grids: uploaded per call).  Returns (dtype of the output, element size, byte range or None)."""
    if _is_torch(table):
        if not _is_torch(grids):
            raise ValueError("%s: a torch `table` goes with torch grids (numpy grids take a numpy table)" % what)
        if table.dim() != 1 or table.numel() != 256 or not table.is_contiguous():
            raise ValueError("%s: `table` must be a contiguous 1-D tensor of 256 elements, not shape %s" % (what, tuple(table.shape)))
        esize = int(table.element_size())
        if esize not in (2, 4) or table.is_complex():
            raise ValueError("%s: `table` elements must be 2 or 4 bytes, not %s" % (what, table.dtype))
        if table.device != grids.device:
            raise ValueError("%s: `table` lives on %s, the grids on %s" % (what, table.device, grids.device))
        return table.dtype, esize, (table.data_ptr(), table.data_ptr() + 256 * esize)
    if not isinstance(table, np.ndarray):
        raise ValueError("%s: `table` must be a torch tensor or numpy array of 256 elements" % what)
    if table.ndim != 1 or table.shape[0] != 256 or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("%s: `table` must be a contiguous 1-D array of 256 elements, not shape %s" % (what, table.shape))
    esize = int(table.dtype.itemsize)
    if esize not in (2, 4) or table.dtype.kind not in "fiu":
        raise ValueError("%s: `table` elements must be 2 or 4 bytes, not %s" % (what, table.dtype))
    if _is_torch(grids):
        import torch
        try:
            return torch.from_numpy(np.empty(0, table.dtype)).dtype, esize, None
        except TypeError:
            raise ValueError("%s: torch has no dtype for a %s `table`: pass a tensor" % (what, table.dtype))
    return table.dtype, esize, (table.ctypes.data, table.ctypes.data + 256 * esize)


def _views_launch(plan, ctx, fused, each, check=None):
    """One view-list call on plan.device: `fused(stream, d_plan, info)` -> status of the one launch; `each(ctx, view layout)` ->
    status of one pitched call, composed per view when the plan or the launch is not served (HGI_EUNSUPPORTED).  `check`: what
    raises for a launch status of another library than libhgi_views.so.  Returns the plan's destination views."""
    import torch
    from . import _ffi_views
    if len(plan) == 0 or plan.device is None:
        return list(plan.dsts)
    dev = plan.device.index if plan.device.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != dev:      # both routes judge the context alike (_bind_ctx)
        raise ValueError("the views live on cuda:%d but the context was created for cuda:%d" % (dev, ctx.device))
    st = _ffi.EUNSUPPORTED
    if plan.fused:
        if plan.blob is None:      # only empty views
            return list(plan.dsts)
        with torch.cuda.device(dev):
            st = fused(_ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), plan.blob.data_ptr(), ctypes.addressof(plan.info))
    if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from one pitched call per view
        bound = _bind_ctx(plan.srcs[0], ctx)
        for lay in plan.layouts:
            if lay[2] and lay[3]:
                _ffi.check(each(bound, lay))
        return list(plan.dsts)
    (check or _ffi_views.check)(st)
    return list(plan.dsts)


def _np_image(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected a (height, width) uint8 image")
    return a


class Encoder:
    """`Encoder::new(interpolator, quantizator, scale_level)` -- src/encoder.rs:18."""

    def __init__(self, interpolator, quantizator, scale_level, context=None):
        if not isinstance(interpolator, Interpolator) or not isinstance(quantizator, Quantizator):
            raise TypeError("Encoder(interpolator: Interpolator, quantizator: Quantizator, scale_level)")
        self.interpolator, self.quantizator = interpolator, quantizator
        self._interp = _interp_id(interpolator)
        self.scale_level = int(scale_level)
        self._lut = np.ascontiguousarray(quantizator.table(), dtype=np.uint8)
        self._ctx = context

    def encode(self, image):
        """`encode(GrayImage) -> Grid` -- src/encoder.rs:39.  The input is not modified."""
        if _is_torch(image):
            if image.dim() != 2:
                raise ValueError("expected a (height, width) image; use encode_batch for stacks")
            out = self.encode_batch(image.unsqueeze(0))
            return Grid(out[0], image.shape[1])
        img = _np_image(image)
        h, w = img.shape
        grid = np.empty_like(img)
        ctx = self._ctx or _ffi.default_context(0)
        _ffi.check(_ffi.lib().hgi_encode_u8(ctx.handle, img.ctypes.data, w, h, self.scale_level,
                                            self._interp, self._lut.ctypes.data,
                                            grid.ctypes.data))
        return Grid(grid, w)

    def encode_batch(self, images, out=None):
        """(B, H, W) uint8 CUDA tensor -> (B, H, W) residual planes, asynchronous on the current stream.
        A (B, H, W) numpy array (host memory) goes through hgi_encode_u8_batch instead: synchronous, the frames
        pipelined through the device so that uploads overlap downloads."""
        if not _is_torch(images):
            imgs = np.ascontiguousarray(images, dtype=np.uint8)
            if imgs.ndim != 3:
                raise ValueError("expected a (batch, height, width) stack")
            b, h, w = imgs.shape
            out = np.empty_like(imgs) if out is None else _check_out(out, imgs, "encode_batch")
            ctx = self._ctx or _ffi.default_context(0)
            _ffi.check(_ffi.lib().hgi_encode_u8_batch(ctx.handle, imgs.ctypes.data, w, h, self.scale_level, self._interp,
                                                      self._lut.ctypes.data, out.ctypes.data, b, h * w))
            return out
        import torch
        ctx = _torch_ctx(images, self._ctx)
        if images.dim() != 3:
            raise ValueError("expected a (batch, height, width) stack")
        b, h, w = images.shape
        out = torch.empty_like(images) if out is None else _check_out(out, images, "encode_batch")
        _ffi.check(_ffi.lib().hgi_encode_u8_dev(ctx.handle, images.data_ptr(), w, h, self.scale_level,
                                                self._interp, self._lut.ctypes.data,
                                                out.data_ptr(), b, h * w))
        return out

    def encode_view(self, images, out=None):
        """Encode a VIEW: a (H, W) or (B, H, W) uint8 slice t[f0:f1, y0:y1, x0:x1] of a larger buffer -- last dimension stride 1,
        any row stride >= W, a uniform frame stride -- where it lies, without a packing copy.  `out` may be such a view too (only
        its W-byte rows are written); without it a packed buffer of the input's shape is returned.  The result, read through its
        strides, is bit for bit `encode_batch` of the packed copy.  CUDA tensors: one hgi_encode_u8_pitched_dev call, asynchronous
        on the current stream; numpy arrays: hgi_encode_u8_pitched frame by frame.  Layouts, dtype, device, shape and overlap are
        validated (ValueError) before the library is called."""
        lay = _view_layout(images, "encode_view")
        if out is None:
            _view_device(images, "encode_view")
        out, olay = _view_out(out, images, lay, "encode_view")
        _view_device(images, "encode_view")      # (a given `out` is judged first: its faults are the caller's to see on any machine)
        (src, b, h, w, sp, sfs, _), (dst, _, _, _, dp, dfs, _) = lay, olay
        if b * h * w == 0:
            return out
        if _is_torch(images):
            ctx = _bind_ctx(images, self._ctx)
            _ffi.check(_ffi.lib().hgi_encode_u8_pitched_dev(ctx.handle, src, sp, w, h, self.scale_level, self._interp,
                                                            self._lut.ctypes.data, dst, dp, b, sfs, dfs))
            return out
        ctx = self._ctx or _ffi.default_context(0)
        for f in range(b):
            _ffi.check(_ffi.lib().hgi_encode_u8_pitched(ctx.handle, src + f * sfs, sp, w, h, self.scale_level, self._interp,
                                                        self._lut.ctypes.data, dst + f * dfs, dp))
        return out

    def encode_with_reconstruction(self, images, out=None, recon=None):
        """Encode a view AND return the image the decoder will make of the grid: `(grid, recon)`, where `grid` is bit for bit
        `encode_view(images)` and `recon` bit for bit `Decoder.decode_view(grid, scale_level)` -- what the reference's
        `Encoder::encode` leaves in its input (src/encoder.rs:63-64).  `images`, `out` and `recon` are views as for `encode_view`
        ((H, W) or (B, H, W), any row stride >= W); only the W-byte rows of the two outputs are written, the input is not
        modified, and none of the three may share memory with another.  CUDA tensors: ONE hgi_recon_encode_u8_dev launch
        (libhgi_recon.so), asynchronous on the current stream -- 3 B/px instead of the 4 B/px of encode + decode.  What that
        launch does not serve (HGI_EUNSUPPORTED: 0 or more than 8 levels, offsets beyond 32 bits, a width that is no multiple
        of 4 with the input's last bytes at the end of a 4-KiB page) is composed from `encode_view` + `decode_view` on the same
        stream: the same bytes, not fused.  numpy arrays are uploaded and downloaded through torch tensors, synchronously.
        Validated (ValueError) before any device call; empty inputs need no device."""
        what = "encode_with_reconstruction"
        lay = _view_layout(images, what)
        if out is None and recon is None:
            _view_device(images, what)
        out, olay = _view_out(out, images, lay, what)
        recon, rlay = _view_out(recon, images, lay, what, name="recon")
        (g0, gb, _, _, _, gfs, gspan), (r0, _, _, _, _, rfs, rspan) = olay, rlay
        if gb and g0 < r0 + (gb - 1) * rfs + rspan and r0 < g0 + (gb - 1) * gfs + gspan:
            raise ValueError("%s: `recon` shares memory with `out` (byte spans, tested conservatively)" % what)
        _view_device(images, what)
        (src, b, h, w, sp, sfs, _) = lay
        if b * h * w == 0:
            return out, recon
        if not _is_torch(images):
            import torch
            if not torch.cuda.is_available():
                raise _ffi.HgiError(_ffi.EDEVICE, "%s needs a GPU (there is no CPU fallback)" % what)
            dev = self._ctx.device if self._ctx is not None else 0
            t = torch.from_numpy(np.ascontiguousarray(images)).to("cuda:%d" % dev)
            g, r = self.encode_with_reconstruction(t)
            out[...] = g.cpu().numpy()
            recon[...] = r.cpu().numpy()
            return out, recon
        import torch
        from . import _ffi_recon
        dev = images.device.index if images.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Encoder's context alike (_bind_ctx)
            raise ValueError("tensor lives on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        with torch.cuda.device(dev):
            st = _ffi_recon.lib().hgi_recon_encode_u8_dev(
                _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), src, sp, w, h, self.scale_level, self._interp,
                self._lut.ctypes.data, olay[0], olay[4], rlay[0], rlay[4], b, sfs, olay[5], rlay[5])
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from two calls
            self.encode_view(images, out=out)
            Decoder(self.interpolator, context=self._ctx).decode_view(out, self.scale_level, out=recon)
            return out, recon
        _ffi_recon.check(st)
        return out, recon

    def requantize(self, grids, out=None):
        """Re-code GRIDS with this encoder's table: bit for bit `encode_view(Decoder(interpolator).decode_view(grids,
        scale_level))`, without the decoded image ever reaching memory.  A grid stores dequantized residuals, so the quantizer
        is a property of the encode alone; the grids must have been made with this encoder's interpolator and `scale_level`
        (a change of either stays a decode and an encode by the caller).  `grids` and `out` are views as for `decode_view`
        ((H, W) or (B, H, W) uint8, any row stride >= W); only the W-byte rows of `out` are written, the grids are not modified,
        and `out` must not share memory with them.  CUDA tensors: ONE hgi_requant_dev launch (libhgi_requant.so), asynchronous on
        the current stream -- 2 B/px instead of the 4 B/px of decode + encode.  What that launch does not serve
        (HGI_EUNSUPPORTED: 0 or more than 8 levels, offsets beyond 32 bits, a width that is no multiple of 4 with the grids' last
        bytes at the end of a 4-KiB page) is composed from `decode_view` into a temporary + `encode_view` on the same stream;
        under the identity table the result is the source at ANY depth (decode is a bijection on grids and the identity encode
        its inverse) and the rows are copied without a call of the library.  The same bytes, not fused.  numpy arrays are
        uploaded and downloaded through torch tensors, synchronously.  Validated (ValueError) before any device call; empty
        inputs need no device."""
        what = "requantize"
        lay = _view_layout(grids, what)
        empty = lay[1] * lay[2] * lay[3] == 0
        if out is None and not empty:
            _view_device(grids, what)
        out, olay = _view_out(out, grids, lay, what)
        (src, b, h, w, sp, sfs, _), (dst, _, _, _, dp, dfs, _) = lay, olay
        if empty:
            return out
        _view_device(grids, what)      # (a given `out` is judged first: its faults are the caller's to see on any machine)
        if not _is_torch(grids):
            import torch
            if not torch.cuda.is_available():
                raise _ffi.HgiError(_ffi.EDEVICE, "%s needs a GPU (there is no CPU fallback)" % what)
            dev = self._ctx.device if self._ctx is not None else 0
            t = torch.from_numpy(np.ascontiguousarray(grids)).to("cuda:%d" % dev)
            out[...] = self.requantize(t).cpu().numpy()
            return out
        import torch
        from . import _ffi_requant
        dev = grids.device.index if grids.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Encoder's context alike (_bind_ctx)
            raise ValueError("tensor lives on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        if 0 <= self.scale_level <= 31 and bool((self._lut == np.arange(256, dtype=np.uint8)).all()):
            # The identity table keeps every residual d = a - p, and a and p are what the decoder made of the same grid: at any
            # depth encode(decode(g), identity) == g (decode is a bijection on grids and this encode is its inverse).
            out.copy_(grids)
            return out
        with torch.cuda.device(dev):
            st = _ffi_requant.lib().hgi_requant_dev(
                _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), src, sp, w, h, self.scale_level, self._interp,
                self._lut.ctypes.data, dst, dp, b, sfs, dfs)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from two calls
            image = Decoder(self.interpolator, context=self._ctx).decode_view(grids, self.scale_level)
            self.encode_view(image, out=out)
            return out
        _ffi_requant.check(st)
        return out

    def requantize_views(self, plan):
        """Re-code a VIEW LIST of stored grids with this encoder's table: `plan` is a `rustyhgi_amd.views.ViewPlan` of (source
        grid view, destination grid view) pairs -- every pair with a shape and two row pitches of its own; a plan that served
        `encode_views` or `decode_views` serves here unchanged.  Each destination view, read through its pitch, is bit for bit
        `requantize` of its source view alone; only the W-byte rows of the destinations are written, the sources are not
        modified.  ONE hgi_qviews_requant_dev launch (libhgi_qviews.so), asynchronous on the current stream and capturable into
        a graph -- 2 B/px where `decode_views` into a uint8 arena + `encode_views` moves 4 B/px; the plan may be launched any
        number of times.  What that launch does not serve (HGI_EUNSUPPORTED: 0 or more than 8 levels, or a plan that is not
        fused) is composed from one `requantize(src, out=dst)` per view: the same bytes.  Under the identity table the result
        is the source, and the rows are copied per view without a call of the library.  Returns the destination views; empty
        plans need no device."""
        from . import _ffi_qviews
        lut, levels, interp = self._lut.ctypes.data, self.scale_level, self._interp
        pairs = dict((lay, (s, d)) for lay, s, d in zip(plan.layouts, plan.srcs, plan.dsts) if lay[2] and lay[3])

        def fused(stream, blob, info):
            if 0 <= levels <= 31 and bool((self._lut == np.arange(256, dtype=np.uint8)).all()):
                for s, d in pairs.values():      # (`requantize` says why the source is the result at any depth)
                    d.copy_(s)
                return _ffi.OK
            return _ffi_qviews.lib().hgi_qviews_requant_dev(stream, blob, info, levels, interp, lut)

        def each(ctx, v):
            self.requantize(pairs[v][0], out=pairs[v][1])
            return _ffi.OK

        return _views_launch(plan, self._ctx, fused, each, check=_ffi_qviews.check)

    def encode_typed(self, frames, scale=255.0, bias=0.0, out=None):
        """Encode float frames where they lie: a (H, W) or (B, H, W) torch CUDA tensor of float16, bfloat16 or float32 -- a view
        as for `encode_view`, strides counted in elements -- becomes the grids of the uint8 image `v = clamp(rint(x * scale +
        bias), 0, 255)`, NaN -> 0: two separately rounded float32 operations, round half to even, denormals kept
        (include/hgi_typed.h).  The defaults invert `affine_table(dtype)`; `rustyhgi_amd.affine_inverse(s, b)` gives the pair
        that inverts `affine_table(dtype, s, b)`.  `out` may be a uint8 view (only its W-byte rows are written); without it a
        packed uint8 tensor of the frames' shape is returned.  The result is bit for bit `encode_view` of that uint8 image, which
        never reaches memory: ONE hgi_typed_encode_dev launch (libhgi_typed.so), asynchronous on the current stream -- E + 1
        B/px instead of the E + 3 B/px of a conversion and an encode.  What that launch does not serve (HGI_EUNSUPPORTED: 0 or
        more than 8 levels, offsets beyond 32 bits, 2-byte elements of an odd width whose last byte ends a 4-KiB page) is
        composed from the torch conversion and `encode_view` on the same stream: the same bytes, not fused.  Validated
        (ValueError) before any device call; empty inputs need no device."""
        what = "encode_typed"
        if not _is_torch(frames):
            raise ValueError("%s: expected a float16, bfloat16 or float32 torch CUDA tensor" % what)
        import torch
        kinds = {torch.float16: (2, 0), torch.bfloat16: (2, 1), torch.float32: (4, 0)}      # dtype -> (elem_size, elem_kind)
        if frames.dtype not in kinds:
            raise ValueError("%s: expected a float16, bfloat16 or float32 tensor, not %s" % (what, frames.dtype))
        esize, kind = kinds[frames.dtype]
        lay = _typed_view_layout(frames, what, frames.dtype, esize)
        with np.errstate(over="ignore"):
            scale, bias = np.float32(scale), np.float32(bias)
        if not (np.isfinite(scale) and np.isfinite(bias)):
            raise ValueError("%s: `scale` and `bias` must be finite float32 values" % what)
        if out is None:
            if lay[1] * lay[2] * lay[3]:
                _view_device(frames, what)
            out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
            olay = _view_layout(out, what)
        else:
            if not _is_torch(out):
                raise ValueError("%s: `out` must be a torch tensor like the frames" % what)
            olay = _view_layout(out, "%s (out)" % what)
            if tuple(out.shape) != tuple(frames.shape):
                raise ValueError("%s: `out` has shape %s, the frames %s" % (what, tuple(out.shape), tuple(frames.shape)))
            if out.device != frames.device:
                raise ValueError("%s: `out` lives on %s, the frames on %s" % (what, out.device, frames.device))
        (src, b, h, w, sp, sfs, ispan), (dst, _, _, _, dp, dfs, gspan) = lay, olay
        if b * h * w and src < dst + (b - 1) * dfs + gspan and dst < src + (b - 1) * sfs + ispan:
            raise ValueError("%s: `out` shares memory with the frames (byte spans, tested conservatively)" % what)
        if b * h * w == 0:
            return out
        _view_device(frames, what)
        from . import _ffi_typed
        dev = frames.device.index if frames.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Encoder's context alike (_bind_ctx)
            raise ValueError("tensor lives on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        with torch.cuda.device(dev):
            st = _ffi_typed.lib().hgi_typed_encode_dev(
                _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), src, sp, esize, kind, float(scale), float(bias), w, h,
                self.scale_level, self._interp, self._lut.ctypes.data, dst, dp, b, sfs, dfs)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from a conversion and an encode
            t = torch.add(torch.mul(frames.to(torch.float32), float(scale)), float(bias))      # two roundings, as the launch does
            px = torch.where(torch.isnan(t), torch.zeros_like(t), t).round().clamp(0, 255).to(torch.uint8)
            self.encode_view(px, out=out)
            return out
        _ffi_typed.check(st)
        return out

    def encode_views(self, plan):
        """Encode a VIEW LIST: `plan` is a `rustyhgi_amd.views.ViewPlan` of (image view, grid view) pairs -- every pair with a
        shape and two row pitches of its own.  Each destination view, read through its pitch, is bit for bit `encode_view` of
        its source view alone; only the W-byte rows of the destinations are written.  ONE hgi_views_encode_dev launch
        (libhgi_views.so), asynchronous on the current stream and capturable into a graph; the plan may be launched any number
        of times.  What that launch does not serve (HGI_EUNSUPPORTED: 0 or more than 8 levels, an entry beyond the 32-bit
        buffer path or with its last source bytes at the end of a 4-KiB page) is composed from one hgi_encode_u8_pitched_dev
        call per view: the same bytes, not fused.  Returns the destination views."""
        from . import _ffi_views
        lut, levels, interp = self._lut.ctypes.data, self.scale_level, self._interp
        return _views_launch(
            plan, self._ctx,
            lambda stream, blob, info: _ffi_views.lib().hgi_views_encode_dev(stream, blob, info, levels, interp, lut),
            lambda ctx, v: _ffi.lib().hgi_encode_u8_pitched_dev(ctx.handle, v[0], v[4], v[2], v[3], levels, interp, lut, v[1], v[5], 1, 0, 0))

    def encode_views_with_reconstruction(self, plan):
        """Encode a RECON VIEW LIST: `plan` is a `rustyhgi_amd.rviews.ReconViewPlan` of (image view, grid view, reconstruction
        view) triples -- every triple with a shape and three row pitches of its own.  Each grid view, read through its pitch, is
        bit for bit `encode_view` of its source view alone and each reconstruction view bit for bit `Decoder.decode_view` of that
        grid; only the W-byte rows of the two outputs are written, the sources are not modified.  ONE hgi_rviews_encode_dev
        launch (libhgi_rviews.so), asynchronous on the current stream and capturable into a graph -- 3 B/px where `encode_views`
        + `decode_views` move 4 B/px; the plan may be launched any number of times.  What that launch does not serve
        (HGI_EUNSUPPORTED: 0 or more than 8 levels, or a plan that is not fused) is composed from one
        `encode_with_reconstruction(src, out=grid, recon=recon)` per view: the same bytes.  Returns `(grid views, recon views)`;
        empty plans need no device."""
        done = (list(plan.grids), list(plan.recons))
        if len(plan) == 0 or plan.device is None:
            return done
        import torch
        from . import _ffi_rviews
        dev = plan.device.index if plan.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Encoder's context alike (_bind_ctx)
            raise ValueError("the views live on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        st = _ffi.EUNSUPPORTED
        if plan.fused:
            if plan.blob is None:      # only empty views
                return done
            with torch.cuda.device(dev):
                st = _ffi_rviews.lib().hgi_rviews_encode_dev(
                    _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), plan.blob.data_ptr(), ctypes.addressof(plan.info),
                    self.scale_level, self._interp, self._lut.ctypes.data)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from one encode with reconstruction per view
            for s, g, r in zip(plan.srcs, plan.grids, plan.recons):
                if s.numel():
                    self.encode_with_reconstruction(s, out=g, recon=r)
            return done
        _ffi_rviews.check(st)
        return done

    def encode_typed_views(self, plan, scale=255.0, bias=0.0):
        """Encode a TYPED VIEW LIST: `plan` is a `rustyhgi_amd.tviews.TypedViewPlan` of (float frame view, grid view) pairs --
        every pair with a shape and two row pitches of its own.  Each destination view, read through its pitch, is bit for bit
        `encode_typed` of its source view alone under `scale` and `bias`; only the W-byte rows of the destinations are written.
        ONE hgi_tviews_encode_dev launch (libhgi_tviews.so), asynchronous on the current stream and capturable into a graph; the
        plan may be launched any number of times.  A plan or a depth that launch does not serve (HGI_EUNSUPPORTED) is composed
        from one `encode_typed` call per view: the same bytes.  Returns the destination views; empty plans need no device."""
        what = "encode_typed_views"
        with np.errstate(over="ignore"):
            scale, bias = np.float32(scale), np.float32(bias)
        if not (np.isfinite(scale) and np.isfinite(bias)):
            raise ValueError("%s: `scale` and `bias` must be finite float32 values" % what)
        if len(plan) == 0 or plan.device is None:
            return list(plan.dsts)
        import torch
        from . import _ffi_tviews
        dev = plan.device.index if plan.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Encoder's context alike (_bind_ctx)
            raise ValueError("the views live on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        st = _ffi.EUNSUPPORTED
        if plan.fused:
            if plan.blob is None:      # only empty views
                return list(plan.dsts)
            kind = 1 if plan.dtype == torch.bfloat16 else 0
            with torch.cuda.device(dev):
                st = _ffi_tviews.lib().hgi_tviews_encode_dev(
                    _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), plan.blob.data_ptr(), ctypes.addressof(plan.info), kind,
                    float(scale), float(bias), self.scale_level, self._interp, self._lut.ctypes.data)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from one typed encode per view
            for s, d in zip(plan.srcs, plan.dsts):
                if s.numel():
                    self.encode_typed(s, float(scale), float(bias), out=d)
            return list(plan.dsts)
        _ffi_tviews.check(st)
        return list(plan.dsts)

    def encode_list(self, images, out=None):
        """A list of (h_i, w_i) uint8 frames of any shapes -> the list of their residual planes.  CUDA tensors (one device,
        contiguous): ONE hgi_encode_u8_list_dev call, asynchronous on the current stream, the outputs (h_i, w_i) views into one
        allocation unless `out` (a list of tensors) is given.  numpy arrays: hgi_encode_u8 frame by frame.  The list and `out`
        are validated before any device call."""
        frames, use_torch = _check_list(images, out, "encode_list")
        if not use_torch:
            outs = [np.empty_like(f) for f in frames] if out is None else list(out)
            ctx = self._ctx or _ffi.default_context(0) if any(f.size for f in frames) else None
            for f, o in zip(frames, outs):
                if f.size:
                    _ffi.check(_ffi.lib().hgi_encode_u8(ctx.handle, f.ctypes.data, f.shape[1], f.shape[0], self.scale_level,
                                                        self._interp, self._lut.ctypes.data, o.ctypes.data))
            return outs
        ctx = _torch_ctx(frames[0], self._ctx)
        outs = _list_out(frames) if out is None else list(out)
        ins, ws, hs, ptrs = _list_arrays(frames, outs)
        _ffi.check(_ffi.lib().hgi_encode_u8_list_dev(ctx.handle, ins, ws, hs, self.scale_level, self._interp,
                                                     self._lut.ctypes.data, ptrs, len(frames)))
        return outs


class Decoder:
    """`Decoder::new(interpolator)` -- src/decoder.rs:14."""

    def __init__(self, interpolator, context=None):
        if not isinstance(interpolator, Interpolator):
            raise TypeError("Decoder(interpolator: Interpolator)")
        self.interpolator = interpolator
        self._interp = _interp_id(interpolator)
        self._ctx = context

    def decode(self, dimensions, levels, grid):
        """`decode((width, height), levels, &Grid) -> GrayImage` -- src/decoder.rs:18."""
        width, height = int(dimensions[0]), int(dimensions[1])
        buf = grid.buffer if isinstance(grid, Grid) else grid
        if _is_torch(buf):
            return self.decode_batch(buf.reshape(1, height, width), levels)[0]
        g = np.ascontiguousarray(buf, dtype=np.uint8).reshape(height, width)
        img = np.empty_like(g)
        ctx = self._ctx or _ffi.default_context(0)
        _ffi.check(_ffi.lib().hgi_decode_u8(ctx.handle, g.ctypes.data, width, height, int(levels),
                                            self._interp, img.ctypes.data))
        return img

    def decode_batch(self, grids, levels, out=None):
        """CUDA tensor: asynchronous on the current stream; numpy stack: hgi_decode_u8_batch (see Encoder.encode_batch)."""
        if not _is_torch(grids):
            g = np.ascontiguousarray(grids, dtype=np.uint8)
            if g.ndim != 3:
                raise ValueError("expected a (batch, height, width) stack")
            b, h, w = g.shape
            out = np.empty_like(g) if out is None else _check_out(out, g, "decode_batch")
            ctx = self._ctx or _ffi.default_context(0)
            _ffi.check(_ffi.lib().hgi_decode_u8_batch(ctx.handle, g.ctypes.data, w, h, int(levels), self._interp,
                                                      out.ctypes.data, b, h * w))
            return out
        import torch
        ctx = _torch_ctx(grids, self._ctx)
        if grids.dim() != 3:
            raise ValueError("expected a (batch, height, width) stack")
        b, h, w = grids.shape
        out = torch.empty_like(grids) if out is None else _check_out(out, grids, "decode_batch")
        _ffi.check(_ffi.lib().hgi_decode_u8_dev(ctx.handle, grids.data_ptr(), w, h, int(levels),
                                                self._interp, out.data_ptr(), b, h * w))
        return out

    def decode_view(self, grids, levels, out=None):
        """Decode a VIEW of grids (see Encoder.encode_view for the layouts) into `out` -- a window of a canvas, say -- or into a
        packed buffer.  Only the W-byte rows of `out` are written.  Bit for bit `decode_batch` of the packed copy.  CUDA tensors:
        one hgi_decode_u8_pitched_dev call, asynchronous on the current stream; numpy arrays: hgi_decode_u8_pitched frame by
        frame.  Validated (ValueError) before the library is called."""
        lay = _view_layout(grids, "decode_view")
        if out is None:
            _view_device(grids, "decode_view")
        out, olay = _view_out(out, grids, lay, "decode_view")
        _view_device(grids, "decode_view")      # (a given `out` is judged first: its faults are the caller's to see on any machine)
        (src, b, h, w, sp, sfs, _), (dst, _, _, _, dp, dfs, _) = lay, olay
        if b * h * w == 0:
            return out
        if _is_torch(grids):
            ctx = _bind_ctx(grids, self._ctx)
            _ffi.check(_ffi.lib().hgi_decode_u8_pitched_dev(ctx.handle, src, sp, w, h, int(levels), self._interp, dst, dp, b, sfs,
                                                            dfs))
            return out
        ctx = self._ctx or _ffi.default_context(0)
        for f in range(b):
            _ffi.check(_ffi.lib().hgi_decode_u8_pitched(ctx.handle, src + f * sfs, sp, w, h, int(levels), self._interp,
                                                        dst + f * dfs, dp))
        return out

    def decode_region(self, dimensions, levels, grid, rect):
        """The window rect = (x0, y0, w, h) of `decode(dimensions, levels, grid)` as an (h, w) array, bit for bit -- computed by
        the tiles that cover the window only.  numpy grid: hgi_decode_region_u8 (synchronous); CUDA tensor: a tensor, asynchronous
        on the current stream (hgi_decode_region_u8_dev)."""
        width, height = int(dimensions[0]), int(dimensions[1])
        x0, y0, w, h = _check_rect(rect, width, height, "decode_region")
        buf = grid.buffer if isinstance(grid, Grid) else grid
        if _is_torch(buf):
            if buf.numel() != width * height:
                raise ValueError("decode_region: the grid holds %d bytes, not %dx%d" % (buf.numel(), width, height))
            return self.decode_region_batch(buf.reshape(1, height, width), levels, (x0, y0, w, h))[0]
        g = np.ascontiguousarray(buf, dtype=np.uint8)
        if g.size != width * height:
            raise ValueError("decode_region: the grid holds %d bytes, not %dx%d" % (g.size, width, height))
        g = g.reshape(height, width)
        img = np.empty((h, w), np.uint8)
        if w == 0 or h == 0:
            return img
        ctx = self._ctx or _ffi.default_context(0)
        _ffi.check(_ffi.lib().hgi_decode_region_u8(ctx.handle, g.ctypes.data, width, height, int(levels), self._interp,
                                                   x0, y0, w, h, img.ctypes.data, w))
        return img

    def decode_region_batch(self, grids, levels, rect, out=None):
        """(B, H, W) grids -> (B, h, w): the same window of every frame.  CUDA tensor: one hgi_decode_region_u8_dev launch,
        asynchronous on the current stream; numpy stack: hgi_decode_region_u8 frame by frame.  The window and `out` are
        validated before any device call."""
        if grids.ndim != 3:
            raise ValueError("expected a (batch, height, width) stack")
        b, height, width = (int(v) for v in grids.shape)
        x0, y0, w, h = _check_rect(rect, width, height, "decode_region_batch")
        if not _is_torch(grids):
            g = np.ascontiguousarray(grids, dtype=np.uint8)
            out = np.empty((b, h, w), np.uint8) if out is None else _check_region_out(out, g, (b, h, w), "decode_region_batch")
            for f in range(b):
                out[f] = self.decode_region((width, height), levels, g[f], (x0, y0, w, h))
            return out
        import torch
        if out is not None:
            _check_region_out(out, grids, (b, h, w), "decode_region_batch")
        ctx = _torch_ctx(grids, self._ctx)
        if out is None:
            out = torch.empty((b, h, w), dtype=torch.uint8, device=grids.device)
        _ffi.check(_ffi.lib().hgi_decode_region_u8_dev(ctx.handle, grids.data_ptr(), width, height, int(levels), self._interp,
                                                       x0, y0, w, h, out.data_ptr(), w, b, height * width, h * w))
        return out

    def decode_scaled(self, dimensions, levels, grid, shift):
        """`decode(dimensions, levels, grid)[::2**shift, ::2**shift]` as an (sh, sw) array, bit for bit -- decoded from the grid
        bytes of that lattice with levels - shift levels.  numpy grid: hgi_decode_scaled_u8 (synchronous, uploads only the rows
        it reads); CUDA tensor: a tensor, asynchronous on the current stream (hgi_decode_scaled_u8_dev)."""
        shift = _check_shift(shift, "decode_scaled")
        width, height = int(dimensions[0]), int(dimensions[1])
        sw, sh = scaled_size(width, height, shift)
        buf = grid.buffer if isinstance(grid, Grid) else grid
        if _is_torch(buf):
            if buf.numel() != width * height:
                raise ValueError("decode_scaled: the grid holds %d bytes, not %dx%d" % (buf.numel(), width, height))
            return self.decode_scaled_batch(buf.reshape(1, height, width), levels, shift)[0]
        g = np.ascontiguousarray(buf, dtype=np.uint8)
        if g.size != width * height:
            raise ValueError("decode_scaled: the grid holds %d bytes, not %dx%d" % (g.size, width, height))
        g = g.reshape(height, width)
        img = np.empty((sh, sw), np.uint8)
        if width == 0 or height == 0:
            return img
        ctx = self._ctx or _ffi.default_context(0)
        _ffi.check(_ffi.lib().hgi_decode_scaled_u8(ctx.handle, g.ctypes.data, width, height, int(levels), self._interp, shift,
                                                   img.ctypes.data, sw))
        return img

    def decode_scaled_batch(self, grids, levels, shift, out=None):
        """(B, H, W) grids -> (B, sh, sw): every frame at 1 / 2**shift resolution.  CUDA tensor: one hgi_decode_scaled_u8_dev
        call, asynchronous on the current stream; numpy stack: hgi_decode_scaled_u8 frame by frame.  `shift` and `out` are
        validated before any device call."""
        shift = _check_shift(shift, "decode_scaled_batch")
        if grids.ndim != 3:
            raise ValueError("expected a (batch, height, width) stack")
        b, height, width = (int(v) for v in grids.shape)
        sw, sh = scaled_size(width, height, shift)
        if not _is_torch(grids):
            g = np.ascontiguousarray(grids, dtype=np.uint8)
            out = np.empty((b, sh, sw), np.uint8) if out is None else _check_region_out(out, g, (b, sh, sw), "decode_scaled_batch")
            for f in range(b):
                out[f] = self.decode_scaled((width, height), levels, g[f], shift)
            return out
        import torch
        if out is not None:
            _check_region_out(out, grids, (b, sh, sw), "decode_scaled_batch")
        ctx = _torch_ctx(grids, self._ctx)
        if out is None:
            out = torch.empty((b, sh, sw), dtype=torch.uint8, device=grids.device)
        if b == 0 or width == 0 or height == 0:
            return out
        _ffi.check(_ffi.lib().hgi_decode_scaled_u8_dev(ctx.handle, grids.data_ptr(), width, height, int(levels), self._interp,
                                                       shift, out.data_ptr(), sw, b, height * width, sh * sw))
        return out

    def decode_list(self, grids, levels, out=None):
        """A list of (h_i, w_i) uint8 grids of any shapes, all coded with `levels` -> the list of their images.  CUDA tensors:
        ONE hgi_decode_u8_list_dev call, asynchronous on the current stream (outputs as in Encoder.encode_list); numpy arrays:
        hgi_decode_u8 frame by frame.  The list and `out` are validated before any device call."""
        frames, use_torch = _check_list(grids, out, "decode_list")
        if not use_torch:
            outs = [np.empty_like(f) for f in frames] if out is None else list(out)
            ctx = self._ctx or _ffi.default_context(0) if any(f.size for f in frames) else None
            for f, o in zip(frames, outs):
                if f.size:
                    _ffi.check(_ffi.lib().hgi_decode_u8(ctx.handle, f.ctypes.data, f.shape[1], f.shape[0], int(levels),
                                                        self._interp, o.ctypes.data))
            return outs
        ctx = _torch_ctx(frames[0], self._ctx)
        outs = _list_out(frames) if out is None else list(out)
        ins, ws, hs, ptrs = _list_arrays(frames, outs)
        _ffi.check(_ffi.lib().hgi_decode_u8_list_dev(ctx.handle, ins, ws, hs, int(levels), self._interp, ptrs, len(frames)))
        return outs

    def decode_views(self, plan, levels):
        """Decode a VIEW LIST: `plan` is a `rustyhgi_amd.views.ViewPlan` of (grid view, image view) pairs, all coded with
        `levels` (see Encoder.encode_views).  ONE hgi_views_decode_dev launch; what it does not serve is composed from one
        hgi_decode_u8_pitched_dev call per view.  Returns the destination views."""
        from . import _ffi_views
        levels, interp = int(levels), self._interp
        return _views_launch(
            plan, self._ctx,
            lambda stream, blob, info: _ffi_views.lib().hgi_views_decode_dev(stream, blob, info, levels, interp),
            lambda ctx, v: _ffi.lib().hgi_decode_u8_pitched_dev(ctx.handle, v[0], v[4], v[2], v[3], levels, interp, v[1], v[5], 1, 0, 0))

    def decode_scaled_views(self, plan, levels):
        """Decode a SCALED VIEW LIST: `plan` is a `rustyhgi_amd.sviews.ScaledViewPlan` of (grid view, image view) pairs, all
        coded with `levels`; every image view becomes `decode(grid view, levels)[::2**shift, ::2**shift]`, bit for bit, shift
        being the plan's.  ONE hgi_sviews_decode_dev launch (libhgi_sviews.so), asynchronous on the current stream; a plan or a
        depth that launch does not serve (HGI_EUNSUPPORTED: shift 0, levels <= shift, nine and more levels left above the
        lattice, an entry beyond the 32-bit buffer path) is composed from one hgi_decode_scaled_u8_dev call per view, into the
        destination's pitch, from the grid view itself when its rows are packed and from a packed copy otherwise: the same
        bytes.  Empty plans need no device.  Returns the destination views."""
        if len(plan) == 0 or plan.device is None:
            return list(plan.dsts)
        import torch
        from . import _ffi_sviews
        levels = int(levels)
        dev = plan.device.index if plan.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Decoder's context alike (_bind_ctx)
            raise ValueError("the views live on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        st = _ffi.EUNSUPPORTED
        if plan.fused:
            if plan.blob is None:      # only empty views
                return list(plan.dsts)
            with torch.cuda.device(dev):
                st = _ffi_sviews.lib().hgi_sviews_decode_dev(_ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), plan.blob.data_ptr(),
                                                             ctypes.addressof(plan.info), levels, self._interp)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bytes from one scaled decode per view
            bound = _bind_ctx(plan.srcs[0], self._ctx)
            for s, (_, dst, w, h, sp, dp) in zip(plan.srcs, plan.layouts):
                if w and h:
                    g = s if h == 1 or sp == w else s.contiguous()
                    _ffi.check(_ffi.lib().hgi_decode_scaled_u8_dev(bound.handle, g.data_ptr(), w, h, levels, self._interp, plan.shift,
                                                                   dst, dp, 1, 0, 0))
            return list(plan.dsts)
        _ffi_sviews.check(st)
        return list(plan.dsts)

    def decode_mapped(self, grids, levels, table, out=None):
        """Decode a view of grids straight into frames of the `table`'s dtype: `out[..., y, x] = table[decoded[..., y, x]]`,
        `decoded` being `decode_view(grids, levels)` -- float16 / bfloat16 / float32 frames, normalised however the table says
        (`rustyhgi_amd.affine_table`), without the uint8 image ever reaching memory.  `grids` is a view as for `decode_view`;
        `table` holds 256 elements of a 2- or 4-byte dtype: a 1-D contiguous torch CUDA tensor on the grids' device, or a numpy
        array (a dtype numpy lacks, such as bfloat16, needs a tensor).  A numpy table is uploaded on every call: the hot path
        keeps the table on the device and passes that tensor.  The result has the table's dtype and the grids' shape; `out` may
        be a view of that dtype (last stride 1 element, any row stride >= W elements) of which only the W-element rows are
        written.  The library copies the table's bits and does no arithmetic (NaN patterns and signed zeros come through).
        CUDA tensors: ONE hgi_map_decode_dev launch (libhgi_map.so), asynchronous on the current stream -- 1 + E B/px instead of
        the 3 + E B/px of a decode and a conversion.  What that launch does not serve (HGI_EUNSUPPORTED: 0 or more than 8
        levels, offsets beyond 32 bits, a width that is no multiple of 4 with the grids' last bytes at the end of a 4-KiB page)
        is composed from `decode_view` into a temporary and a gather on the same stream: the same bits, not fused.  numpy grids
        are uploaded and downloaded through torch tensors, synchronously; without a GPU that raises HgiError(EDEVICE).
        Validated (ValueError) before any device call; empty inputs need no device."""
        what = "decode_mapped"
        lay = _view_layout(grids, what)
        dtype, esize, tspan = _map_table(table, grids, what)
        (src, b, h, w, sp, sfs, gspan) = lay
        if out is None:
            _view_device(grids, what)
            if _is_torch(grids):
                import torch
                out = torch.empty(tuple(grids.shape), dtype=dtype, device=grids.device)
            else:
                out = np.empty(grids.shape, dtype)
            olay = _typed_view_layout(out, what, dtype, esize)
        else:
            if _is_torch(grids) != _is_torch(out):
                raise ValueError("%s: `out` must be a %s like the grids" % (what, "torch tensor" if _is_torch(grids) else "numpy array"))
            olay = _typed_view_layout(out, "%s (out)" % what, dtype, esize)
            if tuple(out.shape) != tuple(grids.shape):
                raise ValueError("%s: `out` has shape %s, the grids %s" % (what, tuple(out.shape), tuple(grids.shape)))
            if _is_torch(grids):
                if out.device != grids.device:
                    raise ValueError("%s: `out` lives on %s, the grids on %s" % (what, out.device, grids.device))
            elif not out.flags["WRITEABLE"]:
                raise ValueError("%s: `out` is not writable" % what)
        (dst, _, _, _, dp, dfs, ospan) = olay
        if b * h * w:
            g_lo, g_hi = src, src + (b - 1) * sfs + gspan
            o_lo, o_hi = dst, dst + (b - 1) * dfs + ospan
            if g_lo < o_hi and o_lo < g_hi:
                raise ValueError("%s: `out` shares memory with the grids (byte spans, tested conservatively)" % what)
            if tspan is not None and tspan[0] < o_hi and o_lo < tspan[1]:
                raise ValueError("%s: `out` shares memory with `table`" % what)
            if tspan is not None and tspan[0] < g_hi and g_lo < tspan[1]:
                raise ValueError("%s: `table` shares memory with the grids" % what)
        _view_device(grids, what)
        if b * h * w == 0:
            return out
        import torch
        bits = {2: (np.int16, torch.int16), 4: (np.int32, torch.int32)}[esize]      # elements travel as their bit patterns
        if not _is_torch(grids):
            if not torch.cuda.is_available():
                raise _ffi.HgiError(_ffi.EDEVICE, "%s needs a GPU (there is no CPU fallback)" % what)
            dev = "cuda:%d" % (self._ctx.device if self._ctx is not None else 0)
            g = torch.from_numpy(np.ascontiguousarray(grids)).to(dev)
            t = torch.from_numpy(table.view(bits[0])).to(dev)
            out.view(bits[0])[...] = self.decode_mapped(g, levels, t).cpu().numpy().reshape(out.shape)
            return out
        from . import _ffi_map
        dev = grids.device.index if grids.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Decoder's context alike (_bind_ctx)
            raise ValueError("tensor lives on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        if not _is_torch(table):
            table = torch.from_numpy(table).to(grids.device)
        with torch.cuda.device(dev):
            st = _ffi_map.lib().hgi_map_decode_dev(
                _ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), src, sp, w, h, int(levels), self._interp,
                table.data_ptr(), esize, dst, dp, b, sfs, dfs)
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bits from a decode and a gather
            tmp = self.decode_view(grids, levels)
            out.view(bits[1]).copy_(table.view(bits[1])[tmp.long()])
            return out
        _ffi_map.check(st)
        return out

    def decode_mapped_views(self, plan, levels, table):
        """Decode a MAPPED VIEW LIST: `plan` is a `rustyhgi_amd.mviews.MappedViewPlan` of (grid view, frame view) pairs, all
        coded with `levels`; every frame view becomes `table[decoded grid view]`, as `decode_mapped` writes it.  `table` is as
        for `decode_mapped`, of the plan's dtype.  ONE hgi_mviews_decode_dev launch (libhgi_mviews.so), asynchronous on the
        current stream; a plan or a depth that launch does not serve (HGI_EUNSUPPORTED) is composed from one `decode_mapped`
        call per view: the same bits.  Returns the destination views."""
        what = "decode_mapped_views"
        if len(plan) == 0 or plan.device is None:
            return list(plan.dsts)
        import torch
        from . import _ffi_mviews
        dtype, esize, _ = _map_table(table, plan.srcs[0], what)
        if dtype != plan.dtype:
            raise ValueError("%s: `table` holds %s elements, the plan was made for %s" % (what, dtype, plan.dtype))
        dev = plan.device.index if plan.device.index is not None else torch.cuda.current_device()
        if self._ctx is not None and self._ctx.device != dev:      # both routes judge the Decoder's context alike (_bind_ctx)
            raise ValueError("the views live on cuda:%d but the context was created for cuda:%d" % (dev, self._ctx.device))
        if not _is_torch(table):
            table = torch.from_numpy(table).to(plan.device)
        levels = int(levels)
        st = _ffi.EUNSUPPORTED
        if plan.fused:
            if plan.blob is None:      # only empty views
                return list(plan.dsts)
            with torch.cuda.device(dev):
                st = _ffi_mviews.lib().hgi_mviews_decode_dev(_ffi._vp(torch.cuda.current_stream(dev).cuda_stream or 0), plan.blob.data_ptr(),
                                                             ctypes.addressof(plan.info), levels, self._interp, table.data_ptr())
        if st == _ffi.EUNSUPPORTED:      # not served by the one launch: the same bits from one mapped decode per view
            for s, d in zip(plan.srcs, plan.dsts):
                if s.numel():
                    self.decode_mapped(s, levels, table, out=d)
            return list(plan.dsts)
        _ffi_mviews.check(st)
        return list(plan.dsts)
