"""ctypes binding of libhgi_tviews.so -- the C ABI declared in include/hgi_tviews.h (typed view lists).  Path, loading and
errors: _ffi_companion."""
import ctypes

from ._ffi_companion import Companion, vp, u32, i32, sz, f32, c_char_p

u64 = ctypes.c_uint64
MAGIC = 0x56544731


class TViewPair(ctypes.Structure):
    """hgi_tview_pair"""
    _fields_ = [("src", u64), ("dst", u64), ("width", u32), ("height", u32), ("src_pitch", u64), ("dst_pitch", u64)]


class TViewsInfo(ctypes.Structure):
    """hgi_tviews_info"""
    _fields_ = [("magic", u32), ("count", u32), ("edge_tiles", u32), ("interior_tiles", u32), ("max_width", u32), ("elem_size", u32),
                ("plan_bytes", u64), ("records_offset", u64), ("edge_prefix_offset", u64), ("interior_prefix_offset", u64)]


# every symbol include/hgi_tviews.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_tviews_plan_bytes", sz, [sz]),
    ("hgi_tviews_plan", i32, [vp, sz, u32, vp, sz, vp]),
    ("hgi_tviews_encode_dev", i32, [vp, vp, vp, u32, f32, f32, u32, i32, vp]),
    ("hgi_tviews_last_error", c_char_p, []),
    ("hgi_tviews_version", c_char_p, []),
]

_c = Companion("tviews", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
