"""ctypes binding of libhgi_sviews.so -- the C ABI declared in include/hgi_sviews.h (scaled view lists).  Path, loading and
errors: _ffi_companion."""
import ctypes

from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

u64 = ctypes.c_uint64
MAGIC = 0x56534731


class SViewPair(ctypes.Structure):
    """hgi_sview_pair"""
    _fields_ = [("src", u64), ("dst", u64), ("width", u32), ("height", u32), ("src_pitch", u64), ("dst_pitch", u64)]


class SViewsInfo(ctypes.Structure):
    """hgi_sviews_info"""
    _fields_ = [("magic", u32), ("count", u32), ("edge_tiles", u32), ("interior_tiles", u32), ("max_width", u32), ("shift", u32),
                ("plan_bytes", u64), ("records_offset", u64), ("edge_prefix_offset", u64), ("interior_prefix_offset", u64)]


# every symbol include/hgi_sviews.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_sviews_plan_bytes", sz, [sz]),
    ("hgi_sviews_plan", i32, [vp, sz, u32, vp, sz, vp]),
    ("hgi_sviews_decode_dev", i32, [vp, vp, vp, u32, i32]),
    ("hgi_sviews_last_error", c_char_p, []),
    ("hgi_sviews_version", c_char_p, []),
]

_c = Companion("sviews", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
