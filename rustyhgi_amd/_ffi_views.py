"""ctypes binding of libhgi_views.so -- the C ABI declared in include/hgi_views.h (view lists).  Path, loading and errors:
_ffi_companion."""
import ctypes

from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

u64 = ctypes.c_uint64
MAGIC = 0x56494731


class ViewPair(ctypes.Structure):
    """hgi_view_pair"""
    _fields_ = [("src", u64), ("dst", u64), ("width", u32), ("height", u32), ("src_pitch", u64), ("dst_pitch", u64)]


class ViewsInfo(ctypes.Structure):
    """hgi_views_info"""
    _fields_ = [("magic", u32), ("count", u32), ("edge_tiles", u32), ("interior_tiles", u32), ("max_width", u32), ("reserved", u32),
                ("plan_bytes", u64), ("records_offset", u64), ("edge_prefix_offset", u64), ("interior_prefix_offset", u64)]


# every symbol include/hgi_views.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_views_plan_bytes", sz, [sz]),
    ("hgi_views_plan", i32, [vp, sz, vp, sz, vp]),
    ("hgi_views_encode_dev", i32, [vp, vp, vp, u32, i32, vp]),
    ("hgi_views_decode_dev", i32, [vp, vp, vp, u32, i32]),
    ("hgi_views_last_error", c_char_p, []),
    ("hgi_views_version", c_char_p, []),
]

_c = Companion("views", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
