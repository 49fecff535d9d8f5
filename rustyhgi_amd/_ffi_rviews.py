"""ctypes binding of libhgi_rviews.so -- the C ABI declared in include/hgi_rviews.h (recon view lists).  Path, loading and
errors: _ffi_companion."""
import ctypes

from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

u64 = ctypes.c_uint64
MAGIC = 0x56524731


class RViewTriple(ctypes.Structure):
    """hgi_rview_triple"""
    _fields_ = [("src", u64), ("grid", u64), ("recon", u64), ("width", u32), ("height", u32), ("src_pitch", u64), ("grid_pitch", u64),
                ("recon_pitch", u64)]


class RViewsInfo(ctypes.Structure):
    """hgi_rviews_info"""
    _fields_ = [("magic", u32), ("count", u32), ("edge_tiles", u32), ("interior_tiles", u32), ("max_width", u32), ("reserved", u32),
                ("plan_bytes", u64), ("records_offset", u64), ("edge_prefix_offset", u64), ("interior_prefix_offset", u64),
                ("recon_offset", u64)]


# every symbol include/hgi_rviews.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_rviews_plan_bytes", sz, [sz]),
    ("hgi_rviews_plan", i32, [vp, sz, vp, sz, vp]),
    ("hgi_rviews_encode_dev", i32, [vp, vp, vp, u32, i32, vp]),
    ("hgi_rviews_last_error", c_char_p, []),
    ("hgi_rviews_version", c_char_p, []),
]

_c = Companion("rviews", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
