"""ctypes binding of libhgi_qviews.so -- the C ABI declared in include/hgi_qviews.h (requantize view lists).  The plan, its blob
and its info structure are the view lists' (_ffi_views: ViewPair, ViewsInfo, hgi_views_plan).  Path, loading and errors:
_ffi_companion."""
from ._ffi_companion import Companion, vp, u32, i32, c_char_p

# every symbol include/hgi_qviews.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_qviews_requant_dev", i32, [vp, vp, vp, u32, i32, vp]),
    ("hgi_qviews_last_error", c_char_p, []),
    ("hgi_qviews_version", c_char_p, []),
]

_c = Companion("qviews", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
