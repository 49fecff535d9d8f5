"""ctypes binding of libhgi_requant.so -- the C ABI declared in include/hgi_requant.h (requantize).  Path, loading and errors:
_ffi_companion."""
from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

# every symbol include/hgi_requant.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_requant_dev", i32, [vp, vp, sz, u32, u32, u32, i32, vp, vp, sz, sz, sz, sz]),
    ("hgi_requant_last_error", c_char_p, []),
    ("hgi_requant_version", c_char_p, []),
]

_c = Companion("requant", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
