"""ctypes binding of libhgi_typed.so -- the C ABI declared in include/hgi_typed.h (typed encode).  Path, loading and errors:
_ffi_companion."""
from ._ffi_companion import Companion, vp, u32, i32, sz, f32, c_char_p

# every symbol include/hgi_typed.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_typed_encode_dev", i32, [vp, vp, sz, u32, u32, f32, f32, u32, u32, u32, i32, vp, vp, sz, sz, sz, sz]),
    ("hgi_typed_last_error", c_char_p, []),
    ("hgi_typed_version", c_char_p, []),
]

_c = Companion("typed", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
