"""ctypes binding of libhgi_map.so -- the C ABI declared in include/hgi_map.h (mapped decode).  Path, loading and errors:
_ffi_companion."""
from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

# every symbol include/hgi_map.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_map_decode_dev", i32, [vp, vp, sz, u32, u32, u32, i32, vp, u32, vp, sz, sz, sz, sz]),
    ("hgi_map_last_error", c_char_p, []),
    ("hgi_map_version", c_char_p, []),
]

_c = Companion("map", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
