"""ctypes binding of libhgi_recon.so -- the C ABI declared in include/hgi_recon.h (encode with reconstruction).  Path, loading and errors:
_ffi_companion."""
from ._ffi_companion import Companion, vp, u32, i32, sz, c_char_p

# every symbol include/hgi_recon.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_recon_encode_u8_dev", i32, [vp, vp, sz, u32, u32, u32, i32, vp, vp, sz, vp, sz, sz, sz, sz, sz]),
    ("hgi_recon_last_error", c_char_p, []),
    ("hgi_recon_version", c_char_p, []),
]

_c = Companion("recon", SYMBOLS)
LIB_PATH, lib, last_error, check = _c.path, _c.lib, _c.last_error, _c.check
