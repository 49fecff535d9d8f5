"""ctypes binding of libhgi_typed.so -- the C ABI declared in include/hgi_typed.h (typed encode).

A library of its own beside libhgi_hip.so, with a table and a path of its own; HGI_TYPED_LIB_PATH overrides the path (in
Python only: the library reads no environment variable).  There is no fallback: a missing library raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HGI_TYPED_LIB_PATH") or os.path.join(_HERE, "libhgi_typed.so")

_vp, _u32, _int, _sz, _f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
# every symbol include/hgi_typed.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_typed_encode_dev", _int, [_vp, _vp, _sz, _u32, _u32, _f32, _f32, _u32, _u32, _u32, _int, _vp, _vp, _sz, _sz, _sz, _sz]),
    ("hgi_typed_last_error", ctypes.c_char_p, []),
    ("hgi_typed_version", ctypes.c_char_p, []),
]

_lib = None


def lib():
    """Load libhgi_typed.so (built in-tree by __graft_entry__.build() / typed/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `make -C rustyhgi_amd/typed` (there is no CPU fallback)" % LIB_PATH)
        _ffi._share_torch_hip_runtime()      # one HIP runtime per process (see _ffi)
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def last_error():
    return lib().hgi_typed_last_error().decode("utf-8", "replace")


def check(status):
    if status != _ffi.OK:
        raise _ffi.HgiError(status, last_error())
