"""ctypes binding of libhgi_requant.so -- the C ABI declared in include/hgi_requant.h (requantize).

A library of its own beside libhgi_hip.so, with a table and a path of its own; HGI_REQUANT_LIB_PATH overrides the path (in
Python only: the library reads no environment variable).  There is no fallback: a missing library raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HGI_REQUANT_LIB_PATH") or os.path.join(_HERE, "libhgi_requant.so")

_vp, _u32, _int, _sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
# every symbol include/hgi_requant.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("hgi_requant_dev", _int, [_vp, _vp, _sz, _u32, _u32, _u32, _int, _vp, _vp, _sz, _sz, _sz, _sz]),
    ("hgi_requant_last_error", ctypes.c_char_p, []),
    ("hgi_requant_version", ctypes.c_char_p, []),
]

_lib = None


def lib():
    """Load libhgi_requant.so (built in-tree by __graft_entry__.build() / requant/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `make -C rustyhgi_amd/requant` (there is no CPU fallback)" % LIB_PATH)
        _ffi._share_torch_hip_runtime()      # one HIP runtime per process (see _ffi)
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def last_error():
    return lib().hgi_requant_last_error().decode("utf-8", "replace")


def check(status):
    if status != _ffi.OK:
        raise _ffi.HgiError(status, last_error())
