"""The loader the ctypes bindings of the companion libraries share (_ffi_recon, _ffi_map, _ffi_typed, _ffi_requant).

Each companion is a library of its own beside libhgi_hip.so, with a symbol table and a path of its own;
HGI_<NAME>_LIB_PATH overrides the path (in Python only: the libraries read no environment variable).  There is no fallback: a
missing library raises.
"""
import ctypes
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))

vp, u32, i32, sz, f32, c_char_p = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_char_p


class Companion:
    """libhgi_<name>.so: `symbols` is every symbol include/hgi_<name>.h declares, as (name, restype, argtypes)."""

    def __init__(self, name, symbols):
        self.name, self.symbols, self._lib = name, symbols, None
        self.path = os.environ.get("HGI_%s_LIB_PATH" % name.upper()) or os.path.join(_HERE, "libhgi_%s.so" % name)

    def lib(self):
        """Load the library (built in-tree by __graft_entry__.build() / <name>/Makefile)."""
        if self._lib is None:
            if not os.path.exists(self.path):
                raise ImportError("%s is missing: build it with `make -C rustyhgi_amd/%s` (there is no CPU fallback)" % (self.path, self.name))
            _ffi._share_torch_hip_runtime()      # one HIP runtime per process (see _ffi)
            L = ctypes.CDLL(self.path)
            for name, res, args in self.symbols:
                fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
                fn.restype, fn.argtypes = res, args
            self._lib = L
        return self._lib

    def last_error(self):
        return getattr(self.lib(), "hgi_%s_last_error" % self.name)().decode("utf-8", "replace")

    def check(self, status):
        if status != _ffi.OK:
            raise _ffi.HgiError(status, self.last_error())
