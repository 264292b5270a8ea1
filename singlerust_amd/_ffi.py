"""ctypes binding of libsrx_hip.so (include/srx.h, include/srx_synth.h).

This is plumbing: it loads the in-tree HIP library and applies the C ABI that ``_abi.py`` describes.  That module
is generated from the two headers (scripts/gen_ctypes_bindings.py); every constant, structure and signature of it
is re-exported here, so ``_ffi.Csr``, ``_ffi.E_HIP``, ``_ffi.EXPORTS`` ... are the names to use.  There is no
CPU fallback — if the library is missing, or no GPU is visible when a compute call is made,
the call raises (``SrxError``).
"""
from __future__ import annotations

import ctypes as C
import os

from ._abi import *  # noqa: F401,F403  (the constants without their SRX_ prefix, the structures in camel case)
from ._abi import E_HIP, EXPORTS, HOST_ALLREDUCE_FN, OK, SIGNATURES, STATUS_NAMES, P  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsrx_hip.so")


class SrxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code
        self.msg = msg


_lib = None


def lib() -> C.CDLL:
    """Load libsrx_hip.so (built in-tree by singlerust_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SrxError(E_HIP, f"{LIB_PATH} is missing: run `python -m singlerust_amd.build` "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, ctx=None) -> None:
    if rc != OK:
        msg = lib().srx_last_error(ctx)
        raise SrxError(rc, msg.decode() if msg else "")


def ptr(a):
    """void* of a numpy array (or None)."""
    return None if a is None else C.c_void_p(a.ctypes.data)
