"""ctypes binding of the C ABI declared in include/ccnet_ohemdsn.h (the OHEM + DSN criterion on logits up-sampled in-kernel).

The product loads ``ccnet_amd/csrc_ohem/libccnet_ohemdsn.so`` (built for gfx950 by ``__graft_entry__.build()``): the second
translation unit of the OHEM row, a library of its own beside ``libccnet_ohem.so`` (:mod:`ccnet_amd._clib` holds what the
bindings share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_ohem")
LIB_PATH = os.path.join(CSRC, "libccnet_ohemdsn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_ohemdsn.h")

CCNET_OHEMDSN_VERSION = 100    # include/ccnet_ohemdsn.h
MAX_CLASSES = 256              # the bound of ccnet_dsn.h

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_ohemdsn.h one to one
_PROTOTYPES = {
    "ccnet_ohemdsn_version": (c_int, []),
    "ccnet_ohemdsn_arch": (c_char_p, []),
    "ccnet_ohemdsn_last_error": (c_char_p, []),
    "ccnet_ohemdsn_workspace_bytes": (c_size_t, [c_int] * 8),
    "ccnet_ohemdsn_forward_f32": (c_int, [_P, _P, _P, c_longlong, c_float, c_int, c_int, _P, _P, _P, _P, _P, c_size_t]
                                  + [c_int] * 7 + [_P]),
    "ccnet_ohemdsn_backward_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_size_t] + [c_int] * 8 + [_P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_ohemdsn.h declares."""
    return _clib.declared_symbols(header)


class OhemDsnError(RuntimeError):
    pass


class OhemDsnLibrary(_clib.CLibrary):
    """A loaded libccnet_ohemdsn.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_ohemdsn", OhemDsnError
    KERNELS = "OHEM + DSN criterion kernels"
    LAST_ERROR = "ccnet_ohemdsn_last_error"


_lib: Optional[OhemDsnLibrary] = None


def get_lib() -> OhemDsnLibrary:
    """The process-wide device library; raises OhemDsnError when it has not been built."""
    return OhemDsnLibrary.shared()
