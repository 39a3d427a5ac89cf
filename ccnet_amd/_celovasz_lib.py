"""ctypes binding of the C ABI declared in include/ccnet_celovasz.h (the CE + Lovász criterion on logits up-sampled in-kernel).

The product loads ``ccnet_amd/csrc_lovasz/libccnet_celovasz.so`` (built for gfx950 by ``__graft_entry__.build()``): the second
translation unit in the Lovász library's directory, a library of its own beside ``libccnet_lovasz.so`` (:mod:`ccnet_amd._clib` holds what the
bindings share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_lovasz")
LIB_PATH = os.path.join(CSRC, "libccnet_celovasz.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_celovasz.h")

CCNET_CELOVASZ_VERSION = 100   # include/ccnet_celovasz.h
MIN_CLASSES, MAX_CLASSES = 2, 256

_P = c_void_p  # every tensor argument is a raw device pointer; class_weights is a host array

# name -> (restype, argtypes); mirrors include/ccnet_celovasz.h one to one
_PROTOTYPES = {
    "ccnet_celovasz_version": (c_int, []),
    "ccnet_celovasz_arch": (c_char_p, []),
    "ccnet_celovasz_last_error": (c_char_p, []),
    "ccnet_celovasz_workspace_bytes": (c_size_t, [c_int] * 7),
    "ccnet_celovasz_forward_f32": (c_int, [_P, _P, c_longlong, c_int, c_int, _P, _P, _P, _P, _P, c_size_t] + [c_int] * 6 + [_P]),
    "ccnet_celovasz_backward_f32": (c_int, [_P, _P, _P, _P, c_size_t] + [c_int] * 7 + [_P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_celovasz.h declares."""
    return _clib.declared_symbols(header)


class CeLovaszError(RuntimeError):
    pass


class CeLovaszLibrary(_clib.CLibrary):
    """A loaded libccnet_celovasz.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_celovasz", CeLovaszError
    KERNELS = "CE + Lovász criterion kernels"
    LAST_ERROR = "ccnet_celovasz_last_error"


_lib: Optional[CeLovaszLibrary] = None


def get_lib() -> CeLovaszLibrary:
    """The process-wide device library; raises CeLovaszError when it has not been built."""
    return CeLovaszLibrary.shared()
