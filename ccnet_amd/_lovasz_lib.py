"""ctypes binding of the C ABI declared in include/ccnet_lovasz.h (the Lovász-softmax library).

The product loads ``ccnet_amd/csrc_lovasz/libccnet_lovasz.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside the other five (one scaffold, six libraries; :mod:`ccnet_amd._clib` holds what the bindings
share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_lovasz")
LIB_PATH = os.path.join(CSRC, "libccnet_lovasz.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_lovasz.h")

CCNET_LOVASZ_VERSION = 100     # include/ccnet_lovasz.h
MAX_CLASSES = 256

_P = c_void_p  # every tensor argument is a raw device pointer; class_weights is a host array

# name -> (restype, argtypes); mirrors include/ccnet_lovasz.h one to one
_PROTOTYPES = {
    "ccnet_lovasz_version": (c_int, []),
    "ccnet_lovasz_arch": (c_char_p, []),
    "ccnet_lovasz_last_error_string": (c_char_p, []),
    "ccnet_lovasz_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ccnet_lovasz_forward_f32": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_longlong, c_int,
                                         c_int, c_int, _P, _P]),
    "ccnet_lovasz_backward_f32": (c_int, [_P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_lovasz.h declares."""
    return _clib.declared_symbols(header)


class LovaszError(RuntimeError):
    pass


class LovaszLibrary(_clib.CLibrary):
    """A loaded libccnet_lovasz.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_lovasz", LovaszError
    KERNELS = "Lovász-softmax kernels"


def class_selection(classes, C: int):
    """The reference's ``classes`` argument as (present_only, class weights as a ctypes byte array or None).

    'present' and 'all' select every class ('present' drops the absent ones per segment); a list selects exactly its
    entries, a duplicate counting once more each time it repeats, as the reference's loop does."""
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f"lovasz_softmax: classes must be 'present', 'all' or a list of class ids, not {classes!r}")
        return classes == "present", None
    counts = [0] * C
    for c in classes:
        c = int(c)
        if not 0 <= c < C:
            raise ValueError(f"lovasz_softmax: class id {c} outside [0, {C})")
        counts[c] += 1
        if counts[c] > 255:
            raise ValueError(f"lovasz_softmax: class id {c} listed more than 255 times")
    return False, (ctypes.c_ubyte * C)(*counts)


_lib: Optional[LovaszLibrary] = None


def get_lib() -> LovaszLibrary:
    """The process-wide device library; raises LovaszError when it has not been built."""
    return LovaszLibrary.shared()
