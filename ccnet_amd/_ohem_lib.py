"""ctypes binding of the C ABI declared in include/ccnet_ohem.h (the OHEM cross-entropy library).

The product loads ``ccnet_amd/csrc_ohem/libccnet_ohem.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside the other five (one scaffold, six libraries; :mod:`ccnet_amd._clib` holds what the bindings
share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_ohem")
LIB_PATH = os.path.join(CSRC, "libccnet_ohem.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_ohem.h")

CCNET_OHEM_VERSION = 100       # include/ccnet_ohem.h

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_ohem.h one to one
_PROTOTYPES = {
    "ccnet_ohem_version": (c_int, []),
    "ccnet_ohem_arch": (c_char_p, []),
    "ccnet_ohem_last_error_string": (c_char_p, []),
    "ccnet_ohem_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ccnet_ohem_forward_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int,
                                       c_longlong, c_float, c_int, c_int, _P]),
    "ccnet_ohem_backward_f32": (c_int, [_P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_ohem.h declares."""
    return _clib.declared_symbols(header)


class OhemError(RuntimeError):
    pass


class OhemLibrary(_clib.CLibrary):
    """A loaded libccnet_ohem.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_ohem", OhemError
    KERNELS = "OHEM cross-entropy kernels"


_lib: Optional[OhemLibrary] = None


def get_lib() -> OhemLibrary:
    """The process-wide device library; raises OhemError when it has not been built."""
    return OhemLibrary.shared()
