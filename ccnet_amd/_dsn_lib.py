"""ctypes binding of the C ABI declared in include/ccnet_dsn.h (the DSN cross-entropy on logits up-sampled in-kernel).

The product loads ``ccnet_amd/csrc_dsn/libccnet_dsn.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside the other six (one scaffold, seven libraries; :mod:`ccnet_amd._clib` holds what the bindings
share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_dsn")
LIB_PATH = os.path.join(CSRC, "libccnet_dsn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_dsn.h")

CCNET_DSN_VERSION = 100        # include/ccnet_dsn.h
MAX_CLASSES = 256              # the bound of CCNET_EVAL_MAX_CLASSES

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_dsn.h one to one
_PROTOTYPES = {
    "ccnet_dsn_version": (c_int, []),
    "ccnet_dsn_arch": (c_char_p, []),
    "ccnet_dsn_last_error_string": (c_char_p, []),
    "ccnet_dsn_workspace_bytes": (c_size_t, [c_int] * 7),
    "ccnet_dsn_forward_f32": (c_int, [_P, _P, _P, c_float, c_float, _P, _P, _P, _P, c_size_t] + [c_int] * 7
                              + [c_longlong, _P]),
    "ccnet_dsn_backward_f32": (c_int, [_P, _P, _P, _P, _P, c_float, c_float, _P, c_size_t] + [c_int] * 7 + [_P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_dsn.h declares."""
    return _clib.declared_symbols(header)


class DsnError(RuntimeError):
    pass


class DsnLibrary(_clib.CLibrary):
    """A loaded libccnet_dsn.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_dsn", DsnError
    KERNELS = "DSN cross-entropy kernels"


_lib: Optional[DsnLibrary] = None


def get_lib() -> DsnLibrary:
    """The process-wide device library; raises DsnError when it has not been built."""
    return DsnLibrary.shared()
