"""ctypes binding of the C ABI declared in include/ccnet_eval.h (the sliding-window evaluation library).

The product loads ``ccnet_amd/csrc_eval/libccnet_eval.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside the other five (one scaffold, six libraries; :mod:`ccnet_amd._clib` holds what the bindings
share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_longlong, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_eval")
LIB_PATH = os.path.join(CSRC, "libccnet_eval.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_eval.h")

CCNET_EVAL_VERSION = 100       # include/ccnet_eval.h
MAX_TILES = 64                 # CCNET_EVAL_MAX_TILES
MAX_CLASSES = 256              # CCNET_EVAL_MAX_CLASSES

_P = c_void_p  # every tensor argument is a raw device pointer (tile_y1x1: a host int array)

# name -> (restype, argtypes); mirrors include/ccnet_eval.h one to one
_PROTOTYPES = {
    "ccnet_eval_version": (c_int, []),
    "ccnet_eval_arch": (c_char_p, []),
    "ccnet_eval_last_error_string": (c_char_p, []),
    "ccnet_eval_sliding_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P,
                                       c_longlong, _P, _P, _P, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_eval.h declares."""
    return _clib.declared_symbols(header)


def origins_array(origins):
    """[(y1, x1), ...] -> the host int array tile_y1x1 of the C ABI (kept alive by the caller for the call)."""
    flat = [int(v) for yx in origins for v in yx]
    return (c_int * max(len(flat), 1))(*flat)


class EvalError(RuntimeError):
    pass


class EvalLibrary(_clib.CLibrary):
    """A loaded libccnet_eval.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_eval", EvalError
    KERNELS = "evaluation kernel"


_lib: Optional[EvalLibrary] = None


def get_lib() -> EvalLibrary:
    """The process-wide device library; raises EvalError when it has not been built."""
    return EvalLibrary.shared()
