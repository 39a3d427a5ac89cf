"""ctypes binding of the C ABI declared in include/ccnet_mseval.h (the multi-scale evaluation library).

The product loads ``ccnet_amd/csrc_eval/libccnet_mseval.so`` (built for gfx950 by ``__graft_entry__.build()``): the second
translation unit of the evaluation row, a library of its own beside ``libccnet_eval.so`` (:mod:`ccnet_amd._clib` holds what
the bindings share).  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_longlong, c_void_p
from typing import List, Optional

from . import _clib
from ._eval_lib import origins_array  # noqa: F401  (tile_y1x1 is the same host int array)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_eval")
LIB_PATH = os.path.join(CSRC, "libccnet_mseval.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_mseval.h")

CCNET_MSEVAL_VERSION = 100     # include/ccnet_mseval.h
MAX_TILES = 64                 # CCNET_MSEVAL_MAX_TILES
MAX_CLASSES = 256              # CCNET_MSEVAL_MAX_CLASSES

_P = c_void_p  # every tensor argument is a raw device pointer (tile_y1x1: a host int array)

# name -> (restype, argtypes); mirrors include/ccnet_mseval.h one to one
_PROTOTYPES = {
    "ccnet_mseval_version": (c_int, []),
    "ccnet_mseval_arch": (c_char_p, []),
    "ccnet_mseval_last_error_string": (c_char_p, []),
    "ccnet_mseval_tiles_f32": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int,
                                       c_int, _P, _P]),
    "ccnet_mseval_accumulate_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_int, _P, _P, c_int, _P, c_longlong, _P, _P, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_mseval.h declares."""
    return _clib.declared_symbols(header)


class MsEvalError(RuntimeError):
    pass


class MsEvalLibrary(_clib.CLibrary):
    """A loaded libccnet_mseval.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_mseval", MsEvalError
    KERNELS = "multi-scale evaluation kernels"


_lib: Optional[MsEvalLibrary] = None


def get_lib() -> MsEvalLibrary:
    """The process-wide device library; raises MsEvalError when it has not been built."""
    return MsEvalLibrary.shared()
