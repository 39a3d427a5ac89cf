"""ctypes binding of the C ABI declared in include/ccnet_sgd.h (the optimiser step: momentum SGD with weight decay over a whole
parameter list in one launch, gradients zeroed in the same pass, the learning rate from a device-side schedule).

The product loads ``ccnet_amd/csrc_sgd/libccnet_sgd.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of its
own beside the others (:mod:`ccnet_amd._clib` holds what the bindings share).  As with :mod:`ccnet_amd._lib`
there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import POINTER, c_char_p, c_int, c_int64, c_void_p
from typing import List, Optional

import numpy as np

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_sgd")
LIB_PATH = os.path.join(CSRC, "libccnet_sgd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_sgd.h")

CCNET_SGD_VERSION = 100        # include/ccnet_sgd.h
CHUNK = 4096                   # CCNET_SGD_CHUNK
MAX_GROUPS = 8                 # CCNET_SGD_MAX_GROUPS
MAX_TENSORS = 65535            # CCNET_SGD_MAX_TENSORS
DEFAULT_CAP = 2048             # CCNET_SGD_DEFAULT_CAP
TENSOR_WORDS = 5               # CCNET_SGD_TENSOR_WORDS
(P, G, B, NUMEL, GROUP) = range(5)                             # CCNET_SGD_<field>

_P = c_void_p  # every table and tensor argument is a raw pointer

# name -> (restype, argtypes); mirrors include/ccnet_sgd.h one to one
_PROTOTYPES = {
    "ccnet_sgd_version": (c_int, []),
    "ccnet_sgd_arch": (c_char_p, []),
    "ccnet_sgd_last_error_string": (c_char_p, []),
    "ccnet_sgd_plan": (c_int, [_P, c_int, _P, c_int64, POINTER(c_int64)]),
    "ccnet_sgd_step": (c_int, [_P, _P, c_int, _P, _P, c_int64, _P, _P, _P, c_int, _P, c_int, _P, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_sgd.h declares."""
    return _clib.declared_symbols(header)


class SgdError(RuntimeError):
    pass


class SgdLibrary(_clib.CLibrary):
    """A loaded libccnet_sgd.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_sgd", SgdError
    KERNELS = "optimiser kernels"

    def plan(self, numels) -> np.ndarray:
        """The chunk table of tensors with these element counts, int32 (n_chunks, 2), by the library's own arithmetic."""
        numel = np.ascontiguousarray(numels, np.int64)
        n = c_int64(0)
        self.check(self.ccnet_sgd_plan(numel.ctypes.data, numel.size, None, 0, n), "ccnet_sgd_plan")
        chunks = np.empty((n.value, 2), np.int32)
        self.check(self.ccnet_sgd_plan(numel.ctypes.data, numel.size, chunks.ctypes.data, n.value, n), "ccnet_sgd_plan")
        return chunks


_lib: Optional[SgdLibrary] = None


def get_lib() -> SgdLibrary:
    """The process-wide device library; raises SgdError when it has not been built."""
    return SgdLibrary.shared()
