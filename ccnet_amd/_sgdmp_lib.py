"""ctypes binding of the C ABI declared in include/ccnet_sgdmp.h (the mixed-precision optimiser step: momentum SGD with weight
decay over a parameter list of float32 tensors and bf16 tensors with float32 masters, in one launch, gradients zeroed in the
same pass, the learning rate from a device-side schedule).

The product loads ``ccnet_amd/csrc_sgdmp/libccnet_sgdmp.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of
its own beside the others (:mod:`ccnet_amd._clib` holds what the bindings share).  As with
:mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import POINTER, c_char_p, c_int, c_int64, c_void_p
from typing import List, Optional

import numpy as np

from . import _clib
from ._sgd_lib import CHUNK, DEFAULT_CAP, MAX_GROUPS, MAX_TENSORS  # noqa: F401  (include/ccnet_sgdmp.h takes them from ccnet_sgd.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_sgdmp")
LIB_PATH = os.path.join(CSRC, "libccnet_sgdmp.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_sgdmp.h")

CCNET_SGDMP_VERSION = 100      # include/ccnet_sgdmp.h
TENSOR_WORDS = 6               # CCNET_SGDMP_TENSOR_WORDS
(P, G, B, NUMEL, GROUP, M) = range(6)                          # CCNET_SGDMP_<field>

_P = c_void_p  # every table and tensor argument is a raw pointer

# name -> (restype, argtypes); mirrors include/ccnet_sgdmp.h one to one
_PROTOTYPES = {
    "ccnet_sgdmp_version": (c_int, []),
    "ccnet_sgdmp_arch": (c_char_p, []),
    "ccnet_sgdmp_last_error_string": (c_char_p, []),
    "ccnet_sgdmp_plan": (c_int, [_P, c_int, _P, c_int64, POINTER(c_int64)]),
    "ccnet_sgdmp_step": (c_int, [_P, _P, c_int, _P, _P, c_int64, _P, _P, _P, c_int, _P, c_int, _P, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_sgdmp.h declares."""
    return _clib.declared_symbols(header)


class SgdmpError(RuntimeError):
    pass


class SgdmpLibrary(_clib.CLibrary):
    """A loaded libccnet_sgdmp.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_sgdmp", SgdmpError
    KERNELS = "mixed-precision optimiser kernels"

    def plan(self, numels) -> np.ndarray:
        """The chunk table of tensors with these element counts, int32 (n_chunks, 2), by the library's own arithmetic."""
        numel = np.ascontiguousarray(numels, np.int64)
        n = c_int64(0)
        self.check(self.ccnet_sgdmp_plan(numel.ctypes.data, numel.size, None, 0, n), "ccnet_sgdmp_plan")
        chunks = np.empty((n.value, 2), np.int32)
        self.check(self.ccnet_sgdmp_plan(numel.ctypes.data, numel.size, chunks.ctypes.data, n.value, n), "ccnet_sgdmp_plan")
        return chunks


_lib: Optional[SgdmpLibrary] = None


def get_lib() -> SgdmpLibrary:
    """The process-wide device library; raises SgdmpError when it has not been built."""
    return SgdmpLibrary.shared()
