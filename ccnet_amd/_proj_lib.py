"""ctypes binding of the C ABI declared in include/ccnet_proj.h (the module's bf16 projections on the library's own MFMA GEMM).

The product loads ``ccnet_amd/csrc_proj/libccnet_proj.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of its
own beside the other five (one scaffold, six libraries; :mod:`ccnet_amd._clib` holds what the bindings share).
As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_long, c_size_t, c_void_p
from typing import List, Optional, Tuple

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_proj")
LIB_PATH = os.path.join(CSRC, "libccnet_proj.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_proj.h")

CCNET_PROJ_VERSION = 100    # include/ccnet_proj.h
CCNET_PROJ_E_BADSHAPE, CCNET_PROJ_E_NULLPTR, CCNET_PROJ_E_BADFLAGS, CCNET_PROJ_E_WORKSPACE = -1, -2, -3, -4
CCNET_PROJ_BF16, CCNET_PROJ_F32 = 0, 1
TILE_ROWS = 256             # rows of the GEMM's workgroup tile (csrc/cca_gemm.hpp PG_BM)
MAX_ELEMS = 1 << 30         # bf16 elements whose byte offsets stay below 2^31

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_proj.h one to one
_PROTOTYPES = {
    "ccnet_proj_version": (c_int, []),
    "ccnet_proj_arch": (c_char_p, []),
    "ccnet_proj_last_error": (c_char_p, []),
    "ccnet_proj_gemm_bf16": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_long, c_long, c_long, c_long, _P]),
    "ccnet_proj_pack": (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, c_int, c_int, _P]),
    "ccnet_proj_colsum_workspace_bytes": (c_size_t, [c_int, c_int]),
    "ccnet_proj_colsum_bf16": (c_int, [_P, _P, c_int, c_int, c_long, _P, c_size_t, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_proj.h declares."""
    return _clib.declared_symbols(header)


def gemm_contract_ok(N: int, K: int, lda: int, ldw: int, ldo: int, ldadd: Optional[int] = None) -> bool:
    """The shape half of ``ccnet_proj_gemm_bf16``'s contract (the row count is the planner's business)."""
    return (N > 0 and K > 0 and K % 8 == 0 and N % 4 == 0 and lda % 8 == 0 and ldw % 8 == 0 and ldo % 4 == 0
            and lda >= K and ldw >= K and ldo >= N and N * ldw < MAX_ELEMS
            and (ldadd is None or (ldadd % 4 == 0 and ldadd >= N)))


def plan_rows(M: int, lda: int, ldo: int, ldadd: int = 0) -> List[Tuple[int, int]]:
    """[(first row, rows)] of the launches that cover M rows: every launch but the last is a whole number of 256-row tiles, and
    rows * stride < 2^30 elements for each of the three row-strided operands (every byte offset of a launch below 2^31).  An
    empty list: not even one tile fits under the limit."""
    widest = max(lda, ldo, ldadd)
    if M <= 0 or widest <= 0:
        return []
    rows = (MAX_ELEMS - 1) // widest // TILE_ROWS * TILE_ROWS
    if rows <= 0:
        return []
    return [(m0, min(rows, M - m0)) for m0 in range(0, M, rows)]


class ProjError(RuntimeError):
    pass


class ProjLibrary(_clib.CLibrary):
    """A loaded libccnet_proj.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_proj", ProjError
    KERNELS = "projection kernels"
    LAST_ERROR = "ccnet_proj_last_error"


_lib: Optional[ProjLibrary] = None


def get_lib() -> ProjLibrary:
    """The process-wide device library; raises ProjError when it has not been built."""
    return ProjLibrary.shared()
