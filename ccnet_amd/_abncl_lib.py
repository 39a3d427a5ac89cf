"""ctypes binding of the C ABI declared in include/ccnet_abncl.h (activated batch normalisation on pixel-major, that is dense
channels_last, tensors).

The product loads ``ccnet_amd/csrc_abncl/libccnet_abncl.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of
its own whose kernels include csrc_abn/'s arithmetic (:mod:`ccnet_amd._clib` holds what the bindings share).
As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_abncl")
LIB_PATH = os.path.join(CSRC, "libccnet_abncl.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_abncl.h")

CCNET_ABNCL_VERSION = 100     # include/ccnet_abncl.h
CCNET_ABNCL_F32, CCNET_ABNCL_BF16 = 0, 1
CCNET_ABNCL_IDENTITY, CCNET_ABNCL_RELU, CCNET_ABNCL_LEAKY_RELU, CCNET_ABNCL_ELU = 0, 1, 2, 3
CCNET_ABNCL_GAMMA_WEIGHT, CCNET_ABNCL_GAMMA_ABS_EPS = 0, 1
CCNET_ABNCL_FROM_INPUT, CCNET_ABNCL_FROM_OUTPUT = 0, 1


class AbnClDesc(Structure):
    """``ccnet_abncl_desc``"""
    _fields_ = [("dtype", c_int), ("M", c_longlong), ("C", c_int), ("activation", c_int), ("act_param", c_float),
                ("gamma_mode", c_int), ("eps", c_float)]


_P = c_void_p  # every tensor argument is a raw device pointer
_D = POINTER(AbnClDesc)

# name -> (restype, argtypes); mirrors include/ccnet_abncl.h one to one
_PROTOTYPES = {
    "ccnet_abncl_version": (c_int, []),
    "ccnet_abncl_arch": (c_char_p, []),
    "ccnet_abncl_last_error_string": (c_char_p, []),
    "ccnet_abncl_workspace_bytes": (c_size_t, [_D]),
    "ccnet_abncl_splits": (c_int, [_D]),
    "ccnet_abncl_stats": (c_int, [_D, _P, _P, _P, c_size_t, _P]),
    "ccnet_abncl_stats_combine": (c_int, [_D, _P, c_int, c_float, _P, _P, _P, _P]),
    "ccnet_abncl_forward": (c_int, [_D, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ccnet_abncl_backward_reduce": (c_int, [_D, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "ccnet_abncl_backward_apply": (c_int, [_D, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_abncl.h declares."""
    return _clib.declared_symbols(header)


def make_desc(dtype: int, M: int, C: int, activation: int, act_param: float, gamma_mode: int, eps: float) -> AbnClDesc:
    return AbnClDesc(dtype, M, C, activation, act_param, gamma_mode, eps)


class AbnClError(RuntimeError):
    pass


class AbnClLibrary(_clib.CLibrary):
    """A loaded libccnet_abncl.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_abncl", AbnClError
    KERNELS = "channels_last ABN kernels"


_lib: Optional[AbnClLibrary] = None


def get_lib() -> AbnClLibrary:
    """The process-wide device library; raises AbnClError when it has not been built."""
    return AbnClLibrary.shared()
