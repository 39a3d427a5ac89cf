"""ctypes binding of the C ABI declared in include/ccnet_abn.h (activated batch normalisation on the device).

The product loads ``ccnet_amd/csrc_abn/libccnet_abn.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of its
own beside the other five (one scaffold, six libraries; :mod:`ccnet_amd._clib` holds what the bindings share).
As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_abn")
LIB_PATH = os.path.join(CSRC, "libccnet_abn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_abn.h")

CCNET_ABN_VERSION = 100     # include/ccnet_abn.h
CCNET_ABN_F32, CCNET_ABN_BF16 = 0, 1
CCNET_ABN_IDENTITY, CCNET_ABN_RELU, CCNET_ABN_LEAKY_RELU, CCNET_ABN_ELU = 0, 1, 2, 3
CCNET_ABN_GAMMA_WEIGHT, CCNET_ABN_GAMMA_ABS_EPS = 0, 1
CCNET_ABN_FROM_INPUT, CCNET_ABN_FROM_OUTPUT = 0, 1


class AbnDesc(Structure):
    """``ccnet_abn_desc``"""
    _fields_ = [("dtype", c_int), ("N", c_int), ("C", c_int), ("H", c_int), ("W", c_int), ("activation", c_int),
                ("act_param", c_float), ("gamma_mode", c_int), ("eps", c_float)]


_P = c_void_p  # every tensor argument is a raw device pointer
_D = POINTER(AbnDesc)

# name -> (restype, argtypes); mirrors include/ccnet_abn.h one to one
_PROTOTYPES = {
    "ccnet_abn_version": (c_int, []),
    "ccnet_abn_arch": (c_char_p, []),
    "ccnet_abn_last_error_string": (c_char_p, []),
    "ccnet_abn_workspace_bytes": (c_size_t, [_D]),
    "ccnet_abn_stats": (c_int, [_D, _P, _P, _P, c_size_t, _P]),
    "ccnet_abn_stats_combine": (c_int, [_D, _P, c_int, c_float, _P, _P, _P, _P]),
    "ccnet_abn_forward": (c_int, [_D, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ccnet_abn_backward_reduce": (c_int, [_D, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "ccnet_abn_backward_apply": (c_int, [_D, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
}

ACTIVATIONS = {"identity": CCNET_ABN_IDENTITY, "none": CCNET_ABN_IDENTITY, "relu": CCNET_ABN_RELU,
               "leaky_relu": CCNET_ABN_LEAKY_RELU, "elu": CCNET_ABN_ELU}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_abn.h declares."""
    return _clib.declared_symbols(header)


def make_desc(dtype: int, N: int, C: int, H: int, W: int, activation: int, act_param: float, gamma_mode: int,
              eps: float) -> AbnDesc:
    return AbnDesc(dtype, N, C, H, W, activation, act_param, gamma_mode, eps)


class AbnError(RuntimeError):
    pass


class AbnLibrary(_clib.CLibrary):
    """A loaded libccnet_abn.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_abn", AbnError
    KERNELS = "ABN kernels"


_lib: Optional[AbnLibrary] = None


def get_lib() -> AbnLibrary:
    """The process-wide device library; raises AbnError when it has not been built."""
    return AbnLibrary.shared()
