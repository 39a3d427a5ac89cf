"""ctypes binding of the C ABI declared in include/ccnet_conv3.h (the 3x3 dilated convolution on bf16 channels_last activations as
an implicit GEMM on the library's own MFMA kernels).

The product loads ``ccnet_amd/csrc_conv3/libccnet_conv3.so`` (built for gfx950 by ``__graft_entry__.build()``), a library of its
own beside the others (:mod:`ccnet_amd._clib` holds what the bindings share).  As with :mod:`ccnet_amd._lib` there is no
fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import c_char_p, c_int, c_long, c_size_t, c_void_p
from typing import List, Optional, Tuple

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_conv3")
LIB_PATH = os.path.join(CSRC, "libccnet_conv3.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_conv3.h")

CCNET_CONV3_VERSION = 100   # include/ccnet_conv3.h
CCNET_CONV3_E_BADSHAPE, CCNET_CONV3_E_NULLPTR, CCNET_CONV3_E_BADFLAGS, CCNET_CONV3_E_WORKSPACE = -1, -2, -3, -4
CCNET_CONV3_BF16, CCNET_CONV3_F32 = 0, 1
MAX_ELEMS = 1 << 30         # bf16 elements whose byte offsets stay below 2^31

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_conv3.h one to one
_PROTOTYPES = {
    "ccnet_conv3_version": (c_int, []),
    "ccnet_conv3_arch": (c_char_p, []),
    "ccnet_conv3_last_error": (c_char_p, []),
    "ccnet_conv3_bf16": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_long, c_long, c_long, _P]),
    "ccnet_conv3_pack": (c_int, [_P, c_int, _P, _P, c_int, c_int, _P]),
    "ccnet_conv3_wgrad_slabs": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "ccnet_conv3_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "ccnet_conv3_wgrad_bf16": (c_int, [_P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_long, c_long, c_int, _P]),
    "ccnet_conv3_wgrad_finish": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_conv3.h declares."""
    return _clib.declared_symbols(header)


def plan_images(B: int, HW: int, widest: int) -> List[Tuple[int, int]]:
    """[(first image, images)] of the launches that cover B images of HW pixels: every launch takes whole images (taps never
    cross an image boundary, so the cut is exact) and images * HW * ``widest`` < 2^30 elements, ``widest`` the largest row stride
    among the row-strided operands (every byte offset of a launch below 2^31).  An empty list: not even one image fits."""
    if B <= 0 or HW <= 0 or widest <= 0:
        return []
    per = (MAX_ELEMS - 1) // (HW * widest)
    if per <= 0:
        return []
    return [(b0, min(per, B - b0)) for b0 in range(0, B, per)]


class Conv3Error(RuntimeError):
    pass


class Conv3Library(_clib.CLibrary):
    """A loaded libccnet_conv3.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_conv3", Conv3Error
    KERNELS = "3x3 convolution kernels"
    LAST_ERROR = "ccnet_conv3_last_error"


_lib: Optional[Conv3Library] = None


def get_lib() -> Conv3Library:
    """The process-wide device library; raises Conv3Error when it has not been built."""
    return Conv3Library.shared()
