"""ctypes binding of the C ABI declared in include/ccnet_augment.h (the training input pipeline: scale, pad, crop, mirror and
label remap as one gather over packed uint8 frames).

The product loads ``ccnet_amd/csrc_augment/libccnet_augment.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside the others (:mod:`ccnet_amd._clib` holds what the bindings share).  As with
:mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_void_p
from typing import List, Optional

from . import _clib

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_augment")
LIB_PATH = os.path.join(CSRC, "libccnet_augment.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_augment.h")

CCNET_AUGMENT_VERSION = 100    # include/ccnet_augment.h
DESC_INTS = 16                 # CCNET_AUGMENT_DESC_INTS
(FRAME_OFF, LABEL_OFF, HS, WS, PITCH, NUM, DEN, HZ, WZ, H_OFF, W_OFF, MIRROR) = range(12)      # CCNET_AUGMENT_<field>
MAX_RATIO = 1024               # CCNET_AUGMENT_MAX_RATIO
MAX_SIDE = 65535               # CCNET_AUGMENT_MAX_SIDE

_P = c_void_p  # every tensor argument is a raw pointer

# name -> (restype, argtypes); mirrors include/ccnet_augment.h one to one
_PROTOTYPES = {
    "ccnet_augment_version": (c_int, []),
    "ccnet_augment_arch": (c_char_p, []),
    "ccnet_augment_last_error_string": (c_char_p, []),
    "ccnet_augment_scaled_size": (c_int, [c_int] * 4 + [POINTER(c_int)] * 2),
    "ccnet_augment_crop_u8": (c_int, [_P, c_size_t, _P, c_size_t, _P, _P, _P, _P, _P] + [c_int] * 3 + [c_float] * 3
                              + [c_int] * 2 + [_P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_augment.h declares."""
    return _clib.declared_symbols(header)


class AugmentError(RuntimeError):
    pass


class AugmentLibrary(_clib.CLibrary):
    """A loaded libccnet_augment.so (or, in the CPU tests, the emulator build of the same sources)."""

    PREFIX, ERROR = "ccnet_augment", AugmentError
    KERNELS = "input-pipeline kernel"

    def scaled_size(self, h: int, w: int, num: int, den: int):
        """(Hz, Wz) by the library's own arithmetic; raises outside its limits."""
        hz, wz = c_int(0), c_int(0)
        self.check(self.ccnet_augment_scaled_size(h, w, num, den, hz, wz), "ccnet_augment_scaled_size")
        return hz.value, wz.value


_lib: Optional[AugmentLibrary] = None


def get_lib() -> AugmentLibrary:
    """The process-wide device library; raises AugmentError when it has not been built."""
    return AugmentLibrary.shared()
