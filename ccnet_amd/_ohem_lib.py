"""ctypes binding of the C ABI declared in include/ccnet_ohem.h (the OHEM cross-entropy library).

The product loads ``ccnet_amd/csrc_ohem/libccnet_ohem.so`` (built for gfx950 by ``__graft_entry__.build()``), a library
of its own beside libccnet_cca.so.  As with :mod:`ccnet_amd._lib` there is no fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc_ohem")
LIB_PATH = os.path.join(CSRC, "libccnet_ohem.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ccnet_ohem.h")

CCNET_OHEM_VERSION = 100       # include/ccnet_ohem.h

_P = c_void_p  # every tensor argument is a raw device pointer

# name -> (restype, argtypes); mirrors include/ccnet_ohem.h one to one
_PROTOTYPES = {
    "ccnet_ohem_version": (c_int, []),
    "ccnet_ohem_arch": (c_char_p, []),
    "ccnet_ohem_last_error_string": (c_char_p, []),
    "ccnet_ohem_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ccnet_ohem_forward_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int,
                                       c_longlong, c_float, c_int, c_int, _P]),
    "ccnet_ohem_backward_f32": (c_int, [_P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
}


def declared_symbols(header: str = HEADER_PATH) -> List[str]:
    """Every function name include/ccnet_ohem.h declares."""
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ccnet_\w+)\s*\(", text)))


class OhemError(RuntimeError):
    pass


class OhemLibrary:
    """A loaded libccnet_ohem.so (or, in the CPU tests, the emulator build of the same sources)."""

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise OhemError(
                f"{path} not found: build the HIP extensions first (python -c 'import __graft_entry__ as g; g.build()').  "
                "ccnet_amd has no CPU or PyTorch fallback for the OHEM cross-entropy kernels.")
        self.path = path
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        if self.ccnet_ohem_version() != CCNET_OHEM_VERSION:
            raise OhemError(f"{path} exports C ABI version {self.ccnet_ohem_version()}, this binding is written against "
                            f"{CCNET_OHEM_VERSION} (include/ccnet_ohem.h): rebuild the extension")

    def last_error(self) -> str:
        return self.ccnet_ohem_last_error_string().decode()

    def check(self, code: int, what: str = "") -> None:
        if code != 0:
            raise OhemError(f"{what or 'ccnet_ohem'} failed with code {code}: {self.last_error()}")


_lib: Optional[OhemLibrary] = None


def get_lib() -> OhemLibrary:
    """The process-wide device library; raises OhemError when it has not been built."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (map PyTorch's HIP runtime first, as _lib.get_lib does)
        _lib = OhemLibrary(LIB_PATH)
    return _lib
