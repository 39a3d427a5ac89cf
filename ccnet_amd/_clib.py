"""What the ctypes bindings of the fifteen C-ABI libraries share: the header scan, loading, prototypes, the version check, errors.

Each ``_x_lib.py`` keeps its constants, its ``_PROTOTYPES`` table and a :class:`CLibrary` subclass that names what differs.
There is deliberately NO fallback: a missing library raises.  ``import torch`` must precede the ``CDLL`` of a device library
so that the HIP runtime already mapped by PyTorch (same SONAME ``libamdhip64.so.7``) is the one the library binds to.
"""
from __future__ import annotations

import ctypes
import os
import re
import sys
from typing import List, Optional


def declared_symbols(header: str) -> List[str]:
    """Every function name the C header declares (used by the symbol-export tests)."""
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ccnet_\w+)\s*\(", text)))


class CLibrary:
    """A loaded libccnet_x.so (or, in the CPU tests, the emulator build of the same sources).  The subclass's module holds
    ``LIB_PATH``, ``_PROTOTYPES``, the version constant ``CCNET_X_VERSION`` and the ``_lib`` slot; the subclass sets:"""

    PREFIX = ""                 # "ccnet_x": include/ccnet_x.h, ccnet_x_version, CCNET_X_VERSION, the default ``what`` of check()
    ERROR = RuntimeError        # the library's own RuntimeError subclass
    KERNELS = ""                # "... no CPU or PyTorch fallback for the <KERNELS>."
    LAST_ERROR = None           # name of the exported last-error function, if not ccnet_x_last_error_string
    BUILD_FIRST = "build the HIP extensions first"

    def __init__(self, path: Optional[str] = None):
        module = sys.modules[type(self).__module__]
        path = module.LIB_PATH if path is None else path
        if not os.path.exists(path):
            raise self.ERROR(
                f"{path} not found: {self.BUILD_FIRST} (python -c 'import __graft_entry__ as g; g.build()').  "
                f"ccnet_amd has no CPU or PyTorch fallback for the {self.KERNELS}.")
        self.path = path
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in module._PROTOTYPES.items():
            fn = getattr(self.dll, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        got, want = getattr(self, self.PREFIX + "_version")(), getattr(module, self.PREFIX.upper() + "_VERSION")
        if got != want:
            raise self.ERROR(f"{path} exports C ABI version {got}, this binding is written against "
                             f"{want} (include/{self.PREFIX}.h): rebuild the extension")

    def last_error(self) -> str:
        return getattr(self, self.LAST_ERROR or self.PREFIX + "_last_error_string")().decode()

    def check(self, code: int, what: str = "") -> None:
        if code != 0:
            raise self.ERROR(f"{what or self.PREFIX} failed with code {code}: {self.last_error()}")

    @classmethod
    def shared(cls):
        """The process-wide device library, kept in the subclass's module (``_lib``) and loaded on first use."""
        module = sys.modules[cls.__module__]
        if module._lib is None:
            import torch  # noqa: F401  (map PyTorch's HIP runtime first, see module docstring)
            module._lib = cls(module.LIB_PATH)
        return module._lib
