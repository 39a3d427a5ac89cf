"""The memory behaviour of the pixel-major and split-plane families of the attention core in the SIMT emulator: the case
table of tests/cca_cases.py -- every entry point on guarded buffers in the dense, packed, padded and tight view forms, with an
exact-size workspace -- through the emulator build of the kernel sources on numpy buffers.  tests/test_gpu_cca_bounds.py runs
the same table on the device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
from emu_util import EmuOps  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return EmuOps().lib


@pytest.fixture(scope="module")
def mem():
    return HostMemory()


@pytest.mark.parametrize("cid,form", K.ids(emulator=True), ids=lambda v: v)
def test_views_bands_and_workspace(lib, mem, cid, form):
    K.run_case(lib, mem, cid, form)
