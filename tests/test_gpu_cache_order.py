"""Option "cache_order" on the device: the traversal order of the streaming launches of the split-plane step moves workgroups and
nothing else.  tests/test_emu_cache_order.py holds the same property in the SIMT emulator on an eight-CU device; here the shapes
reach the tail split and the XCD decodes of the real 256-CU grid:

  (8, 64, 65, 4)   row strips 520 = 512 whole + 8 cut, all divisible by 8 with B % 8 == 0: the image-major XCD decode of the NCHW
                   row pass (bits 1 and 5), the tail of the dv row pass
  (8, 64, 4, 97)   column strips 776 on 768 slots: the tail of the two column passes
  (2, 64, 5, 6)    the smallest

The plane-free step of tests/cca_cases.py on guarded buffers: y, A, dq | dk | dv and dgamma start as NaN and ``Arena.settle``
refuses a NaN left in them, the guard bands must stay intact; every order is held bit for bit to order 0."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
from guarded_memory import DeviceMemory  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(8, 64, 65, 4), (8, 64, 4, 97), (2, 64, 5, 6)]
ORDERS = [-1, 1, 2, 4, 8, 16, 32]
BITS = ("y", "A", "dq", "dk", "dv", "dgamma")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _lib
    return _lib.get_lib()


@pytest.fixture(scope="module")
def mem(lib):
    return DeviceMemory()


def step(lib, mem, shape, order):
    with K._options(lib, {"cache_order": order}):
        r = K.run_planes(lib, mem, "tight", True, False, shape, shape[1] // 8, "free")
    for n in BITS:
        assert not K.is_nan(r[n]).any(), (n, "NaN left in an output")
    return r


def test_the_default_is_the_shipped_pattern(lib):
    assert lib.get_option("cache_order") == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_order_moves_workgroups_and_nothing_else(lib, mem, shape):
    ref = step(lib, mem, shape, 0)
    for order in ORDERS:
        got = step(lib, mem, shape, order)
        diff = [n for n in BITS if not np.array_equal(got[n], ref[n])]
        assert not diff, (shape, order, diff)
