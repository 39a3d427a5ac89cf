"""Option "stream_policy" on the device: the cache policy of the C-sized streams of the split-plane step (non-temporal loads and
stores, 16-byte write-through stores; ccnet_amd/csrc/cca_policy.hpp) changes where a line is kept and nothing else.

  (8, 64, 65, 4)    row strips 520 = 512 whole + 8 cut: the XCD decode of the NCHW row pass, the tail of the dv row pass
  (8, 64, 4, 97)    column strips 776 on 768 slots: the tail of the two column passes
  (2, 64, 5, 6)     the smallest
  (1, 128, 100, 7)  two channel groups at the full 100-position tile: a ring fill and the previous group's stores are in flight
                    together under the new modifiers

The plane-free step of tests/cca_cases.py on guarded buffers: y, A, dq | dk | dv and dgamma start as NaN and ``Arena.settle``
refuses a NaN left in them, the guard bands must stay intact; the default (-1 = the shipped mask), every single bit and all-ones
are held bit for bit to mask 0, the step of before the option."""
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
SHAPES = [(8, 64, 65, 4), (8, 64, 4, 97), (2, 64, 5, 6), (1, 128, 100, 7)]
NBITS = 14
MASKS = [-1] + [1 << b for b in range(NBITS)] + [770, (1 << NBITS) - 1]           # (770: the shipped mask by value)
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


def step(lib, mem, shape, mask):
    with K._options(lib, {"stream_policy": mask}):
        r = K.run_planes(lib, mem, "tight", True, False, shape, shape[1] // 8, "free")
    for n in BITS:
        assert not K.is_nan(r[n]).any(), (n, "NaN left in an output")
    return r


def test_the_default_is_the_shipped_mask(lib):
    assert lib.get_option("stream_policy") == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_policy_changes_no_bit(lib, mem, shape):
    ref = step(lib, mem, shape, 0)
    for mask in MASKS:
        got = step(lib, mem, shape, mask)
        diff = [n for n in BITS if not np.array_equal(got[n], ref[n])]
        assert not diff, (shape, mask, diff)
