"""Option "stream_policy" in the SIMT emulator: the cache policy of the C-sized streams of the split-plane step selects another
instantiation of the same kernel with the same arguments, and nothing else.

The emulator has no caches, so a policy has no meaning there (ccnet_amd/csrc/cca_policy.hpp forwards to the plain primitives):
what this file proves is the plumbing -- every mask launches the same kernels on the same buffers with the same grids.  The
plane-free step of tests/cca_cases.py (``run_planes``, mode 'free') on guarded buffers whose outputs start as NaN, on the shapes
and the eight-CU device of tests/test_emu_cache_order.py (device id 2, see there): the default (-1 = the shipped mask), every
single bit and all-ones are held bit for bit to mask 0, the step of before the option."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
from emu_util import EmuOps  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402

SHAPES = [(8, 160, 5, 6), (3, 160, 7, 9), (1, 64, 3, 97), (2, 64, 5, 6)]
NBITS = 14
MASKS = [-1] + [1 << b for b in range(NBITS)] + [770, (1 << NBITS) - 1]           # (770: the shipped mask by value)
BITS = ("y", "A", "dq", "dk", "dv", "dgamma")


@pytest.fixture(scope="module")
def lib():
    lib = EmuOps().lib
    lib.dll.cca_emu_set_device(2, 8)
    yield lib
    lib.dll.cca_emu_set_device(0, 0)


@pytest.fixture(scope="module")
def mem():
    return HostMemory()


def step(lib, mem, shape, mask):
    with K._options(lib, {"stream_policy": mask}):
        r = K.run_planes(lib, mem, "tight", True, False, shape, shape[1] // 8, "free")
    for n in BITS:
        assert not K.is_nan(r[n]).any(), (n, "NaN left in an output")
    return r


def test_the_default_is_the_shipped_mask(lib):
    assert lib.get_option("stream_policy") == -1
    assert lib.ccnet_cca_set_option(b"stream_policy", 1 << NBITS, None) == -3
    assert lib.ccnet_cca_set_option(b"stream_policy", -2, None) == -3
    assert lib.get_option("stream_policy") == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_policy_selects_the_same_kernels_with_the_same_arguments(lib, mem, shape):
    ref = step(lib, mem, shape, 0)
    for mask in MASKS:
        got = step(lib, mem, shape, mask)
        diff = [n for n in BITS if not np.array_equal(got[n], ref[n])]
        assert not diff, (shape, mask, diff)
