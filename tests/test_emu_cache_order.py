"""Option "cache_order" in the SIMT emulator: the traversal order of the streaming launches of the split-plane step (forward
column / NCHW row pass, dA, dv column / row pass) moves workgroups and nothing else.

The plane-free step of tests/cca_cases.py (``run_planes``, mode 'free') on guarded buffers: y, A, dq | dk | dv and dgamma start
as NaN and ``Arena.settle`` refuses a NaN in any of them after the call, so a strip that no workgroup visited shows as the
prefill left in place; a strip visited twice cannot show in the bits, but the grid holds exactly one workgroup per
(strip, channel range), so one visited twice means another one skipped.  Every order -- the default (-1), every single bit -- is
held bit for bit to order 0, the traversal of before the option.

The emulated device has eight CUs (16 row slots, 24 column slots), so the tail split, the XCD-aware decode and the image-major
XCD decode are reached at toy sizes.  It is device id 2: the host caches the CU count per device id for the life of the process
(num_cus, cca_api.hip) and tests/test_emu_modes.py runs its multi-stage cases on id 1 with TWO CUs -- an eight-CU id 1 set here
first would leave those cases on eight CUs and their barriers between channel groups unreached.  "planes_stream" 3 makes three
persistent dA workgroups walk many strips each, in reverse, across ring boundaries.  The whole table runs again under CCA_EMU_REVERSE: the counted barriers of the dA ring must not depend on
which strip a workgroup drew."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
import emu_modes as M  # noqa: E402
from emu_util import EmuOps  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402

SHAPES = [
    (8, 160, 5, 6),      # row strips 40 on 16 slots: n_whole 32 + 8 cut strips, all divisible by 8 and B % 8 == 0 -> the image-major
                         # XCD decode (bits 1 and 5); 160 = 2 x 64 + 32: the last channel group is partial
    (3, 160, 7, 9),      # column strips 27 on 24 slots: 3 cut strips; row strips 21: no XCD decode, the linear one reversed
    (1, 64, 3, 97),      # one image, the longest strip
    (2, 64, 5, 6),       # the smallest
]
ORDERS = [-1, 1, 2, 4, 8, 16, 32]
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


def step(lib, mem, shape, stream, order):
    with K._options(lib, {"planes_stream": stream, "cache_order": order}):
        r = K.run_planes(lib, mem, "tight", True, False, shape, shape[1] // 8, "free")
    for n in BITS:                                   # (settle has refused NaN already; said here once more, on the bits returned)
        assert not K.is_nan(r[n]).any(), (n, "NaN left in an output")
    return r


def test_the_default_is_the_shipped_pattern(lib):
    assert lib.get_option("cache_order") == -1
    assert lib.ccnet_cca_set_option(b"cache_order", 64, None) == -3 and lib.ccnet_cca_set_option(b"cache_order", -2, None) == -3
    assert lib.get_option("cache_order") == -1


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending-schedule", "reversed-schedule"])
@pytest.mark.parametrize("stream", [1, 3], ids=["stream1", "stream3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_order_moves_workgroups_and_nothing_else(lib, mem, monkeypatch, shape, stream, reverse):
    M.set_mode(monkeypatch, *((M.REVERSE,) if reverse else ()))
    ref = step(lib, mem, shape, stream, 0)
    for order in ORDERS:
        got = step(lib, mem, shape, stream, order)
        diff = [n for n in BITS if not np.array_equal(got[n], ref[n])]
        assert not diff, (shape, stream, order, diff)
