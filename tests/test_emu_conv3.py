"""libccnet_conv3.so's kernels in the SIMT emulator: ccnet_amd/csrc_conv3/conv3_api.hip compiled for the host against tests/emu/
and tests/emu_conv3/ (the emulator twins of the platform headers, first on the include path), driven through the same binding
as the device library on numpy buffers.  The case table and its bars live in tests/conv3_cases.py; tests/test_gpu_conv3.py runs
the same table on the device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conv3_cases as K  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402
from lib_checks import INCLUDE, build_emu_library  # noqa: E402

ROOT = os.path.dirname(HERE)
EMU_DIR, EMU_CONV3_DIR = os.path.join(HERE, "emu"), os.path.join(HERE, "emu_conv3")
CSRC, CONV3_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc"), os.path.join(ROOT, "ccnet_amd", "csrc_conv3")
EMU_LIB = os.path.join(EMU_CONV3_DIR, "libconv3_emu.so")


def build_emu():
    return build_emu_library(EMU_LIB, os.path.join(CONV3_CSRC, "conv3_api.hip"),
                             [EMU_DIR, EMU_CONV3_DIR, CONV3_CSRC, CSRC, INCLUDE])          # the emulator's headers FIRST


@pytest.fixture(scope="module")
def lib():
    from ccnet_amd._conv3_lib import Conv3Library
    return Conv3Library(build_emu())


@pytest.fixture(scope="module")
def mem():
    return HostMemory()


@pytest.mark.parametrize("cid,direction,variant", K.conv_ids(), ids=lambda v: v)
def test_conv_case_table(lib, mem, cid, direction, variant):
    K.run_conv(lib, mem, cid, direction, variant)


@pytest.mark.parametrize("case", K.TAP_CASES, ids=lambda v: "x".join(map(str, v)))
def test_one_hot_tap_shifts_the_image_bit_for_bit(lib, mem, case):
    K.run_tap_shift(lib, mem, case)


@pytest.mark.parametrize("case", K.EPILOGUE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_conv_of_zero_rows_is_the_rounded_bias_plus_addend(lib, mem, case):
    K.run_epilogue(lib, mem, case)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("co,ci", K.PACK_CASES)
def test_pack_matches_numpy(lib, mem, co, ci, f32):
    K.run_pack(lib, mem, co, ci, f32)


@pytest.mark.parametrize("case", K.WGRAD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_weight_gradient_case_table(lib, mem, case):
    K.run_wgrad(lib, mem, case)


@pytest.mark.parametrize("case", K.ONEHOT_CASES, ids=lambda v: "x".join(map(str, v[:6])) + "@" + "x".join(map(str, v[6])))
def test_one_hot_dy_picks_the_shifted_row_bit_for_bit(lib, mem, case):
    K.run_wgrad_onehot(lib, mem, case)


# ---------------------------------------------------------------------------------------------------------------------
# the emulator's other modes (tests/emu_modes.py): LDS-DMAs that land as late as the kernels' own waits allow, and the reversed
# schedule, each held bit for bit to the default mode; and the coverage condition tests/test_emu_modes.py states for the two
# libraries it drives, stated here for this one: every line that calls the stage barrier has run in late mode with an un-landed
# LDS-DMA in the wave's queue, the counted ones with a keep above 0
# ---------------------------------------------------------------------------------------------------------------------
import re  # noqa: E402

import numpy as np  # noqa: E402

import emu_modes as M  # noqa: E402

# nk = 9 with tails | a boundary-spanning tile, both directions | nk = 18 | nk = 27 | two N tiles
MODE_CONV = [("1x5x7-8-8-d2", "fwd", "bias-add-dense"), ("2x9x15-64-64-d2", "fwd", "plain-dense"), ("2x9x15-64-64-d2", "adj", "add-packed"),
             ("1x5x7-128-8-d1", "fwd", "plain-dense"), ("1x5x7-192-8-d2", "fwd", "bias-packed"), ("1x5x7-64-136-d1", "fwd", "bias-packed")]
# one, two, three and five stages per slab: every prologue form of the weight-gradient kernel and its loop's two barriers
MODE_WGRAD = [(1, 5, 7, 8, 64, 1, 1), (1, 10, 10, 136, 72, 1, 1), (2, 9, 15, 64, 64, 2, 2), (2, 9, 15, 16, 24, 2, 1)]
_DEFAULT = {}


def _wgrad_bits(lib, mem, case):
    B, H, W, N, C, d, S = case
    rng = np.random.default_rng(sum(case))
    dy, x = (K.bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((B, H, W, N), (B, H, W, C)))
    part, dw32, dw16, _ = K.launch_wgrad(lib, mem, "dense", dy, x, d, S)
    return part.tobytes() + dw32.tobytes() + dw16.tobytes()


def _in_mode(lib, mem, monkeypatch, mode, key, call):
    M.set_mode(monkeypatch)
    if key not in _DEFAULT:
        _DEFAULT[key] = call()
    M.set_mode(monkeypatch, *mode)
    got = call()
    M.set_mode(monkeypatch)
    return got == _DEFAULT[key]


@pytest.mark.parametrize("mode", ["late", "reversed"])
@pytest.mark.parametrize("cid,direction,variant", MODE_CONV, ids=lambda v: v)
def test_conv_cases_in_the_other_modes(lib, mem, monkeypatch, cid, direction, variant, mode):
    call = lambda: K.conv_bits(lib, mem, cid, direction, variant).tobytes()          # noqa: E731
    assert _in_mode(lib, mem, monkeypatch, (M.LATE,) if mode == "late" else (M.REVERSE,), (cid, direction, variant), call)


@pytest.mark.parametrize("mode", ["late", "reversed"])
@pytest.mark.parametrize("case", MODE_WGRAD, ids=lambda v: "x".join(map(str, v)))
def test_wgrad_cases_in_the_other_modes(lib, mem, monkeypatch, case, mode):
    assert _in_mode(lib, mem, monkeypatch, (M.LATE,) if mode == "late" else (M.REVERSE,), case, lambda: _wgrad_bits(lib, mem, case))


def stage_barrier_lines():
    """{"conv3_kernels.hpp:line": needs a keep above 0} for every line of the kernels that calls stage_barrier<K>()"""
    out = {}
    for i, text in enumerate(open(os.path.join(CONV3_CSRC, "conv3_kernels.hpp")).read().splitlines()):
        for m in re.finditer(r"\bstage_barrier\s*<([^>]*)>\s*\(", text.split("//")[0]):
            key = f"conv3_kernels.hpp:{i + 1}"
            out[key] = out.get(key, False) or m.group(1).strip() != "0"
    return out


def test_every_stage_barrier_line_is_reached_with_a_dma_in_flight(lib, mem, monkeypatch):
    lines = stage_barrier_lines()
    assert len(lines) == 8 and sum(lines.values()) == 5
    # (the platform header defines the barrier on one line; nothing else in the library calls the counted barrier by its own name)
    for f in os.listdir(CONV3_CSRC):
        if f.endswith((".hpp", ".hip")):
            calls = [t for t in open(os.path.join(CONV3_CSRC, f)).read().splitlines() if re.search(r"\bbarrier_dma_keep", t.split("//")[0])]
            assert len(calls) == (1 if f == "conv3_platform.hpp" else 0), (f, calls)
    M.set_mode(monkeypatch, M.LATE)
    for cid, direction, variant in MODE_CONV:
        K.conv_bits(lib, mem, cid, direction, variant)
    for case in MODE_WGRAD:
        _wgrad_bits(lib, mem, case)
    M.set_mode(monkeypatch)
    st = M.vmem_stats(lib.dll)
    missing = {}
    for key, needs_keep in lines.items():
        runs, unlanded, keep, keep_unlanded = st["sites"].get(key, (0, 0, -1, -1))
        if not unlanded:
            missing[key] = "never reached with an un-landed DMA in the queue"
        elif needs_keep and keep_unlanded <= 0:
            missing[key] = "never reached with a keep above 0 and an un-landed DMA in the queue"
    assert not missing, (missing, st["sites"])
    assert st["dma_issued"] > 0 and 0 < st["retired_by_counted_barriers"] <= st["dma_issued"]
