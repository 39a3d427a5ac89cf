"""Self-tests of the SIMT emulator's late-landing vector-memory model and of its reversed schedule on the toy
kernels of tests/emu_toy/toy_kernels.hpp.  For every kernel the run under a mode differs from the default run exactly as stated:
a test here fails when the rule it names is taken out of tests/emu/hip_emu.cpp."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import emu_modes as M  # noqa: E402

EMU_DIR, TOY_DIR = os.path.join(HERE, "emu"), os.path.join(HERE, "emu_toy")
TOY_LIB = os.path.join(TOY_DIR, "libtoy_emu.so")
HOST_CXX = "/opt/rocm/lib/llvm/bin/clang++"
POISON = 0x7FC0DEAD                      # what the emulator fills a workgroup's LDS with
SENTINEL = np.float32(-1.0)              # toy::kSentinel
NSTAGE = 5


def build_toy():
    srcs = [os.path.join(d, f) for d in (EMU_DIR, TOY_DIR) for f in os.listdir(d) if f.endswith((".hpp", ".cpp"))]
    if os.path.exists(TOY_LIB) and os.path.getmtime(TOY_LIB) >= max(os.path.getmtime(s) for s in srcs):
        return TOY_LIB
    cxx = HOST_CXX if os.path.exists(HOST_CXX) else "g++"
    subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + EMU_DIR, os.path.join(TOY_DIR, "toy_api.cpp"),
                    os.path.join(EMU_DIR, "hip_emu.cpp"), "-o", TOY_LIB], check=True, cwd=HERE)
    return TOY_LIB


@pytest.fixture(scope="module")
def toy():
    return ctypes.CDLL(build_toy())


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _src(n):
    return np.arange(1, n + 1, dtype=np.float32)


def ring(toy, variant):
    src, out = _src(NSTAGE * 128), np.full(NSTAGE * 128, np.nan, np.float32)
    toy.toy_ring(_p(src), _p(out), NSTAGE, variant)
    return out.view(np.uint32)


RING_WANT = _src(NSTAGE * 128).reshape(NSTAGE, 2, 64)[:, ::-1].ravel().view(np.uint32)       # every wave reads the other's half
MODES = {"default": (), "late": (M.LATE,), "reversed": (M.REVERSE,), "late+reversed": (M.LATE, M.REVERSE)}


@pytest.mark.parametrize("mode", MODES)
def test_a_correct_ring_is_bit_identical_in_every_mode(toy, monkeypatch, mode):
    M.set_mode(monkeypatch, *MODES[mode])
    assert np.array_equal(ring(toy, 0), RING_WANT)


@pytest.mark.parametrize("variant", [1, 2], ids=["keep-one-too-large", "lds-only-barrier"])
def test_a_wrong_wait_in_the_ring_shows_in_late_mode_only(toy, monkeypatch, variant):
    for mode in ("default", "reversed"):
        M.set_mode(monkeypatch, *MODES[mode])
        assert np.array_equal(ring(toy, variant), RING_WANT), mode
    M.set_mode(monkeypatch, M.LATE)
    got = ring(toy, variant).reshape(NSTAGE, 128)
    want = RING_WANT.reshape(NSTAGE, 128)
    # the fill of stage s is still in flight when stage s is read
    assert (got[:2] == POISON).all()
    if variant == 1:                               # ... and lands at the next step's wait: the slot holds stage s - 2
        assert np.array_equal(got[2:], want[:-2])
    else:                                          # nothing in the kernel waits for any fill: only its end lands them
        assert (got == POISON).all()


def test_the_teeth_variable_makes_the_correct_ring_fail_like_a_keep_one_too_large(toy, monkeypatch):
    M.set_mode(monkeypatch, M.LATE, M.KEEP_PLUS)
    got = ring(toy, 0)
    M.set_mode(monkeypatch, M.LATE)
    assert np.array_equal(got, ring(toy, 1)) and not np.array_equal(got, RING_WANT)
    M.set_mode(monkeypatch, M.KEEP_PLUS)                         # without the late mode the variable changes nothing
    assert np.array_equal(ring(toy, 0), RING_WANT)


def test_counters_of_the_ring(toy, monkeypatch):
    M.set_mode(monkeypatch, M.LATE)
    M.vmem_stats(toy, reset=True)
    ring(toy, 0)
    st = M.vmem_stats(toy, reset=True)
    assert st["dma_issued"] == 2 * NSTAGE                        # one fill per stage and wave, 64 lanes each
    assert st["retired_by_counted_barriers"] == 2 * NSTAGE       # ... and every one is waited for by a counted barrier
    sites = {k: v for k, v in st["sites"].items() if k.startswith("toy_kernels.hpp:")}
    assert sorted(v[2] for v in sites.values()) == [1, 2]        # the keep<1> line (first and last step) and the keep<2> line
    for runs, unlanded, keep, keep_unlanded in sites.values():
        assert runs == unlanded and keep == keep_unlanded        # every run of them met an un-landed fill
    assert sum(v[0] for v in sites.values()) == 2 * NSTAGE       # per wave and step
    M.set_mode(monkeypatch)
    ring(toy, 0)
    st = M.vmem_stats(toy)
    assert st["dma_issued"] == 0 and not st["sites"]             # the model is off: nothing is counted


def test_one_wave_instruction_is_one_slot_and_an_instruction_no_lane_issues_is_none(toy, monkeypatch):
    src = _src(128)

    def run():
        out, sink = np.full(192, np.nan, np.float32), np.zeros(64, np.float32)
        toy.toy_lane_count(_p(src), _p(out), _p(sink))
        assert np.array_equal(sink, np.where(np.arange(64) & 1, 1, 0).astype(np.float32))      # ordinary stores act at once
        return out.reshape(3, 64)

    M.set_mode(monkeypatch)
    x, y, y_end = run()
    assert np.array_equal(x, src[:64]) and np.array_equal(y, src[64:]) and np.array_equal(y_end, src[64:])
    M.set_mode(monkeypatch, M.LATE)
    x, y, y_end = run()
    assert np.array_equal(x, src[:64])             # X landed: the two stores count at least once (keep<2>: Y and one store)
    assert (y == SENTINEL).all()                   # Y did not: they count at most once
    assert np.array_equal(y_end, src[64:])         # wait_vmem_all() lands everything


def test_syncthreads_waits_for_visible_fills_only_and_an_lds_barrier_for_nothing(toy, monkeypatch):
    src = _src(128)

    def run():
        out = np.full(256, np.nan, np.float32)
        toy.toy_syncthreads(_p(src), _p(out))
        return out.reshape(4, 64)

    M.set_mode(monkeypatch)
    seen = run()
    assert np.array_equal(seen[0], src[:64]) and np.array_equal(seen[1], src[64:])
    assert np.array_equal(seen[2], src[:64]) and np.array_equal(seen[3], src[64:])
    M.set_mode(monkeypatch, M.LATE)
    seen = run()
    assert np.array_equal(seen[0], src[:64]) and np.array_equal(seen[2], src[:64])
    assert (seen[1] == SENTINEL).all() and (seen[3] == SENTINEL).all()


def handover(toy, writer, with_barrier):
    out = np.full(64, np.nan, np.float32)
    toy.toy_handover(_p(out), writer, with_barrier)
    return out.view(np.uint32)


HANDOVER_WANT = (100 + (np.arange(64) + 1) % 64).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("writer", [0, 1])
def test_a_missing_barrier_shows_in_one_schedule_and_its_mirror_image_in_the_other(toy, monkeypatch, writer):
    for reverse in (False, True):
        M.set_mode(monkeypatch, *((M.REVERSE,) if reverse else ()))
        assert np.array_equal(handover(toy, writer, 1), HANDOVER_WANT)            # with its barrier: right in both
        got = handover(toy, writer, 0)
        if (writer == 0) != reverse:               # the writing wave is visited first: the race goes the lucky way
            assert np.array_equal(got, HANDOVER_WANT), (writer, reverse)
        else:
            assert (got == POISON).all(), (writer, reverse)


def test_lanes_whose_instructions_have_no_single_order_abort_and_name_the_site():
    build_toy()
    text = open(os.path.join(TOY_DIR, "toy_kernels.hpp")).read().splitlines()
    lines = [i + 1 for i, t in enumerate(text) if "UNMERGEABLE-" in t]
    assert len(lines) == 2
    code = ("import ctypes, sys; toy = ctypes.CDLL(sys.argv[1]); sink = (ctypes.c_float * 64)(); toy.toy_unmergeable(sink); "
            "print('survived', list(sink)[::32])")
    env = {k: v for k, v in os.environ.items() if k not in M.ALL}
    plain = subprocess.run([sys.executable, "-c", code, TOY_LIB], env=env, capture_output=True, text=True)
    assert plain.returncode == 0 and "survived [1.0, 2.0]" in plain.stdout, plain.stderr     # the default mode does not model the queue
    late = subprocess.run([sys.executable, "-c", code, TOY_LIB], env=dict(env, **{M.LATE: "1"}), capture_output=True, text=True)
    assert late.returncode == -6 and "survived" not in late.stdout, (late.returncode, late.stdout)
    named = [int(n) for n in re.findall(r"toy_kernels\.hpp:(\d+)", late.stderr)]            # the barrier's line, then the branch's
    assert len(named) == 2 and named[0] == lines[1] + 1 and named[1] in lines, late.stderr
