"""The DSN cross-entropy kernel sources (ccnet_amd/csrc_dsn/) run in the SIMT emulator (tests/emu/ + the twin header of
tests/emu_dsn/) through the same C ABI as on the device, against the float64 reference fixtures of tests/golden/dsn_*.npz."""
import numpy as np
import pytest

import dsn_oracle as D
import lib_checks as L
from guarded_memory import HostMemory

SMALL = [n for n in D.CASES if n != "recipe"]       # (the recipe case is the GPU suite's: 2 x 19 x 591 361 emulated pixels)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._dsn_lib import DsnLibrary
    return DsnLibrary(L.build_shared_scaffold_emu("dsn"))


def test_every_case_has_a_fixture():
    assert set(D.fixture_names()) == set(D.CASES)


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernels_match_reference_fixture(emu, name):
    fx = D.load_fixture(name)
    weights = D.WEIGHTS if fx["heads"] == 2 else (1.0, 0.0)
    r = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], weights)
    assert r["intact"] and r["out_of_range"] == 0
    D.check_against_fixture(fx, r["loss"], r["grads"], r["valid"])


def test_emulated_runs_repeat_bitwise_and_scale_with_grad_out(emu):
    fx = D.load_fixture("frac")
    a = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    b = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    c = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], grad_out=0.5)
    assert a["loss"] == b["loss"] and np.array_equal(a["head_loss"], b["head_loss"])
    for ga, gb, gc in zip(a["grads"], b["grads"], c["grads"]):
        assert np.array_equal(ga, gb)
        np.testing.assert_allclose(gc, 0.5 * ga, rtol=1e-6, atol=0)


def test_emulated_out_of_range_labels_are_ignored_and_counted(emu):
    logits, target = D.make_case_inputs(1, 19, 7, 11, 50, 83, seed=31)
    bad = target.copy()
    rng = np.random.default_rng(32)
    pick = rng.random(target.shape) < 0.05
    bad[pick] = rng.integers(19, 255, int(pick.sum()))
    bad[0, 0, :7] = [-1, -5, 19, 254, 256, 2 ** 40, -2 ** 40]
    clean = np.where((bad < 0) | ((bad >= 19) & (bad != 255)), 255, bad)
    r = D.run_raw(emu, HostMemory(), logits, bad)
    q = D.run_raw(emu, HostMemory(), logits, clean)
    assert r["out_of_range"] == int((clean != bad).sum()) > 7 and q["out_of_range"] == 0
    assert r["valid"] == q["valid"] == int((clean != 255).sum())
    assert r["loss"] == q["loss"] and all(np.array_equal(a, b) for a, b in zip(r["grads"], q["grads"]))
