"""The fused OHEM + DSN criterion's kernel sources (ccnet_amd/csrc_ohem/ohemdsn_*, with ohem_kernels.hpp beside them and
csrc_dsn/dsn_kernels.hpp) run in the SIMT emulator (tests/emu/ + the twin headers of tests/emu_ohem/ and tests/emu_dsn/)
through the same C ABI as on the device, against the reference fixtures of tests/golden/ohemdsn_*.npz and, for the cases no
fixture covers, against tests/ohemdsn_oracle.py.  A dropped tap, a wrong kept flag or a wrong divisor shows here."""
import os

import numpy as np
import pytest

import lib_checks as L
import ohem_oracle as O
import ohemdsn_oracle as D
from conftest import ROOT
from guarded_memory import HostMemory

SMALL = [n for n in D.CASES if n != "recipe" and n not in D.ORACLE_ONLY]       # (the recipe case is the GPU suite's)


def build_emu(force=False):
    amd, tests = os.path.join(ROOT, "ccnet_amd"), os.path.join(ROOT, "tests")
    emu_ohem = os.path.join(tests, "emu_ohem")
    dirs = [emu_ohem, os.path.join(tests, "emu_dsn"), L.EMU_DIR, os.path.join(amd, "csrc_ohem"), os.path.join(amd, "csrc_dsn"),
            L.INCLUDE]
    return L.build_emu_library(os.path.join(emu_ohem, "libohemdsn_emu.so"), os.path.join(amd, "csrc_ohem", "ohemdsn_api.hip"),
                               dirs, reads=(L.EMU_COMMON_DIR, L.COMMON_CSRC), force=force)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._ohemdsn_lib import OhemDsnLibrary
    return OhemDsnLibrary(build_emu())


def test_every_case_has_a_fixture_or_is_the_oracles():
    assert set(D.fixture_names()) == set(D.CASES) - set(D.ORACLE_ONLY)


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernels_match_reference_fixture(emu, name):
    fx = D.load_fixture(name)
    r = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], **fx["args"])
    assert r["intact"]
    D.check_against_fixture(fx, r)


@pytest.mark.parametrize("name", D.ORACLE_ONLY)
def test_emulated_kernels_match_the_oracle_where_the_reference_cannot_run(emu, name):
    logits, target, args = D.case_inputs(name)
    r = D.run_raw(emu, HostMemory(), logits, target, **args)
    assert r["intact"] and r["threshold"] == 1.0 and r["num_valid_zoomed"] == 0
    D.check_against_oracle(name, logits, target, args, r)


def test_emulated_identity_case_equals_the_ohem_kernels_bit_for_bit(emu):
    """scale 1: l1 = 0 on both axes, the interpolated logits are the logits, so threshold and mask are libccnet_ohem's own"""
    from ccnet_amd._ohem_lib import OhemLibrary
    from test_ohem_host import emu_ohem, kept_mask_from_grad
    fx = D.load_fixture("identity")
    r = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], **fx["args"])
    o = emu_ohem(OhemLibrary(L.build_shared_scaffold_emu("ohem")), fx["logits"][0], fx["target"], **fx["args"])
    assert np.float32(r["threshold"]).tobytes() == np.float32(o["threshold"]).tobytes()
    assert np.array_equal(r["kept_mask"], kept_mask_from_grad(o["grad"])) and r["kept"] == o["kept"]
    assert r["num_valid_zoomed"] == o["num_valid"]


def test_emulated_tie_group_at_the_kth_key_is_kept_whole_at_full_resolution(emu):
    """Low-resolution logits constant over 2 x 2 squares (ohem_oracle.make_tie_inputs, block 2), rounded to multiples of 1/8
    so that at the exact ratio 8 -- weights that are multiples of 1/8 -- every interpolated logit inside a square is the
    square's own, bit for bit: the full-resolution pixels of a square share one target probability and the zoomed keys
    form groups of equal values.  min_kept puts the k-th rank inside the largest group; every full-resolution pixel of that
    value is kept."""
    B, C, h, w, H, W = 1, 19, 13, 13, 97, 97
    low, _ = O.make_tie_inputs(B, C, h, w, seed=2, block=2)
    low = (np.round(low * 8) / 8).astype(np.float32)
    rng = np.random.default_rng(3)
    logits = [low, (rng.standard_normal(low.shape) * 3).astype(np.float32)]
    up = D.upsample(low, (H, W)).numpy()
    target = up.argmax(1).astype(np.int64)
    rand = rng.integers(0, C, target.shape)
    pick = rng.random(target.shape) < 0.5
    target[pick] = rand[pick]
    target[rng.random(target.shape) < 0.03] = 255
    groups = [g for g in O.tie_groups(up, target, factor=8, thresh=0.0) if g[2] >= 3][:3]
    assert groups, "no group of equal zoomed keys"
    for value, below, size in groups:
        args = dict(thresh=0.0, min_kept=(below + (size + 1) // 2) * 64)
        r = D.run_raw(emu, HostMemory(), logits, target, **args)
        sel = D.select(low, target, **args)
        assert sel["threshold"] == value
        D.check_against_oracle("tie", logits, target, args, r)
        group = sel["valid"] & (sel["target_prob"] == value)
        assert group.sum() >= size and r["kept_mask"][group].all(), (value, int(r["kept_mask"][group].sum()), int(group.sum()))


def test_emulated_runs_repeat_bitwise_and_scale_with_grad_out(emu):
    fx = D.load_fixture("frac")
    a = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], **fx["args"])
    b = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], **fx["args"])
    c = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], grad_out=0.5, **fx["args"])
    assert a["loss"] == b["loss"] and np.array_equal(a["head_loss"], b["head_loss"]) and a["threshold"] == b["threshold"]
    for ga, gb, gc in zip(a["grads"], b["grads"], c["grads"]):
        assert np.array_equal(ga, gb)
        np.testing.assert_allclose(gc, 0.5 * ga, rtol=1e-6, atol=0)


def test_emulated_out_of_range_labels_are_ignored_and_counted(emu):
    logits, target, args = D.case_inputs("frac", seed=31)
    bad = target.copy()
    rng = np.random.default_rng(32)
    pick = rng.random(target.shape) < 0.05
    bad[pick] = rng.integers(19, 255, int(pick.sum()))
    bad[0, 0, :7] = [-1, -5, 19, 254, 256, 2 ** 40, -2 ** 40]
    clean = np.where((bad < 0) | ((bad >= 19) & (bad != 255)), 255, bad)
    r = D.run_raw(emu, HostMemory(), logits, bad, **args)
    q = D.run_raw(emu, HostMemory(), logits, clean, **args)
    assert r["out_of_range"] == int((clean != bad).sum()) > 7 and q["out_of_range"] == 0
    assert r["valid"] == q["valid"] == int((clean != 255).sum()) and r["kept"] == q["kept"]
    assert r["threshold"] == q["threshold"] and np.array_equal(r["kept_mask"], q["kept_mask"])
    assert r["loss"] == q["loss"] and all(np.array_equal(a, b) for a, b in zip(r["grads"], q["grads"]))


def test_emulated_one_head_module_form_equals_head_zero_of_two(emu):
    """heads == 1 is the OHEM head alone: the same threshold, mask and head-0 gradient as with a second head beside it"""
    fx = D.load_fixture("kth")
    two = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], **fx["args"])
    one = D.run_raw(emu, HostMemory(), fx["logits"][:1], fx["target"], **fx["args"])
    assert one["threshold"] == two["threshold"] and np.array_equal(one["kept_mask"], two["kept_mask"])
    assert one["loss"] == two["head_loss"][0] == one["head_loss"][0] and one["head_loss"][1] == 0
    assert np.array_equal(one["grads"][0], two["grads"][0])
