"""The fused CE + Lovász criterion's kernel sources (ccnet_amd/csrc_lovasz/celovasz_*, with lovasz_kernels.hpp and
lovasz_launch.hpp beside them and csrc_dsn/dsn_kernels.hpp) run in the SIMT emulator (tests/emu/ + the twin headers of
tests/emu_lovasz/ and tests/emu_dsn/) through the same C ABI as on the device, on guarded host buffers with the gradients
pre-filled with NaN, against the reference fixtures of tests/golden/celovasz_*.npz and, for the variants and the cases no
fixture covers, against tests/celovasz_oracle.py.  A dropped tap, a wrong segment base or a wrong divisor shows here."""
import os

import numpy as np
import pytest

import celovasz_oracle as D
import lib_checks as L
from conftest import ROOT
from guarded_memory import HostMemory

FIXTURES = [n for n in D.CASES if n not in D.ORACLE_ONLY]


def build_emu(force=False):
    amd, tests = os.path.join(ROOT, "ccnet_amd"), os.path.join(ROOT, "tests")
    emu_lovasz = os.path.join(tests, "emu_lovasz")
    dirs = [emu_lovasz, os.path.join(tests, "emu_dsn"), L.EMU_DIR, os.path.join(amd, "csrc_lovasz"), os.path.join(amd, "csrc_dsn"),
            L.INCLUDE]
    return L.build_emu_library(os.path.join(emu_lovasz, "libcelovasz_emu.so"), os.path.join(amd, "csrc_lovasz", "celovasz_api.hip"),
                               dirs, reads=(L.EMU_COMMON_DIR, L.COMMON_CSRC), force=force)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._celovasz_lib import CeLovaszLibrary
    return CeLovaszLibrary(build_emu())


def check_saved_regions(r, target, C):
    """the two documented regions of the workspace: the labels as the criterion read them, a finite log-sum-exp where valid"""
    labels, _ = D.clean_labels(target, C)
    assert np.array_equal(r["labels"], np.where(labels == D.IGNORE, -1, labels).astype(np.int16))
    assert np.isfinite(r["lse"][labels != D.IGNORE]).all() and not r["lse"][labels == D.IGNORE].any()


def test_every_case_has_a_fixture_or_is_the_oracles():
    assert set(D.fixture_names()) == set(D.CASES) - set(D.ORACLE_ONLY)


@pytest.mark.parametrize("name", FIXTURES)
def test_emulated_kernels_match_reference_fixture(emu, name):
    fx = D.load_fixture(name)
    r = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    assert r["intact"]
    D.check_against_fixture(fx, r)
    assert np.array_equal(r["grad"], r["grad2"])                        # the backward leaves the workspace as it found it
    check_saved_regions(r, fx["target"], fx["logits"].shape[1])


@pytest.mark.parametrize("variant", list(D.VARIANTS))
def test_emulated_variants_of_s8_match_the_oracle(emu, variant):
    logits, target = D.case_inputs("s8")
    r = D.run_raw(emu, HostMemory(), logits, target, **D.VARIANTS[variant])
    assert r["intact"] and np.array_equal(r["grad"], r["grad2"])
    D.check_against_oracle("s8/" + variant, logits, target, r, **D.VARIANTS[variant])


def test_emulated_out_of_range_labels_are_ignored_by_both_terms_and_counted(emu):
    logits, target = D.case_inputs("out_of_range")
    clean, n_bad = D.clean_labels(target, logits.shape[1])
    r = D.run_raw(emu, HostMemory(), logits, target)
    q = D.run_raw(emu, HostMemory(), logits, clean)
    assert r["out_of_range"] == n_bad > 7 and q["out_of_range"] == 0 and r["valid"] == q["valid"] == int((clean != D.IGNORE).sum())
    assert r["loss"] == q["loss"] and np.array_equal(r["head_loss"], q["head_loss"]) and np.array_equal(r["grad"], q["grad"])
    D.check_against_oracle("out_of_range", logits, target, r)
    check_saved_regions(r, target, logits.shape[1])


def test_emulated_all_ignored_gives_nan_loss_and_a_zero_gradient(emu):
    logits, target = D.case_inputs("ignored")
    r = D.run_raw(emu, HostMemory(), logits, target)
    assert r["intact"] and r["valid"] == 0 and r["n_kept"] == 0
    D.check_against_oracle("ignored", logits, target, r)
    assert np.isnan(r["loss"]) and not r["grad"].any() and not r["grad2"].any()


def test_emulated_runs_repeat_bitwise_and_scale_with_grad_out(emu):
    fx = D.load_fixture("frac")
    a = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    b = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    c = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"], grad_out=0.5)
    assert a["loss"] == b["loss"] == c["loss"] and np.array_equal(a["head_loss"], b["head_loss"])
    assert np.array_equal(a["grad"], b["grad"])
    np.testing.assert_allclose(c["grad"], 0.5 * a["grad"], rtol=1e-6, atol=0)


def test_emulated_identity_case_equals_the_lovasz_kernels_on_the_stock_softmax(emu):
    """scale 1: the interpolated logits are the logits, so the Lovász term is libccnet_lovasz's own on softmax(logits) up to
    the rounding of p (exp(z - lse) here, exp(z - max) / sum there): same kept classes, loss within the bar"""
    import torch
    from ccnet_amd._lovasz_lib import LovaszLibrary
    from test_lovasz_host import emu_lovasz
    fx = D.load_fixture("identity")
    r = D.run_raw(emu, HostMemory(), fx["logits"], fx["target"])
    prob = torch.softmax(torch.from_numpy(fx["logits"]), 1).numpy()
    o = emu_lovasz(LovaszLibrary(L.build_shared_scaffold_emu("lovasz")), prob, fx["target"], ignore=D.IGNORE)
    assert r["n_kept"] == o["n_kept"] and abs(float(r["head_loss"][1]) - o["loss"]) <= D.LOSS_RTOL * abs(o["loss"])
