"""CPU checks of the OHEM cross-entropy (include/ccnet_ohem.h, ccnet_amd/csrc_ohem/): the numpy oracle against the
reference fixtures, its zoom against scipy, the shipped gfx950 library's surface, and the kernel sources themselves run in
the SIMT emulator (tests/emu/ + the OHEM primitives of tests/emu_ohem/) against the oracle."""
import ctypes
import glob
import os

import numpy as np
import pytest

import lib_checks as L
import ohem_oracle as O
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ohem_*.npz")))
SMALL = [f for f in FIXTURES if "769x769" not in f]
OHEM_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_ohem")


def _id(path):
    return os.path.basename(path)[:-4]


def test_fixtures_cover_the_issue_cases():
    names = {_id(f) for f in FIXTURES}
    assert {"ohem_2x19x97x97_kth", "ohem_1x19x129x257_hw", "ohem_1x19x65x65_keepall", "ohem_1x19x65x97_minkept0",
            "ohem_1x19x33x33_ignored", "ohem_2x19x97x97_below", "ohem_1x19x769x769_recipe"} <= names


@pytest.mark.parametrize("path", FIXTURES, ids=_id)
def test_oracle_reproduces_reference_fixture(path):
    fx = O.load_fixture(path)
    o = O.ohem(fx["logits"], fx["target"], **fx["args"])
    np.testing.assert_array_equal(o["new_target"], fx["new_target"])
    assert o["threshold"] == fx["threshold"]
    if np.isnan(fx["loss"]):
        assert np.isnan(o["loss"])
    else:
        assert abs(o["loss"] - float(fx["loss"])) <= 1e-6 * abs(float(fx["loss"]))
    O.check_against_fixture(fx, o["threshold"], o["new_target"] != 255, o["loss"], o["grad"])


@pytest.mark.parametrize("factor", [4, 8])
@pytest.mark.parametrize("n", [65, 97, 129, 257, 513, 769])
def test_numpy_zoom_equals_scipy(n, factor):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(n * 10 + factor)
    prob = rng.random((2, 3, n, n)).astype(np.float32)
    lab = rng.integers(0, 19, (2, n, n)).astype(np.int64)
    np.testing.assert_array_equal(O.zoom_order1(prob, factor), nd.zoom(prob, (1.0, 1.0, 1.0 / factor, 1.0 / factor), order=1))
    np.testing.assert_array_equal(O.zoom_order0(lab, factor), nd.zoom(lab, (1.0, 1.0 / factor, 1.0 / factor), order=0))


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ohem_lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _ohem_lib
    return _ohem_lib.LIB_PATH


def test_library_exports_exactly_the_header(ohem_lib_path):
    from ccnet_amd import _ohem_lib
    names = _ohem_lib.declared_symbols()
    assert set(names) == set(_ohem_lib._PROTOTYPES) and len(names) == 6
    assert L.exported_symbols(ohem_lib_path) == names


def test_library_contains_gfx950_code(ohem_lib_path):
    blob = open(ohem_lib_path, "rb").read()
    assert b"gfx950" in blob and b"select_kernel" in blob and b"forward_kernel" in blob


def test_version_and_argument_validation_without_a_gpu(ohem_lib_path):
    from ccnet_amd import _ohem_lib
    lib = _ohem_lib.OhemLibrary(ohem_lib_path)
    assert lib.ccnet_ohem_version() == 100 and lib.ccnet_ohem_arch() == b"gfx950"
    assert lib.ccnet_ohem_workspace_bytes(0, 19, 97, 97, 8) == 0
    n = lib.ccnet_ohem_workspace_bytes(2, 19, 97, 97, 8)
    assert n >= 4 * (2 * 12 * 12 + 2 * 2 * 97 * 97)
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    assert lib.ccnet_ohem_forward_f32(p, p, p, None, None, None, p, n, 0, 19, 97, 97, 255, 0.7, 100000, 8, None) == -1
    assert lib.ccnet_ohem_forward_f32(p, p, p, None, None, None, p, n, 2, 19, 97, 97, 255, 0.7, -1, 8, None) == -1
    assert lib.ccnet_ohem_forward_f32(p, p, p, None, None, None, p, n, 2, 19, 97, 97, 255, 0.7, 100000, 0, None) == -1
    assert lib.ccnet_ohem_forward_f32(None, p, p, None, None, None, p, n, 2, 19, 97, 97, 255, 0.7, 100000, 8, None) == -2
    assert lib.ccnet_ohem_forward_f32(p, p, p, None, None, None, p, n - 1, 2, 19, 97, 97, 255, 0.7, 100000, 8, None) == -3
    assert "workspace" in lib.last_error()
    assert lib.ccnet_ohem_backward_f32(p, p, None, p, n, 2, 19, 97, 97, 8, None) == -2
    assert lib.ccnet_ohem_backward_f32(p, p, p, p, n, 2, 19, 97, 0, 8, None) == -1
    assert lib.ccnet_ohem_backward_f32(p, p, p, p, 16, 2, 19, 97, 97, 8, None) == -3
    assert lib.last_error().startswith("ccnet_ohem:")


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(ohem_lib_path, tmp_path):
    kernels = L.code_object_kernels(ohem_lib_path, tmp_path, "_ZN4ohem")
    assert len(kernels) == 5, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_sources_carry_no_env_knobs_and_no_emulator_code():
    files = L.product_sources(OHEM_CSRC, L.COMMON_CSRC)
    assert "ohem_api.hip" in files and "ccnet_device.hpp" in files and "ccnet_host.hpp" in files
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._ohem_lib import OhemLibrary
    return OhemLibrary(L.build_shared_scaffold_emu("ohem"))


def emu_ohem(lib, logits, target, ignore_label=255, thresh=0.7, min_kept=100000, factor=8, grad_out=1.0):
    """forward + backward through the emulated C ABI with numpy buffers standing in for device memory."""
    B, C, H, W = logits.shape
    logits = np.ascontiguousarray(logits, np.float32)
    target = np.ascontiguousarray(target, np.int64)
    n = lib.ccnet_ohem_workspace_bytes(B, C, H, W, factor)
    ws = np.full(n // 4 + 1, np.nan, np.float32)
    loss, thr = np.full(1, np.nan, np.float32), np.full(1, np.nan, np.float32)
    counts = np.full(2, -7, np.int32)
    lib.check(lib.ccnet_ohem_forward_f32(logits.ctypes.data, target.ctypes.data, loss.ctypes.data, thr.ctypes.data,
                                         counts.ctypes.data, counts.ctypes.data + 4, ws.ctypes.data, n, B, C, H, W,
                                         ignore_label, thresh, min_kept, factor, None), "forward")
    g = np.full(1, grad_out, np.float32)
    grad = np.full_like(logits, np.nan)
    lib.check(lib.ccnet_ohem_backward_f32(g.ctypes.data, logits.ctypes.data, grad.ctypes.data, ws.ctypes.data, n,
                                          B, C, H, W, factor, None), "backward")
    return {"loss": float(loss[0]), "threshold": thr[0], "kept": int(counts[0]), "num_valid": int(counts[1]), "grad": grad}


def kept_mask_from_grad(grad):
    """A kept pixel has a nonzero gradient row (p_target < 1 at these logits), every other pixel an all-zero one."""
    return (grad != 0).any(axis=1)


@pytest.mark.parametrize("path", SMALL, ids=_id)
def test_emulated_kernels_match_reference_fixture(emu, path):
    fx = O.load_fixture(path)
    r = emu_ohem(emu, fx["logits"], fx["target"], **fx["args"])
    o = O.ohem(fx["logits"], fx["target"], **fx["args"])
    assert r["num_valid"] == o["num_valid"]
    mask = kept_mask_from_grad(r["grad"])
    assert r["kept"] == int(mask.sum())
    O.check_against_fixture(fx, r["threshold"], mask, r["loss"], r["grad"])


@pytest.mark.parametrize("case", O.EDGE_CASES)
def test_emulated_edge_cases_match_oracle(emu, case):
    logits, target, case = O.edge_case_inputs(case)
    r = emu_ohem(emu, logits, target, **case)
    o = O.ohem(logits, target, **case)
    assert r["num_valid"] == o["num_valid"]
    assert O.ulp_distance(r["threshold"], o["threshold"]) <= 2
    mask = kept_mask_from_grad(r["grad"])
    np.testing.assert_array_equal(mask, o["new_target"] != case.get("ignore_label", 255))
    assert abs(r["loss"] - o["loss"]) <= 1e-5 * abs(o["loss"])
    assert np.abs(r["grad"] - o["grad"]).max() <= 1e-5 * np.abs(o["grad"]).max()


def test_emulated_tie_group_at_the_kth_key_is_kept_whole(emu):
    """Many equal zoomed keys; the k-th is the last of its group, so one rank more selects the next larger value."""
    logits, target = O.make_tie_inputs(1, 19, 128, 192, seed=2)
    groups = [g for g in O.tie_groups(logits, target, factor=4, thresh=0.002) if g[2] >= 4][:6]
    assert len(groups) >= 3
    for value, below, size in groups:
        args = dict(thresh=0.002, min_kept=(below + size) * 16, factor=4)
        r = emu_ohem(emu, logits, target, **args)
        mask = kept_mask_from_grad(r["grad"])
        o, _ = O.check_result(logits, target, args, r["threshold"], mask, r["loss"], r["grad"])
        group = o["valid"] & (o["target_prob"] == value)
        assert o["threshold"] == value and group.sum() >= size and mask[group].all(), (value, int(mask[group].sum()))


def test_emulated_all_ignored_gives_nan_loss_and_zero_gradient(emu):
    logits, target = O.make_case_inputs(1, 19, 16, 16, seed=3, all_ignored=True)
    r = emu_ohem(emu, logits, target, thresh=0.7, min_kept=0, factor=4)
    assert np.isnan(r["loss"]) and r["kept"] == 0 and r["num_valid"] == 0 and r["threshold"] == 1.0
    assert np.all(r["grad"] == 0)


def test_emulated_gradient_scales_with_grad_out_and_repeats_bitwise(emu):
    logits, target = O.make_case_inputs(1, 19, 33, 41, seed=11)
    a = emu_ohem(emu, logits, target, thresh=0.7, min_kept=2000, factor=8, grad_out=1.0)
    b = emu_ohem(emu, logits, target, thresh=0.7, min_kept=2000, factor=8, grad_out=1.0)
    c = emu_ohem(emu, logits, target, thresh=0.7, min_kept=2000, factor=8, grad_out=0.5)
    assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"])
    np.testing.assert_allclose(c["grad"], 0.5 * a["grad"], rtol=1e-6, atol=0)


def test_cpu_input_raises_instead_of_falling_back():
    import torch
    from ccnet_amd import CriterionOhemDSN, OhemCrossEntropy2d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OhemCrossEntropy2d()(torch.randn(1, 19, 16, 16), torch.zeros(1, 16, 16, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CriterionOhemDSN()([torch.randn(1, 19, 4, 4), torch.randn(1, 19, 4, 4)], torch.zeros(1, 16, 16, dtype=torch.long))


def test_train_driver_flags():
    from ccnet_amd.train_synthetic import build_parser
    a = build_parser().parse_args([])
    assert a.ohem is False and a.ohem_thres == 0.6 and a.ohem_keep == 200000
    a = build_parser().parse_args(["--ohem", "--ohem-thres", "0.7", "--ohem-keep", "100000"])
    assert a.ohem and a.ohem_thres == 0.7 and a.ohem_keep == 100000
