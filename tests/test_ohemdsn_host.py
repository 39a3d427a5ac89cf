"""CPU checks of the fused OHEM + DSN criterion (include/ccnet_ohemdsn.h, ccnet_amd/csrc_ohem/ohemdsn_*): its place in the
build table, the shipped gfx950 library's surface, its binding's refusals, the workspace cap, every argument check without a
device, the oracle against the reference fixtures, and the public layer's and the training driver's refusals."""
import ctypes
import fnmatch
import os

import numpy as np
import pytest

import lib_checks as L
import ohem_oracle as O
import ohemdsn_oracle as D
from conftest import ROOT

RECIPE_B8 = (8, 19, 97, 97, 769, 769)


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _ohemdsn_lib
    return _ohemdsn_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _ohemdsn_lib
    return _ohemdsn_lib.OhemDsnLibrary(lib_path)


def test_build_table_keeps_seven_rows_and_the_ohem_row_has_the_unit():
    import __graft_entry__ as g
    assert len(g.EXTENSIONS) == 7
    row = [e for e in g.EXTENSIONS if e.name == "ohem"][0]
    assert [u.name for u in row.libraries()] == ["ohem", "ohemdsn"]
    unit = row.units[0]
    dsn = os.path.join(ROOT, "ccnet_amd", "csrc_dsn")
    assert unit.csrc == row.csrc and unit.binding == "_ohemdsn_lib" and unit.exports.endswith("ohemdsn_exports.map")
    assert unit.unit.endswith(os.path.join("csrc_ohem", "ohemdsn_api.hip")) and unit.header.endswith("ccnet_ohemdsn.h")
    assert g.OHEMDSN_LIB.endswith(os.path.join("csrc_ohem", "libccnet_ohemdsn.so"))
    # the extra directory is the unit's alone: on its include path and among its sources, not on the row's
    assert g.OHEMDSN_HIPCC_FLAGS[-1] == "-I" + dsn and "-I" + dsn not in g.OHEM_HIPCC_FLAGS
    assert os.path.join(dsn, "dsn_kernels.hpp") in unit.sources() and os.path.join(dsn, "dsn_kernels.hpp") not in row.sources()
    assert sum(len(e.libraries()) for e in g.EXTENSIONS) == 9


def test_the_ohem_librarys_build_line_is_the_parent_commits():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "ccnet_amd", "csrc_ohem")
    assert g.OHEM_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(csrc, "exports.map"), "-I" + csrc,
                                                  "-I" + os.path.join(ROOT, "include")]
    eval_row = [e for e in g.EXTENSIONS if e.name == "eval"][0]
    assert eval_row.units[0].flags[len(g._BASE_FLAGS) + 1:] == eval_row.flags[len(g._BASE_FLAGS) + 1:]


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _ohemdsn_lib
    names = _ohemdsn_lib.declared_symbols()
    assert names == sorted(["ccnet_ohemdsn_version", "ccnet_ohemdsn_arch", "ccnet_ohemdsn_last_error",
                            "ccnet_ohemdsn_workspace_bytes", "ccnet_ohemdsn_forward_f32", "ccnet_ohemdsn_backward_f32"])
    assert set(names) == set(_ohemdsn_lib._PROTOTYPES)
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"_ZN7ohemdsn16zoom_keys_kernel" in blob and b"_ZN7ohemdsn14forward_kernel" in blob
    assert b"_ZN7ohemdsn15backward_kernel" in blob and b"_ZN7ohemdsn15finalize_kernel" in blob
    assert b"_ZN4ohem13select_kernel" in blob                       # the select is libccnet_ohem's own kernel, reused


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN7ohemdsn")
    assert len(kernels) == 4, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad
    select = L.code_object_kernels(lib_path, tmp_path, "_ZN4ohem13select_kernel")
    assert len(select) == 1 and not L.kernels_using_scratch(select)


def test_sources_restate_neither_the_up_sample_nor_the_zoom():
    files = L.product_sources(os.path.join(ROOT, "ccnet_amd", "csrc_ohem"))
    assert {"ohemdsn_api.hip", "ohemdsn_kernels.hpp"} <= set(files)
    text = files["ohemdsn_kernels.hpp"]
    for name in ("axis_taps", "bilinear", "candidates", "pick3", "pixel_head"):
        assert "dsn::" + name in text and " " + name + "(" not in text.replace("dsn::" + name + "(", ""), name
    assert "ohem::zoom_key(" in text and "floor(" not in text and "kSelectThreads" not in text
    assert "ohem::select_kernel" in files["ohemdsn_api.hip"] and "ohem::zoom_step" in files["ohemdsn_api.hip"]
    for f in ("ohemdsn_api.hip", "ohemdsn_kernels.hpp"):
        assert "atomicAdd" not in files[f] and "lds_inc" not in files[f], f            # the backward is a gather


def test_binding_refuses_a_missing_library_and_another_abi_version(lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _ohemdsn_lib as m
    from ccnet_amd._dsn_lib import DsnError
    from ccnet_amd._ohem_lib import OhemError
    assert issubclass(m.OhemDsnError, RuntimeError) and not issubclass(m.OhemDsnError, (OhemError, DsnError))
    with pytest.raises(m.OhemDsnError, match="not found"):
        m.OhemDsnLibrary(str(tmp_path / "libccnet_missing.so"))
    assert m.OhemDsnLibrary(m.LIB_PATH).path == m.LIB_PATH
    monkeypatch.setattr(m, "CCNET_OHEMDSN_VERSION", m.CCNET_OHEMDSN_VERSION + 1)
    with pytest.raises(m.OhemDsnError, match="rebuild"):
        m.OhemDsnLibrary(m.LIB_PATH)


@pytest.mark.parametrize("shape,heads", [(c[:6], c[7]) for c in D.CASES.values()] + [(RECIPE_B8, 2), (RECIPE_B8, 1)],
                         ids=list(D.CASES) + ["recipe_b8", "recipe_b8_one_head"])
def test_workspace_obeys_the_cap(lib, shape, heads):
    B, C, h, w, H, W = shape
    n = lib.ccnet_ohemdsn_workspace_bytes(B, C, h, w, H, W, heads, 8)
    M = B * O.zoom_out_size(H, 8) * O.zoom_out_size(W, 8)
    assert 0 < n <= 16 * B * H * W + 4 * M + 65536, n
    assert n >= (4 * heads + 2) * B * H * W + 4 * M          # a log-sum-exp per head, a two-byte label, the keys
    if B * H * W >= 1024:                                    # (the 3 x 30 case is smaller than the alignment padding)
        assert n < B * C * H * W                             # nothing logits-sized at full resolution (C >= 19 here)


BAD_SHAPES = [(0, 19, 13, 13, 97, 97, 2, 8), (1, 0, 13, 13, 97, 97, 2, 8), (1, 257, 13, 13, 97, 97, 2, 8),
              (1, 19, 0, 13, 97, 97, 2, 8), (1, 19, 13, 0, 97, 97, 2, 8), (1, 19, 98, 13, 97, 97, 2, 8),
              (1, 19, 13, 98, 97, 97, 2, 8), (1, 19, 13, 13, 97, 97, 0, 8), (1, 19, 13, 13, 97, 97, 3, 8),
              (-1, 19, 13, 13, 97, 97, 2, 8), (4, 19, 97, 97, 32768, 32768, 2, 8), (1, 19, 1, 1, (1 << 20) + 1, 1, 1, 8),
              (32768, 1, 1, 1, 1, 1, 1, 8), (1, 19, 13, 13, 97, 97, 2, 0), (1, 19, 13, 13, 97, 97, 2, -8)]


@pytest.mark.parametrize("shape", BAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_of_contract_shapes_are_refused_without_a_device(lib, shape):
    assert lib.ccnet_ohemdsn_workspace_bytes(*shape) == 0
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    geometry, factor = shape[:7], shape[7]
    assert lib.ccnet_ohemdsn_forward_f32(p, p, p, 255, 0.7, 100000, factor, p, p, p, p, p, 1 << 30, *geometry, None) == -1
    assert "unsupported shape" in lib.last_error() and lib.last_error().startswith("ccnet_ohemdsn:")
    assert lib.ccnet_ohemdsn_backward_f32(p, p, p, p, p, p, 1 << 30, *geometry, factor, None) == -1


def test_version_and_argument_validation_without_a_gpu(lib):
    assert lib.ccnet_ohemdsn_version() == 100 and lib.ccnet_ohemdsn_arch() == b"gfx950"
    assert lib.ccnet_ohemdsn_workspace_bytes(1, 256, 97, 97, 97, 97, 2, 1) > 0      # the bounds themselves are inside the contract
    assert lib.ccnet_ohemdsn_workspace_bytes(1, 19, 2, 5, 3, 30, 2, 8) > 0          # an empty zoomed grid is inside it too
    shape = (2, 19, 13, 13, 97, 97)
    n = lib.ccnet_ohemdsn_workspace_bytes(*shape, 2, 8)
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    fwd = lambda *a: lib.ccnet_ohemdsn_forward_f32(*a)                            # noqa: E731
    assert fwd(p, p, p, 255, 0.7, -1, 8, p, p, p, p, p, n, *shape, 2, None) == -1          # min_kept < 0
    assert "min_kept" in lib.last_error()
    assert fwd(p, p, p, 255, float("nan"), 100000, 8, p, p, p, p, p, n, *shape, 2, None) == -1
    assert fwd(None, p, p, 255, 0.7, 100000, 8, p, p, p, p, p, n, *shape, 2, None) == -2
    assert fwd(p, None, p, 255, 0.7, 100000, 8, p, p, p, p, p, n, *shape, 2, None) == -2   # two heads need the second logits
    assert fwd(p, p, None, 255, 0.7, 100000, 8, p, p, p, p, p, n, *shape, 2, None) == -2
    assert fwd(p, p, p, 255, 0.7, 100000, 8, None, p, p, p, p, n, *shape, 2, None) == -2
    assert fwd(p, p, p, 255, 0.7, 100000, 8, p, p, p, p, None, n, *shape, 2, None) == -2
    assert "NULL" in lib.last_error()
    assert fwd(p, p, p, 255, 0.7, 100000, 8, p, p, p, p, p, n - 1, *shape, 2, None) == -3
    assert "workspace" in lib.last_error()
    bwd = lambda *a: lib.ccnet_ohemdsn_backward_f32(*a)                           # noqa: E731
    assert bwd(None, p, p, p, p, p, n, *shape, 2, 8, None) == -2
    assert bwd(p, None, p, p, p, p, n, *shape, 2, 8, None) == -2
    assert bwd(p, p, None, p, p, p, n, *shape, 2, 8, None) == -2
    assert bwd(p, p, p, None, p, p, n, *shape, 2, 8, None) == -2
    assert bwd(p, p, p, p, None, p, n, *shape, 2, 8, None) == -2
    assert bwd(p, p, p, p, p, None, n, *shape, 2, 8, None) == -2
    assert bwd(p, p, p, p, p, p, 16, *shape, 2, 8, None) == -3
    assert lib.last_error().startswith("ccnet_ohemdsn:")
    n1 = lib.ccnet_ohemdsn_workspace_bytes(*shape, 1, 8)
    assert 0 < n1 < n
    # one head, optional outputs absent: the NULLs pass the checks
    assert fwd(p, None, p, 255, 0.7, 100000, 8, p, None, None, None, p, n1 - 1, *shape, 1, None) == -3


# ---------------------------------------------------------------------------------------------------------------------
# fixtures and oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_fixtures_cover_the_cases_and_match_no_other_suites_glob():
    names = D.fixture_names()
    assert set(names) == set(D.CASES) - set(D.ORACLE_ONLY) and D.ORACLE_ONLY == ("zoomed0",)
    for n in names:
        base = os.path.basename(D.fixture_path(n))
        assert base.startswith("ohemdsn_")
        assert not any(fnmatch.fnmatch(base, g) for g in ("ohem_*.npz", "dsn_*.npz", "eval_*.npz", "mseval_*.npz")), base
        assert os.path.getsize(D.fixture_path(n)) < (1 << 20)


def test_window_is_twice_the_largest_recorded_gap_and_the_fixtures_meet_its_conditions():
    gaps = {n: float(np.load(D.fixture_path(n))["p_target_gap"]) for n in D.fixture_names()}
    assert max(gaps.values()) <= D.MEASURED_P_GAP <= 1.001 * max(gaps.values()) and D.NEAR == 2 * D.MEASURED_P_GAP
    for n in D.fixture_names():
        z = np.load(D.fixture_path(n))
        assert float(z["threshold_gap"]) <= D.NEAR and int(z["pixels_in_window"]) <= D.MAX_NEAR, n
        # the reference's own fp32 error leaves the bar 4x headroom
        assert float(z["fp32_loss_rel_err"]) <= D.LOSS_RTOL / 4 and float(z["fp32_grad_rel_err"].max()) <= D.GRAD_RTOL / 4, n


@pytest.mark.parametrize("name", [n for n in D.CASES if n not in D.ORACLE_ONLY])
def test_oracle_reproduces_reference_fixture(name):
    fx = D.load_fixture(name)
    B, C, h, w, H, W = (int(v) for v in fx["shape"])
    sel = D.select(fx["logits"][0], fx["target"], **fx["args"])
    assert sel["threshold"] == fx["threshold"] and sel["num_valid"] == int(fx["num_valid_zoomed"])
    np.testing.assert_array_equal(sel["new_target"], fx["new_target"].astype(np.int64))
    loss, head_loss, grads = D.masked_loss(fx["logits"], fx["target"], fx["kept_mask"])
    r = {"threshold": sel["threshold"], "kept_mask": fx["kept_mask"], "kept": sel["kept"], "valid": int(fx["valid"]),
         "num_valid_zoomed": sel["num_valid"], "out_of_range": 0, "loss": loss, "head_loss": head_loss + [0.0],
         "grads": [g.astype(np.float32) for g in grads]}
    assert D.check_against_fixture(fx, r) == 0
    if not np.isnan(loss):
        assert abs(loss - float(fx["loss"])) <= 1e-12 * abs(loss)


def test_case_table_claims_hold_for_the_oracle_only_case():
    logits, target, args = D.case_inputs("zoomed0")
    sel = D.select(logits[0], target, **args)
    assert O.zoom_out_size(target.shape[1], 8) == 0 and sel["threshold"] == 1.0 and sel["num_valid"] == 0
    assert sel["kept"] == int((target != 255).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the public layer
# ---------------------------------------------------------------------------------------------------------------------
def test_public_layer_raises_on_cpu_tensors_bad_shapes_and_other_reductions():
    import torch
    from ccnet_amd import ohemdsn
    from ccnet_amd.ohem import CriterionOhemDSN as StockCriterionOhemDSN
    t = torch.zeros(1, 16, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ohemdsn.CriterionOhemDSN()([torch.randn(1, 19, 4, 4), torch.randn(1, 19, 4, 4)], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ohemdsn.UpsampledOhemCrossEntropy2d()(torch.randn(1, 19, 4, 4), t)
    for reduction in ("sum", "none", None):
        with pytest.raises(ValueError, match="reduction"):
            ohemdsn.CriterionOhemDSN(reduction=reduction)
    crit = ohemdsn.CriterionOhemDSN(ignore_index=255, thresh=0.6, min_kept=200000, use_weight=True, reduction="mean")
    assert crit.ignore_index == 255 and crit.thresh == 0.6 and crit.min_kept == 200000
    for attr in ("last_threshold", "last_kept", "last_num_valid", "last_num_out_of_range", "last_head_loss"):
        assert getattr(crit, attr) is None and getattr(ohemdsn.UpsampledOhemCrossEntropy2d(), attr) is None
    one = ohemdsn.UpsampledOhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=100000, factor=8)
    assert (one.ignore_label, one.thresh, one.min_kept, one.factor) == (255, 0.7, 100000, 8)
    assert not isinstance(crit, StockCriterionOhemDSN)                                  # the stock criterion is untouched
    assert type(StockCriterionOhemDSN().criterion2) is torch.nn.CrossEntropyLoss


def test_public_layer_raises_on_shape_mismatches_before_anything_else():
    import torch
    from ccnet_amd import ohemdsn
    t = torch.zeros(1, 16, 16, dtype=torch.long)
    x = torch.randn(1, 19, 4, 4)
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        ohemdsn.CriterionOhemDSN()([x, torch.randn(1, 19, 4, 5)], t)
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        ohemdsn.CriterionOhemDSN()([x, x], torch.zeros(2, 16, 16, dtype=torch.long))
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        ohemdsn.UpsampledOhemCrossEntropy2d()(x, t[0])
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        ohemdsn.UpsampledOhemCrossEntropy2d()(x[0], t)


def test_train_driver_accepts_fused_ohem_and_refuses_it_with_lovasz_and_fused_dsn():
    from ccnet_amd.train_synthetic import build_parser, parse_args, run
    assert build_parser().parse_args([]).fused_ohem is False
    a = parse_args(["--fused-ohem", "--ohem-thres", "0.7", "--ohem-keep", "100000"])
    assert a.fused_ohem and a.ohem and a.ohem_thres == 0.7 and a.ohem_keep == 100000 and not a.fused_dsn
    assert parse_args(["--fused-ohem", "--ohem"]).fused_ohem
    b = parse_args(["--ohem", "--fused-dsn"])
    assert b.ohem and b.fused_dsn and not b.fused_ohem                                   # ohem+dsn-fused keeps its meaning
    for other in ("--lovasz", "--fused-dsn"):
        with pytest.raises(SystemExit):
            parse_args(["--fused-ohem", other])
        with pytest.raises(ValueError, match=other):
            run(build_parser().parse_args(["--fused-ohem", other, "--cpu"]))
