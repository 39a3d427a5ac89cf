"""CPU checks of the DSN cross-entropy library (include/ccnet_dsn.h, ccnet_amd/csrc_dsn/): the shipped gfx950 library's surface,
its binding's refusals, the workspace cap, every argument check without a device, and the public layer's refusals."""
import ctypes
import os

import pytest

import dsn_oracle as D
import lib_checks as L
from conftest import ROOT

DSN_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_dsn")
RECIPE_B8 = (8, 19, 97, 97, 769, 769)


@pytest.fixture(scope="module")
def dsn_lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _dsn_lib
    return _dsn_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(dsn_lib_path):
    from ccnet_amd import _dsn_lib
    return _dsn_lib.DsnLibrary(dsn_lib_path)


def test_build_table_has_the_seventh_library():
    import __graft_entry__ as g
    assert [e.name for e in g.EXTENSIONS].count("dsn") == 1 and len(g.EXTENSIONS) == 7
    assert g.DSN_LIB.endswith(os.path.join("csrc_dsn", "libccnet_dsn.so"))


def test_library_exports_exactly_the_header(dsn_lib_path):
    from ccnet_amd import _dsn_lib
    names = _dsn_lib.declared_symbols()
    assert set(names) == set(_dsn_lib._PROTOTYPES) and len(names) == 6
    assert L.exported_symbols(dsn_lib_path) == names


def test_library_contains_gfx950_code(dsn_lib_path):
    blob = open(dsn_lib_path, "rb").read()
    assert b"gfx950" in blob and b"forward_kernel" in blob and b"backward_kernel" in blob and b"finalize_kernel" in blob


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(dsn_lib_path, tmp_path):
    kernels = L.code_object_kernels(dsn_lib_path, tmp_path, "_ZN3dsn")
    assert len(kernels) == 3, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_sources_carry_no_env_knobs_no_emulator_code_and_no_atomics():
    files = L.product_sources(DSN_CSRC)
    assert set(files) == {"dsn_api.hip", "dsn_kernels.hpp", "dsn_platform.hpp"}
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomicAdd" not in text and "lds_inc" not in text, f          # the backward is a gather


def test_binding_refuses_a_missing_library_and_another_abi_version(dsn_lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _dsn_lib as m
    from ccnet_amd._ohem_lib import OhemError
    assert issubclass(m.DsnError, RuntimeError) and not issubclass(m.DsnError, OhemError) and not issubclass(OhemError, m.DsnError)
    with pytest.raises(m.DsnError, match="not found"):
        m.DsnLibrary(str(tmp_path / "libccnet_missing.so"))
    assert m.DsnLibrary(m.LIB_PATH).path == m.LIB_PATH
    monkeypatch.setattr(m, "CCNET_DSN_VERSION", m.CCNET_DSN_VERSION + 1)
    with pytest.raises(m.DsnError, match="rebuild"):
        m.DsnLibrary(m.LIB_PATH)


@pytest.mark.parametrize("shape,heads", [(c[:6], c[7]) for c in D.CASES.values()] + [(RECIPE_B8, 2), (RECIPE_B8, 1)],
                         ids=list(D.CASES) + ["recipe_b8", "recipe_b8_one_head"])
def test_workspace_obeys_the_cap(lib, shape, heads):
    B, C, h, w, H, W = shape
    n = lib.ccnet_dsn_workspace_bytes(B, C, h, w, H, W, heads)
    assert 0 < n <= 16 * B * H * W + 65536, n
    assert n >= (4 * heads + 1) * B * H * W                  # a log-sum-exp per head and at least a byte of label per pixel
    assert n < B * C * H * W                                 # nothing logits-sized at full resolution (C >= 19 here)


BAD_SHAPES = [(0, 19, 13, 13, 97, 97, 2), (1, 0, 13, 13, 97, 97, 2), (1, 257, 13, 13, 97, 97, 2), (1, 19, 0, 13, 97, 97, 2),
              (1, 19, 13, 0, 97, 97, 2), (1, 19, 98, 13, 97, 97, 2), (1, 19, 13, 98, 97, 97, 2), (1, 19, 13, 13, 97, 97, 0),
              (1, 19, 13, 13, 97, 97, 3), (-1, 19, 13, 13, 97, 97, 2), (4, 19, 97, 97, 32768, 32768, 2),
              (1, 19, 1, 1, (1 << 20) + 1, 1, 1)]


@pytest.mark.parametrize("shape", BAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_of_contract_shapes_are_refused_without_a_device(lib, shape):
    assert lib.ccnet_dsn_workspace_bytes(*shape) == 0
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    assert lib.ccnet_dsn_forward_f32(p, p, p, 1.0, 0.4, p, p, p, p, 1 << 30, *shape, 255, None) == -1
    assert "unsupported shape" in lib.last_error() and lib.last_error().startswith("ccnet_dsn:")
    assert lib.ccnet_dsn_backward_f32(p, p, p, p, p, 1.0, 0.4, p, 1 << 30, *shape, None) == -1


def test_version_and_argument_validation_without_a_gpu(lib):
    assert lib.ccnet_dsn_version() == 100 and lib.ccnet_dsn_arch() == b"gfx950"
    assert lib.ccnet_dsn_workspace_bytes(1, 256, 97, 97, 97, 97, 2) > 0          # the bounds themselves are inside the contract
    shape = (2, 19, 13, 13, 97, 97)
    n = lib.ccnet_dsn_workspace_bytes(*shape, 2)
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    fwd = lambda *a: lib.ccnet_dsn_forward_f32(*a)                                # noqa: E731
    assert fwd(None, p, p, 1.0, 0.4, p, p, p, p, n, *shape, 2, 255, None) == -2
    assert fwd(p, None, p, 1.0, 0.4, p, p, p, p, n, *shape, 2, 255, None) == -2   # two heads need the second logits
    assert fwd(p, p, None, 1.0, 0.4, p, p, p, p, n, *shape, 2, 255, None) == -2
    assert fwd(p, p, p, 1.0, 0.4, None, p, p, p, n, *shape, 2, 255, None) == -2
    assert fwd(p, p, p, 1.0, 0.4, p, p, p, None, n, *shape, 2, 255, None) == -2
    assert "NULL" in lib.last_error()
    assert fwd(p, p, p, 1.0, 0.4, p, p, p, p, n - 1, *shape, 2, 255, None) == -3
    assert "workspace" in lib.last_error()
    bwd = lambda *a: lib.ccnet_dsn_backward_f32(*a)                               # noqa: E731
    assert bwd(None, p, p, p, p, 1.0, 0.4, p, n, *shape, 2, None) == -2
    assert bwd(p, None, p, p, p, 1.0, 0.4, p, n, *shape, 2, None) == -2
    assert bwd(p, p, None, p, p, 1.0, 0.4, p, n, *shape, 2, None) == -2
    assert bwd(p, p, p, None, p, 1.0, 0.4, p, n, *shape, 2, None) == -2
    assert bwd(p, p, p, p, None, 1.0, 0.4, p, n, *shape, 2, None) == -2
    assert bwd(p, p, p, p, p, 1.0, 0.4, None, n, *shape, 2, None) == -2
    assert bwd(p, p, p, p, p, 1.0, 0.4, p, 16, *shape, 2, None) == -3
    assert lib.last_error().startswith("ccnet_dsn:")
    n1 = lib.ccnet_dsn_workspace_bytes(*shape, 1)
    assert 0 < n1 < n
    assert fwd(p, None, p, 1.0, 0.0, p, None, None, p, n1 - 1, *shape, 1, 255, None) == -3   # one head: NULLs pass the checks


def test_public_layer_raises_on_cpu_tensors_and_other_reductions():
    import torch
    from ccnet_amd import dsn
    from ccnet_amd.ohem import CriterionOhemDSN
    t = torch.zeros(1, 16, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsn.CriterionDSN()([torch.randn(1, 19, 4, 4), torch.randn(1, 19, 4, 4)], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsn.CriterionDSN()([torch.randn(1, 19, 4, 4)], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsn.UpsampledCrossEntropy2d()(torch.randn(1, 19, 4, 4), t)
    for reduction in ("sum", "none", None):
        with pytest.raises(ValueError, match="reduction"):
            dsn.CriterionDSN(reduction=reduction)
        with pytest.raises(ValueError, match="reduction"):
            CriterionOhemDSN(reduction=reduction, fused_aux=True)
    crit = dsn.CriterionDSN(ignore_index=255, use_weight=True, reduction="mean")      # the reference's constructor
    assert crit.ignore_index == 255 and crit.last_num_valid is None and crit.last_num_out_of_range is None
    assert isinstance(CriterionOhemDSN(fused_aux=True).criterion2, dsn.UpsampledCrossEntropy2d)
    assert isinstance(CriterionOhemDSN().criterion2, torch.nn.CrossEntropyLoss)        # the default is untouched


def test_train_driver_refuses_fused_dsn_with_lovasz():
    from ccnet_amd.train_synthetic import build_parser, parse_args, run
    assert build_parser().parse_args([]).fused_dsn is False
    assert parse_args(["--fused-dsn"]).fused_dsn and parse_args(["--fused-dsn", "--ohem"]).ohem
    with pytest.raises(SystemExit):
        parse_args(["--fused-dsn", "--lovasz"])
    with pytest.raises(ValueError, match="--lovasz"):
        run(build_parser().parse_args(["--fused-dsn", "--lovasz", "--cpu"]))
