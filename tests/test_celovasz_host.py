"""CPU checks of the fused CE + Lovász criterion (include/ccnet_celovasz.h, ccnet_amd/csrc_lovasz/celovasz_*): its place in the
build table, the shipped gfx950 library's surface, its binding's refusals, the workspace bound, every argument check without a
device, the oracle against the reference fixtures, and the public layer's and the training driver's refusals."""
import ctypes
import fnmatch
import os

import numpy as np
import pytest

import celovasz_oracle as D
import lib_checks as L
from conftest import ROOT

RECIPE = (1, 19, 97, 97, 769, 769)
RECIPE_B8 = (8, 19, 97, 97, 769, 769)
CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_lovasz")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _celovasz_lib
    return _celovasz_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _celovasz_lib
    return _celovasz_lib.CeLovaszLibrary(lib_path)


@pytest.fixture(scope="module")
def lovasz_lib(lib_path):
    from ccnet_amd import _lovasz_lib
    return _lovasz_lib.LovaszLibrary(_lovasz_lib.LIB_PATH)


def test_build_table_keeps_its_rows_and_the_library_is_a_second_unit_of_the_lovasz_directory():
    import __graft_entry__ as g
    row = [e for e in g.EXTENSIONS if e.name == "lovasz"][0]
    assert [u.name for u in row.libraries()] == ["lovasz"]
    unit = [e for e in g.SECOND_UNITS if e.name == "celovasz"][0]
    rows = [u for e in g.EXTENSIONS for u in e.libraries()]          # (no count here: the earlier host tests pin the table's)
    assert g.all_libraries() == rows + g.SECOND_UNITS and unit not in rows
    dsn = os.path.join(ROOT, "ccnet_amd", "csrc_dsn")
    assert unit.csrc == row.csrc and unit.binding == "_celovasz_lib" and unit.exports.endswith("celovasz_exports.map")
    assert unit.unit.endswith(os.path.join("csrc_lovasz", "celovasz_api.hip")) and unit.header.endswith("ccnet_celovasz.h")
    assert g.CELOVASZ_LIB.endswith(os.path.join("csrc_lovasz", "libccnet_celovasz.so"))
    # the row's flags and one more include directory, which is this library's alone: on its include path and among its sources
    assert g.CELOVASZ_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(CSRC, "celovasz_exports.map"),
                                                      "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-I" + dsn]
    assert "-fvisibility=hidden" in g._BASE_FLAGS and "-I" + dsn not in g.LOVASZ_HIPCC_FLAGS
    assert os.path.join(dsn, "dsn_kernels.hpp") in unit.sources() and os.path.join(dsn, "dsn_kernels.hpp") not in row.sources()
    assert os.path.join(CSRC, "lovasz_launch.hpp") in unit.sources() and os.path.join(CSRC, "lovasz_launch.hpp") in row.sources()


def test_the_lovasz_librarys_build_line_is_the_parent_commits():
    import __graft_entry__ as g
    assert g.LOVASZ_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-I" + CSRC,
                                                    "-I" + os.path.join(ROOT, "include")]


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _celovasz_lib
    names = _celovasz_lib.declared_symbols()
    assert names == sorted(["ccnet_celovasz_version", "ccnet_celovasz_arch", "ccnet_celovasz_last_error",
                            "ccnet_celovasz_workspace_bytes", "ccnet_celovasz_forward_f32", "ccnet_celovasz_backward_f32"])
    assert set(names) == set(_celovasz_lib._PROTOTYPES)
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob
    for kernel in (b"_ZN8celovasz19pixel_errors_kernel", b"_ZN8celovasz15finalize_kernel", b"_ZN8celovasz16pixel_dot_kernel",
                   b"_ZN8celovasz15backward_kernel"):
        assert kernel in blob, kernel
    # the sort and the scans are libccnet_lovasz's own kernels, reused
    for kernel in (b"_ZN6lovasz20radix_scatter_kernel", b"_ZN6lovasz16scan_grad_kernel", b"_ZN6lovasz15finalize_kernel"):
        assert kernel in blob, kernel


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN8celovasz")
    assert len(kernels) == 4, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_sources_restate_neither_the_up_sample_nor_the_sort():
    files = L.product_sources(CSRC)
    assert {"celovasz_api.hip", "celovasz_kernels.hpp", "lovasz_launch.hpp", "lovasz_api.hip"} <= set(files)
    text = files["celovasz_kernels.hpp"]
    for name in ("axis_taps", "bilinear", "candidates", "pick3", "pixel_head"):
        assert "dsn::" + name in text and " " + name + "(" not in text.replace("dsn::" + name + "(", ""), name
    assert "floor(" not in text and "ballot" not in text and "kRadix" not in text and "jaccard" not in text
    for name in ("kKeyTop", "kInvalidKey", "kFgBit", "kUpBit", "kDownBit"):
        assert "lovasz::" + name in text and "constexpr uint32_t " + name not in text, name
    assert text.count("expf(") == 1                                              # p_c has one definition
    # both units launch the sort and the scans through the one shared sequence
    for unit in ("celovasz_api.hip", "lovasz_api.hip"):
        assert '#include "lovasz_launch.hpp"' in files[unit] and "lovasz::sort_scan_finalize(" in files[unit], unit
        assert "radix_hist_kernel" not in files[unit] and "scan_grad_kernel" not in files[unit], unit
    assert files["lovasz_launch.hpp"].count("radix_scatter_kernel") == 1
    for f in ("celovasz_api.hip", "celovasz_kernels.hpp"):
        assert "atomicAdd" not in files[f] and "lds_inc" not in files[f] and "hipMalloc" not in files[f], f
        assert "hipDeviceSynchronize" not in files[f] and "hipStreamSynchronize" not in files[f] and "getenv" not in files[f], f


def test_binding_refuses_a_missing_library_and_another_abi_version(lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _celovasz_lib as m
    from ccnet_amd._dsn_lib import DsnError
    from ccnet_amd._lovasz_lib import LovaszError
    assert issubclass(m.CeLovaszError, RuntimeError) and not issubclass(m.CeLovaszError, (LovaszError, DsnError))
    with pytest.raises(m.CeLovaszError, match="not found"):
        m.CeLovaszLibrary(str(tmp_path / "libccnet_missing.so"))
    assert m.CeLovaszLibrary(m.LIB_PATH).path == m.LIB_PATH
    monkeypatch.setattr(m, "CCNET_CELOVASZ_VERSION", m.CCNET_CELOVASZ_VERSION + 1)
    with pytest.raises(m.CeLovaszError, match="rebuild"):
        m.CeLovaszLibrary(m.LIB_PATH)


@pytest.mark.parametrize("per_image", [0, 1])
@pytest.mark.parametrize("shape", [c[:6] for c in D.CASES.values()] + [RECIPE, RECIPE_B8], ids=list(D.CASES) + ["recipe", "recipe_b8"])
def test_workspace_obeys_the_bound(lib, lovasz_lib, shape, per_image):
    B, C, h, w, H, W = shape
    n = lib.ccnet_celovasz_workspace_bytes(B, C, h, w, H, W, per_image)
    sort = lovasz_lib.ccnet_lovasz_workspace_bytes(B, C, H, W, per_image)
    assert sort > 0 and sort + 10 * B * H * W <= n <= sort + 12 * B * H * W + 65536, (n, sort)
    assert n % 256 == 0


BAD_SHAPES = [(0, 19, 13, 13, 97, 97, 0), (-1, 19, 13, 13, 97, 97, 0), (1, 1, 13, 13, 97, 97, 0), (1, 0, 13, 13, 97, 97, 0),
              (1, 257, 13, 13, 97, 97, 0), (1, 19, 0, 13, 97, 97, 0), (1, 19, 13, 0, 97, 97, 0), (1, 19, 98, 13, 97, 97, 0),
              (1, 19, 13, 98, 97, 97, 0), (1, 19, 97, 97, 4097, 4097, 1), (29, 19, 97, 97, 769, 769, 0),
              (1, 19, 1, 1, (1 << 20) + 1, 1, 0), (32768, 2, 1, 1, 1, 1, 0), (4000, 19, 1, 1, 2, 2, 1)]


@pytest.mark.parametrize("shape", BAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_of_contract_shapes_are_refused_without_a_device(lib, shape):
    assert lib.ccnet_celovasz_workspace_bytes(*shape) == 0
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    geometry, per_image = shape[:6], shape[6]
    assert lib.ccnet_celovasz_forward_f32(p, p, 255, per_image, 1, None, p, p, p, p, 1 << 40, *geometry, None) == -1
    assert "unsupported shape" in lib.last_error() and lib.last_error().startswith("ccnet_celovasz:")
    assert lib.ccnet_celovasz_backward_f32(p, p, p, p, 1 << 40, *geometry, per_image, None) == -1


def test_version_and_argument_validation_without_a_gpu(lib):
    assert lib.ccnet_celovasz_version() == 100 and lib.ccnet_celovasz_arch() == b"gfx950"
    assert lib.ccnet_celovasz_workspace_bytes(1, 256, 97, 97, 97, 97, 0) > 0       # the bounds themselves are inside the contract
    assert lib.ccnet_celovasz_workspace_bytes(1, 2, 1, 1, 1, 1, 1) > 0
    assert lib.ccnet_celovasz_workspace_bytes(29, 19, 97, 97, 769, 769, 1) > 0     # 29 x 769^2 > 2^24, fine per image
    shape = (2, 19, 13, 13, 97, 97)
    n = lib.ccnet_celovasz_workspace_bytes(*shape, 0)
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    fwd = lambda *a: lib.ccnet_celovasz_forward_f32(*a)                            # noqa: E731
    assert fwd(None, p, 255, 0, 1, None, p, p, p, p, n, *shape, None) == -2
    assert fwd(p, None, 255, 0, 1, None, p, p, p, p, n, *shape, None) == -2
    assert fwd(p, p, 255, 0, 1, None, None, p, p, p, n, *shape, None) == -2
    assert fwd(p, p, 255, 0, 1, None, p, p, p, None, n, *shape, None) == -2
    assert "NULL" in lib.last_error()
    assert fwd(p, p, 255, 0, 1, None, p, p, p, p, n - 1, *shape, None) == -3
    assert "workspace" in lib.last_error()
    assert fwd(p, p, 255, 0, 1, None, p, None, None, p, n - 1, *shape, None) == -3   # optional outputs absent: the NULLs pass
    bwd = lambda *a: lib.ccnet_celovasz_backward_f32(*a)                           # noqa: E731
    assert bwd(None, p, p, p, n, *shape, 0, None) == -2
    assert bwd(p, None, p, p, n, *shape, 0, None) == -2
    assert bwd(p, p, None, p, n, *shape, 0, None) == -2
    assert bwd(p, p, p, None, n, *shape, 0, None) == -2
    assert bwd(p, p, p, p, 16, *shape, 0, None) == -3
    assert lib.last_error().startswith("ccnet_celovasz:")
    # per image the sort workspace is the same size here (same element count), the layout differs: both are accepted sizes
    assert lib.ccnet_celovasz_workspace_bytes(*shape, 1) > 0


# ---------------------------------------------------------------------------------------------------------------------
# fixtures and oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_fixtures_cover_the_cases_and_match_no_other_suites_glob():
    names = D.fixture_names()
    assert set(names) == set(D.CASES) - set(D.ORACLE_ONLY) and set(D.ORACLE_ONLY) == {"out_of_range", "ignored"}
    for n in names:
        base = os.path.basename(D.fixture_path(n))
        assert base.startswith("celovasz_")
        assert not any(fnmatch.fnmatch(base, g) for g in ("lovasz_*.npz", "ohem_*.npz", "dsn_*.npz", "ohemdsn_*.npz")), base
        assert os.path.getsize(D.fixture_path(n)) < (1 << 20)
    assert os.path.exists(D.RECIPE_FIXTURE)


def test_cases_have_three_sort_tiles_a_segment_and_the_fp32_reference_leaves_the_bars_4x_headroom():
    for name, (B, C, h, w, H, W, *_rest) in D.CASES.items():
        if name != "one":
            assert B * H * W > 2 * 2048 and H * W > 2 * 2048, name      # lovasz::kTile = 2048 positions
    for n in D.fixture_names():
        z = np.load(D.fixture_path(n))
        assert float(z["fp32_loss_rel_err"]) <= D.LOSS_RTOL / 4 and float(z["fp32_grad_rel_err"]) <= D.GRAD_RTOL / 4, n


@pytest.mark.parametrize("name", [n for n in D.CASES if n not in D.ORACLE_ONLY])
def test_oracle_reproduces_reference_fixture(name):
    """the restatement in fp32 against the reference's own fp32 run: the same stock ops, the Lovász term with a stable sort"""
    fx = D.load_fixture(name)
    ref = D.reference(fx["logits"], fx["target"])
    D.check_against_fixture(fx, dict(ref, grad=ref["grad"].astype(np.float32)))
    assert abs(ref["head_loss"][0] - float(fx["head_loss"][0])) <= 1e-6 * abs(ref["head_loss"][0])
    ce64, _ = D.stock_cross_entropy(fx["logits"], fx["target"])                        # dsn_oracle's float64 restatement of the CE
    assert abs(ce64 - float(fx["head_loss"][0])) <= D.LOSS_RTOL / 4 * abs(ce64)
    if name == "absent":
        assert ref["n_kept"] == 5


def test_oracle_only_cases_are_what_the_table_says():
    logits, target = D.case_inputs("out_of_range")
    ref = D.reference(logits, target)
    assert ref["out_of_range"] > 7 and ref["valid"] == int(((target >= 0) & (target < 19)).sum())
    logits, target = D.case_inputs("ignored")
    ref = D.reference(logits, target)
    assert ref["valid"] == 0 and np.isnan(ref["loss"]) and not ref["grad"].any()


# ---------------------------------------------------------------------------------------------------------------------
# the public layer
# ---------------------------------------------------------------------------------------------------------------------
def test_public_layer_raises_on_cpu_tensors_bad_shapes_and_other_reductions():
    import torch
    import ccnet_amd
    from ccnet_amd import celovasz
    from ccnet_amd.lovasz import CriterionOhemDSN2 as StockCriterionOhemDSN2
    assert ccnet_amd.celovasz is celovasz and ccnet_amd.UpsampledCELovasz is celovasz.UpsampledCELovasz
    assert ccnet_amd.CriterionOhemDSN2 is StockCriterionOhemDSN2                         # the stock criterion keeps its name
    t = torch.zeros(1, 16, 16, dtype=torch.long)
    x = torch.randn(1, 19, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        celovasz.CriterionOhemDSN2()([x, x], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        celovasz.UpsampledCELovasz()(x, t)
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        celovasz.UpsampledCELovasz()(x, t[0])
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        celovasz.UpsampledCELovasz()(x[0], t)
    with pytest.raises(RuntimeError, match=r"expected logits \(B, C, h, w\)"):
        celovasz.UpsampledCELovasz()(x, torch.zeros(2, 16, 16, dtype=torch.long))
    for reduction in ("sum", "none", None):
        with pytest.raises(ValueError, match="reduction"):
            celovasz.CriterionOhemDSN2(reduction=reduction)
    crit = celovasz.CriterionOhemDSN2(ignore_index=250, thresh=0.6, min_kept=200000, use_weight=True, reduction="mean")
    assert crit.ignore_index == 250 and crit.criterion.ignore_index == 250
    assert crit.criterion.classes == "present" and crit.criterion.per_image is False
    one = celovasz.UpsampledCELovasz(ignore_index=255, classes=[1, 2, 2], per_image=True)
    assert (one.ignore_index, one.classes, one.per_image) == (255, [1, 2, 2], True)
    for attr in ("last_head_loss", "last_num_valid", "last_num_out_of_range", "last_n_kept"):
        assert getattr(one, attr) is None
    assert not isinstance(crit, StockCriterionOhemDSN2)
    assert type(StockCriterionOhemDSN2().criterion) is torch.nn.CrossEntropyLoss         # the stock criterion is untouched


def test_train_driver_accepts_fused_lovasz_and_refuses_it_with_the_other_criteria():
    from ccnet_amd.train_synthetic import build_parser, parse_args, run
    assert build_parser().parse_args([]).fused_lovasz is False
    a = parse_args(["--fused-lovasz"])
    assert a.fused_lovasz and a.lovasz and not a.ohem and not a.fused_dsn and not a.fused_ohem
    assert parse_args(["--fused-lovasz", "--lovasz"]).fused_lovasz
    b = parse_args(["--lovasz"])
    assert b.lovasz and not b.fused_lovasz                                               # --lovasz keeps its meaning
    for other in ("--ohem", "--fused-dsn", "--fused-ohem"):
        with pytest.raises(SystemExit):
            parse_args(["--fused-lovasz", other])
        with pytest.raises(ValueError, match="--fused-lovasz cannot be combined with " + other):
            run(build_parser().parse_args(["--fused-lovasz", other, "--cpu"]))
