"""CPU checks of the Lovász-softmax loss (include/ccnet_lovasz.h, ccnet_amd/csrc_lovasz/): the numpy oracle against the
reference fixtures, the shipped gfx950 library's surface, the Python front end's input handling, and the kernel sources
themselves run in the SIMT emulator (tests/emu/ + the Lovász primitives of tests/emu_lovasz/) against the oracle."""
import ctypes
import glob
import os

import numpy as np
import pytest

import lib_checks as L
import lovasz_oracle as O
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "lovasz_[0-9]*.npz")))
CRITERION_FIXTURE = os.path.join(GOLDEN, "lovasz_criterion_1x19x97x97_769.npz")
LOVASZ_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_lovasz")
TILE = 2048                     # lovasz::kTile: sorted positions per workgroup of every sort and scan pass


def _id(path):
    return os.path.basename(path)[:-4]


def test_fixtures_cover_the_issue_cases():
    names = {_id(f) for f in FIXTURES}
    assert {"lovasz_2x19x65x97_present", "lovasz_2x19x97x97_per_image", "lovasz_1x19x64x64_all_absent",
            "lovasz_1x19x60x70_list_dup", "lovasz_1x19x48x48_ignore_none", "lovasz_1x19x50x80_extra_labels",
            "lovasz_1x150x40x40_c150", "lovasz_2x19x33x129_nonsquare", "lovasz_1x19x769x769_recipe"} <= names
    assert os.path.exists(CRITERION_FIXTURE)


@pytest.mark.parametrize("path", FIXTURES, ids=_id)
def test_oracle_reproduces_reference_fixture(path):
    fx = O.load_fixture(path)
    o = O.lovasz_softmax(fx["probas"], fx["labels"], **fx["args"])
    singles, groups = O.check_against_fixture(fx, o["loss"], o["grad"], rtol=1e-6, gtol=1e-6)
    assert singles > 0 and groups == len(fx["group_key"])


def test_oracle_criterion_composition_reproduces_reference_fixture():
    import torch
    import torch.nn.functional as F
    z = np.load(CRITERION_FIXTURE)
    main, _, target = O.make_criterion_inputs(int(z["seed"]))
    x = torch.from_numpy(main).requires_grad_(True)
    up = F.interpolate(x, size=(769, 769), mode="bilinear", align_corners=True)
    t = torch.from_numpy(target)
    ce = F.cross_entropy(up, t, ignore_index=255)
    prob = F.softmax(up, dim=1)
    o = O.lovasz_softmax(prob.detach().numpy(), target, ignore=255)
    (ce + (prob * torch.from_numpy(o["grad"])).sum()).backward()
    loss = float(ce.detach()) + o["loss"]
    assert abs(loss - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
    g = x.grad.numpy().ravel()[z["grad_index"]]
    assert np.abs(g - z["grad_sample"]).max() <= 1e-5 * float(z["grad_absmax"])
    assert bool(z["aux_grad_is_none"])


def test_tie_groups_are_common_at_the_recipe_shape():
    fx = O.load_fixture(os.path.join(GOLDEN, "lovasz_1x19x769x769_recipe.npz"))
    assert int(fx["n_groups_multi"]) > 10000 and len(fx["group_key"]) == O.GROUP_SAMPLE


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lovasz_lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _lovasz_lib
    return _lovasz_lib.LIB_PATH


def test_library_exports_exactly_the_header(lovasz_lib_path):
    from ccnet_amd import _lovasz_lib
    names = _lovasz_lib.declared_symbols()
    assert set(names) == set(_lovasz_lib._PROTOTYPES) and len(names) == 6
    assert L.exported_symbols(lovasz_lib_path) == names


def test_library_contains_gfx950_code(lovasz_lib_path):
    blob = open(lovasz_lib_path, "rb").read()
    assert b"gfx950" in blob and b"radix_scatter_kernel" in blob and b"scan_grad_kernel" in blob


def test_version_and_argument_validation_without_a_gpu(lovasz_lib_path):
    from ccnet_amd import _lovasz_lib
    lib = _lovasz_lib.LovaszLibrary(lovasz_lib_path)
    assert lib.ccnet_lovasz_version() == 100 and lib.ccnet_lovasz_arch() == b"gfx950"
    assert lib.ccnet_lovasz_workspace_bytes(0, 19, 97, 97, 0) == 0
    assert lib.ccnet_lovasz_workspace_bytes(1, 1, 97, 97, 0) == 0                    # C = 1: the sigmoid form
    assert lib.ccnet_lovasz_workspace_bytes(1, 257, 97, 97, 0) == 0
    assert lib.ccnet_lovasz_workspace_bytes(1, 19, 4097, 4097, 1) == 0                # a segment above 2^24 pixels
    assert lib.ccnet_lovasz_workspace_bytes(29, 19, 769, 769, 0) == 0                 # 29 x 769^2 > 2^24 ...
    assert lib.ccnet_lovasz_workspace_bytes(29, 19, 769, 769, 1) > 0                  # ... fine per image
    n = lib.ccnet_lovasz_workspace_bytes(1, 19, 769, 769, 0)
    assert 20 * 19 * 769 * 769 <= n <= 21 * 19 * 769 * 769                            # about 20.5 B per pixel and class
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    fwd = lib.ccnet_lovasz_forward_f32
    assert fwd(p, p, p, None, p, n, 1, 1, 769, 769, 255, 0, 0, 1, None, None) == -1
    assert fwd(p, p, p, None, p, n, 29, 19, 769, 769, 255, 0, 0, 1, None, None) == -1
    assert fwd(None, p, p, None, p, n, 1, 19, 769, 769, 255, 0, 0, 1, None, None) == -2
    assert fwd(p, p, None, None, p, n, 1, 19, 769, 769, 255, 0, 0, 1, None, None) == -2
    assert fwd(p, p, p, None, p, n - 1, 1, 19, 769, 769, 255, 0, 0, 1, None, None) == -3
    assert "workspace" in lib.last_error()
    bwd = lib.ccnet_lovasz_backward_f32
    assert bwd(p, None, p, n, 1, 19, 769, 769, 0, None) == -2
    assert bwd(p, p, p, n, 1, 19, 769, 0, 0, None) == -1
    assert bwd(p, p, p, 16, 1, 19, 769, 769, 0, None) == -3
    assert lib.last_error().startswith("ccnet_lovasz:")


def test_class_selection_argument():
    from ccnet_amd._lovasz_lib import class_selection
    assert class_selection("present", 19) == (True, None)
    assert class_selection("all", 19) == (False, None)
    po, w = class_selection([1, 3, 3], 5)
    assert not po and list(w) == [0, 1, 0, 2, 0]
    with pytest.raises(ValueError):
        class_selection([5], 5)
    with pytest.raises(ValueError):
        class_selection("some", 5)


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(lovasz_lib_path, tmp_path):
    kernels = L.code_object_kernels(lovasz_lib_path, tmp_path, "_ZN6lovasz")
    assert len(kernels) == 9, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_sources_carry_no_env_knobs_no_emulator_code_and_no_float_atomics():
    files = L.product_sources(LOVASZ_CSRC, L.COMMON_CSRC)
    assert "lovasz_api.hip" in files and "ccnet_device.hpp" in files and "ccnet_host.hpp" in files
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "__fdividef" not in text and "fast-math" not in text and "hipDeviceSynchronize" not in text, f
        assert "hipStreamSynchronize" not in text and "hipMemcpy" not in text, f
    platform = files["lovasz_platform.hpp"] + files["ccnet_device.hpp"]             # its own primitives + the shared ones
    assert platform.count("atomicAdd(") == 1 and "atomicAdd(p, 1u)" in platform       # the LDS integer increment only


def test_cpu_input_and_unsupported_forms_raise():
    import torch
    from ccnet_amd import CriterionOhemDSN2, LovaszSoftmax, lovasz_softmax
    p = torch.softmax(torch.randn(1, 19, 8, 8), 1)
    lab = torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lovasz_softmax(p, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LovaszSoftmax(ignore=255)(p, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CriterionOhemDSN2()([torch.randn(1, 19, 4, 4), torch.randn(1, 19, 4, 4)], torch.zeros(1, 16, 16, dtype=torch.long))
    with pytest.raises(ValueError, match="sigmoid"):
        lovasz_softmax(torch.rand(1, 8, 8), lab)
    with pytest.raises(ValueError, match="sigmoid"):
        lovasz_softmax(torch.rand(1, 1, 8, 8), lab)


def test_train_driver_flags():
    from ccnet_amd.train_synthetic import build_parser
    assert build_parser().parse_args([]).lovasz is False
    a = build_parser().parse_args(["--lovasz"])
    assert a.lovasz and not a.ohem
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--lovasz", "--ohem"])


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._lovasz_lib import LovaszLibrary
    return LovaszLibrary(L.build_shared_scaffold_emu("lovasz"))


def emu_lovasz(lib, probas, labels, classes="present", per_image=False, ignore=None, grad_out=1.0):
    """forward + backward through the emulated C ABI with numpy buffers standing in for device memory."""
    from ccnet_amd._lovasz_lib import class_selection
    B, C, H, W = probas.shape
    probas = np.ascontiguousarray(probas, np.float32)
    labels = np.ascontiguousarray(labels, np.int64)
    n = lib.ccnet_lovasz_workspace_bytes(B, C, H, W, int(per_image))
    ws = np.full(n // 4 + 1, np.nan, np.float32)
    loss = np.full(1, np.nan, np.float32)
    kept = np.full(1, -7, np.int32)
    present_only, weights = class_selection(classes, C)
    lib.check(lib.ccnet_lovasz_forward_f32(probas.ctypes.data, labels.ctypes.data, loss.ctypes.data, kept.ctypes.data,
                                           ws.ctypes.data, n, B, C, H, W, 0 if ignore is None else ignore, int(ignore is None),
                                           int(per_image), int(present_only),
                                           None if weights is None else ctypes.addressof(weights), None), "forward")
    g = np.full(1, grad_out, np.float32)
    grad = np.full_like(probas, np.nan)
    lib.check(lib.ccnet_lovasz_backward_f32(g.ctypes.data, grad.ctypes.data, ws.ctypes.data, n, B, C, H, W, int(per_image),
                                            None), "backward")
    return {"loss": float(loss[0]), "n_kept": int(kept[0]), "grad": grad}


def check_emulated(r, o):
    """The emulator bar: loss within 1e-6 relative, the gradient within 2 ulp (the tie order is the oracle's)."""
    assert r["n_kept"] == o["n_kept"]
    assert abs(r["loss"] - o["loss"]) <= 1e-6 * abs(o["loss"]) or r["loss"] == o["loss"] == 0, (r["loss"], o["loss"])
    assert int(O.ulp_distance(r["grad"], o["grad"]).max()) <= 2


# every segment spans at least three tiles, so each sort and scan pass runs three or more workgroups per segment
EMU_CASES = {
    "present": (dict(B=1, C=5, H=50, W=90), dict(ignore=255)),
    "per_image": (dict(B=2, C=4, H=48, W=90), dict(per_image=True, ignore=255)),
    "all_absent": (dict(B=1, C=4, H=70, W=70, absent=2), dict(classes="all", ignore=255)),
    "list_dup": (dict(B=1, C=5, H=70, W=70, absent=4), dict(classes=[0, 2, 2, 4], ignore=255)),
    "ignore_none_extra": (dict(B=1, C=3, H=64, W=80, extra_frac=0.1), dict(ignore=None)),
    "batch_nonsquare": (dict(B=3, C=3, H=29, W=61), dict(ignore=255)),
}


@pytest.mark.parametrize("name", sorted(EMU_CASES))
def test_emulated_kernels_match_oracle(emu, name):
    shape, args = EMU_CASES[name]
    shape = dict(shape)
    B, C, H, W = (shape.pop(k) for k in ("B", "C", "H", "W"))
    seg = H * W if args.get("per_image") else B * H * W
    assert seg > 2 * TILE
    probas, labels = O.make_case_inputs(B, C, H, W, seed=B * 1000 + H * W + C, **shape)
    # quantise some probabilities so that equal errors (ties) are plentiful
    probas[..., ::3] = np.round(probas[..., ::3] * 64) / 64
    check_emulated(emu_lovasz(emu, probas, labels, **args), O.lovasz_softmax(probas, labels, **args))


@pytest.mark.parametrize("path", [f for f in FIXTURES if "769x769" not in f and "c150" not in f], ids=_id)
def test_emulated_kernels_match_reference_fixture(emu, path):
    fx = O.load_fixture(path)
    r = emu_lovasz(emu, fx["probas"], fx["labels"], **fx["args"])
    O.check_against_fixture(fx, r["loss"], r["grad"], rtol=1e-6, gtol=1e-6)


def test_emulated_tie_order_is_stable_pixel_order(emu):
    """Every probability equal: one tie group per class, so the sorted order is the pixel order and g follows it."""
    B, C, H, W = 1, 3, 64, 70
    probas = np.full((B, C, H, W), 1 / 3, np.float32)
    labels = np.random.default_rng(5).integers(0, C, (B, H, W)).astype(np.int64)
    r = emu_lovasz(emu, probas, labels, ignore=255)
    o = O.lovasz_softmax(probas, labels, ignore=255)
    check_emulated(r, o)
    assert np.array_equal(r["grad"], o["grad"])


def test_emulated_no_valid_pixel_and_one_valid_pixel(emu):
    probas, labels = O.make_case_inputs(1, 4, 50, 90, seed=17)
    none = np.full_like(labels, 255)
    r = emu_lovasz(emu, probas, none, ignore=255)
    assert r["loss"] == 0.0 and r["n_kept"] == 0 and np.all(r["grad"] == 0)
    r = emu_lovasz(emu, probas, none, classes="all", per_image=True, ignore=255)
    assert r["loss"] == 0.0 and np.all(r["grad"] == 0)
    one = none.copy()
    one[0, 20, 33] = 2
    r = emu_lovasz(emu, probas, one, ignore=255)
    o = O.lovasz_softmax(probas, one, ignore=255)
    check_emulated(r, o)
    assert r["n_kept"] == 1 and np.count_nonzero(r["grad"]) == 1


def test_emulated_per_image_with_an_empty_image(emu):
    probas, labels = O.make_case_inputs(2, 3, 48, 90, seed=23)
    labels[1] = 255
    args = dict(per_image=True, ignore=255)
    r = emu_lovasz(emu, probas, labels, **args)
    o = O.lovasz_softmax(probas, labels, **args)
    check_emulated(r, o)
    assert np.all(r["grad"][1] == 0) and r["n_kept"] == 3


def test_emulated_gradient_scales_with_grad_out_and_repeats_bitwise(emu):
    probas, labels = O.make_case_inputs(1, 4, 50, 90, seed=29)
    a = emu_lovasz(emu, probas, labels, ignore=255)
    b = emu_lovasz(emu, probas, labels, ignore=255)
    c = emu_lovasz(emu, probas, labels, ignore=255, grad_out=0.5)
    assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"])
    np.testing.assert_array_equal(c["grad"], 0.5 * a["grad"])


def test_emulated_exact_zero_negative_zero_and_one_probabilities(emu):
    """Where e = |fg - p| = 0 the sign of d e / d p is 0, so the gradient is exactly 0 (+0 and -0 compare equal)."""
    probas, labels = O.make_case_inputs(1, 4, 50, 90, seed=31)
    pick = np.random.default_rng(32).random(probas.shape)
    fg = labels[:, None] == np.arange(4)[None, :, None, None]
    probas[pick < 0.1] = 0.0
    probas[(pick >= 0.1) & (pick < 0.2)] = -0.0
    probas[fg & (pick >= 0.2) & (pick < 0.6)] = 1.0
    r = emu_lovasz(emu, probas, labels, ignore=255)
    o = O.lovasz_softmax(probas, labels, ignore=255)
    assert r["n_kept"] == o["n_kept"] and abs(r["loss"] - o["loss"]) <= 1e-6 * abs(o["loss"])
    assert int(O.ulp_distance(r["grad"] + np.float32(0), o["grad"] + np.float32(0)).max()) <= 2
    zero_e = (np.abs(fg.astype(np.float32) - probas) == 0) & (labels != 255)[:, None]
    assert zero_e.sum() > 1000 and not r["grad"][zero_e].any()


@pytest.mark.parametrize("C,ignore", [(2, 255), (256, None)], ids=["c2", "c256_all_labels"])
@pytest.mark.parametrize("per_image", [False, True], ids=["plain", "per_image"])
def test_emulated_class_count_limits(emu, C, ignore, per_image):
    H, W = (48, 90) if C == 2 else (8, 16)
    probas, labels = O.make_case_inputs(2, C, H, W, seed=33 + C)
    args = dict(per_image=per_image, ignore=ignore)
    check_emulated(emu_lovasz(emu, probas, labels, **args), O.lovasz_softmax(probas, labels, **args))
