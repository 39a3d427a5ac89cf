"""CPU checks of the device ABN (include/ccnet_abn.h, ccnet_amd/csrc_abn/): the shipped gfx950 library's surface, the Python
front end's input handling, and the kernel sources themselves run in the SIMT emulator (tests/emu/ + the ABN primitives of
tests/emu_abn/) against the float64 oracle of tests/abn_oracle.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import abn_cases as K
import abn_oracle as O
import lib_checks as L
from conftest import ROOT

ABN_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_abn")


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abn_lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _abn_lib
    return _abn_lib.LIB_PATH


def test_library_exports_exactly_the_header(abn_lib_path):
    from ccnet_amd import _abn_lib
    names = _abn_lib.declared_symbols()
    assert set(names) == set(_abn_lib._PROTOTYPES) and len(names) == 9
    assert L.exported_symbols(abn_lib_path) == names


def test_library_contains_gfx950_code(abn_lib_path):
    blob = open(abn_lib_path, "rb").read()
    assert b"gfx950" in blob and b"stats_partial_kernel" in blob and b"backward_apply_kernel" in blob


def test_header_constants_match_the_binding():
    from ccnet_amd import _abn_lib
    text = open(_abn_lib.HEADER_PATH).read()
    consts = dict(re.findall(r"#define (CCNET_ABN_\w+) (\d+)", text))
    for name, value in consts.items():
        assert getattr(_abn_lib, name) == int(value), name
    assert len(consts) == 11
    fields = re.search(r"typedef struct ccnet_abn_desc \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f for f, _ in _abn_lib.AbnDesc._fields_]


def _desc(dtype=0, N=1, C=64, H=97, W=97, act=0, p=0.01, gm=0, eps=1e-5):
    from ccnet_amd._abn_lib import make_desc
    return make_desc(dtype, N, C, H, W, act, p, gm, eps)


def test_version_and_argument_validation_without_a_gpu(abn_lib_path):
    from ccnet_amd import _abn_lib
    lib = _abn_lib.AbnLibrary(abn_lib_path)
    assert lib.ccnet_abn_version() == 100 and lib.ccnet_abn_arch() == b"gfx950"
    ws = lib.ccnet_abn_workspace_bytes
    assert ws(None) == 0
    assert ws(ctypes.byref(_desc(N=0))) == 0
    assert ws(ctypes.byref(_desc(dtype=2))) == 0
    assert ws(ctypes.byref(_desc(act=4))) == 0
    assert ws(ctypes.byref(_desc(act=2, p=-0.1))) == 0                       # leaky slope below 0
    assert ws(ctypes.byref(_desc(act=3, p=0.0))) == 0                        # elu alpha 0
    assert ws(ctypes.byref(_desc(gm=1, eps=0.0))) == 0                       # |w| + 0 is not invertible
    assert ws(ctypes.byref(_desc(H=1 << 16, W=1 << 15))) == 0                # a plane of 2^31 elements
    # the stem's 64 channels x 148 k pixels: 19 splits of at least 8192 elements per channel, 16 bytes each
    assert ws(ctypes.byref(_desc(N=1, C=64, H=385, W=385))) == 64 * 19 * 16
    assert ws(ctypes.byref(_desc(N=8, C=64, H=385, W=385))) == 64 * 32 * 16   # 2048 workgroups
    assert ws(ctypes.byref(_desc(N=1, C=2048, H=97, W=97))) == 2048 * 16    # layer 4: one workgroup per channel
    assert ws(ctypes.byref(_desc(N=1, C=1, H=1, W=2))) == 16
    one = ctypes.c_double(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    d = ctypes.byref(_desc())
    n = ws(d)
    assert lib.ccnet_abn_stats(d, None, p, p, n, None) == -2
    assert lib.ccnet_abn_stats(d, p, p, p, n - 1, None) == -3
    assert "workspace" in lib.last_error()
    assert lib.ccnet_abn_stats(ctypes.byref(_desc(C=0)), p, p, p, n, None) == -1
    assert lib.ccnet_abn_stats_combine(d, p, 0, 0.1, None, None, p, None) == -1
    assert lib.ccnet_abn_stats_combine(d, None, 1, 0.1, None, None, p, None) == -2
    assert lib.ccnet_abn_forward(d, p, None, None, p, None, None, None, None, None) == -2
    assert lib.ccnet_abn_forward(d, p, None, p, None, None, None, None, None, None) == -2     # eval without running stats
    relu = ctypes.byref(_desc(act=1))
    red, app = lib.ccnet_abn_backward_reduce, lib.ccnet_abn_backward_apply
    assert red(relu, 1, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -1   # relu from y
    assert "relu" in lib.last_error()
    assert red(ctypes.byref(_desc(act=2, p=0.0)), 1, p, None, p, None, p, None, None, None, None, p, None, None, p, n,
               None) == -1
    assert red(d, 2, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -1      # bad source
    assert red(relu, 0, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -2   # act' needs y
    assert red(d, 0, p, None, p, None, p, None, None, None, None, p, None, None, p, 8, None) == -3
    assert app(d, 0, p, None, p, None, p, None, None, None, None, None, 1, p, None, None) == -2         # no sums
    assert app(d, 0, p, None, p, None, p, None, None, None, None, p, 1, p, None, None) == -1            # dx aliases dy
    assert lib.last_error().startswith("ccnet_abn:")


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(abn_lib_path, tmp_path):
    kernels = L.code_object_kernels(abn_lib_path, tmp_path, "_ZN3abn")
    assert len(kernels) == 12, sorted(kernels)              # 5 templates x 2 dtypes + 2 per-channel kernels
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_sources_carry_no_env_knobs_no_emulator_code_and_no_float_atomics():
    files = L.product_sources(ABN_CSRC)
    assert sorted(files) == ["abn_api.hip", "abn_kernels.hpp", "abn_platform.hpp"]
    # of the shared device primitives the ABN sources take the wave size, the lane id and the sum only (not the LDS counter)
    assert sorted(re.findall(r"ccnet_common::(\w+)", "".join(files.values()))) == ["kWave", "lane_id", "wave_sum"]
    common = L.product_sources(L.COMMON_CSRC)
    assert sorted(common) == ["ccnet_device.hpp", "ccnet_host.hpp"]
    for f, text in {**files, **common}.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        if f == "ccnet_device.hpp":                 # (the shared header's LDS integer increment, which ABN does not take)
            text = text.replace("atomicAdd(p, 1u)", "", 1)
        assert "atomic" not in text.lower(), f
        assert "__fdividef" not in text and "fast-math" not in text and "hipDeviceSynchronize" not in text, f
        assert "hipStreamSynchronize" not in text and "hipMemcpy" not in text, f
    py = open(os.path.join(ROOT, "ccnet_amd", "abn.py")).read() + open(os.path.join(ROOT, "ccnet_amd", "_abn_lib.py")).read()
    assert "environ" not in py and "getenv" not in py


# ---------------------------------------------------------------------------------------------------------------------
# the Python front end without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_cpu_input_and_unsupported_forms_raise():
    import torch
    from ccnet_amd.abn import ABN, InPlaceABN, InPlaceABNSync
    x = torch.randn(2, 4, 5, 5)
    for cls in (ABN, InPlaceABN, InPlaceABNSync):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(4)(x.clone())
    with pytest.raises(ValueError, match="relu"):
        InPlaceABN(4, activation="relu")(x.clone())
    with pytest.raises(ValueError, match="momentum"):
        ABN(4, momentum=None)(x)


def test_convert_abn_keeps_parameters_buffers_and_state_dict_keys():
    import torch
    import inplace_abn
    from ccnet_amd import abn
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2)
    for m in model.modules():
        if isinstance(m, inplace_abn.ABN):
            with torch.no_grad():
                m.weight.uniform_(-1, 1)
                m.running_var.uniform_(0.5, 2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = {id(p) for p in model.parameters()}
    stock = sum(isinstance(m, inplace_abn.ABN) for m in model.modules())
    assert stock == 110                # stem 3, residual units 3 x 33 + 4 downsample, RCCA head 3, DSN 1
    for mode, inplace in (("device", False), ("inplace", True), ("device", False)):
        abn.convert_abn(model, mode)
        dev = [m for m in model.modules() if isinstance(m, inplace_abn.ABN)]
        assert len(dev) == stock and all(type(m) in (abn.ABN, abn.InPlaceABN, abn.InPlaceABNSync) for m in dev)
        assert all(m.inplace is inplace for m in dev)
        assert {id(p) for p in model.parameters()} == params                  # the optimiser's tensors stay
        after = model.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], v) for k, v in before.items())
    assert model.layer1[0].bn3.fused_epilogues and model.layer1[0].downsample[1].activation == "identity"
    with pytest.raises(ValueError, match="mode"):
        abn.convert_abn(model, "cuda")
    relu = torch.nn.Sequential(inplace_abn.ABN(4, activation="relu"))
    abn.convert_abn(relu, "device")
    with pytest.raises(ValueError, match="relu"):
        abn.convert_abn(torch.nn.Sequential(inplace_abn.ABN(4, activation="relu")), "inplace")


def test_driver_flags():
    from ccnet_amd import eval_synthetic, train_synthetic
    for mod in (train_synthetic, eval_synthetic):
        assert mod.build_parser().parse_args([]).abn is None            # unset: the stock torch layers
        for mode in ("torch", "device", "inplace"):
            assert mod.build_parser().parse_args(["--abn", mode]).abn == mode
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--abn", "cuda"])


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._abn_lib import AbnLibrary
    return AbnLibrary(L.build_shared_scaffold_emu("abn"))


def emu_abn(lib, x, weight, bias, rm, rv, dy, **kw):
    """forward + backward through the emulated C ABI, numpy buffers standing in for device memory (abn_cases.run_abn)"""
    return K.run_abn(lib, K.HostMemory(), x, weight, bias, rm, rv, dy, **kw)


_close, _case, dx_scale = K.close, K.make_inputs, K.dx_scale


def check_against_oracle(r, x, w, b, rm, rv, dy, res, training, act, p, gamma_mode, eps=1e-5, bf16=False, tol=None,
                         tol_y=None):
    """the header's bar: 1e-5 (y, statistics) and 1e-4 (gradients) relative to the tensor's scale in fp32; one bf16 rounding
    on bf16 tensors, computed by the oracle from the same bf16-rounded inputs"""
    if bf16:
        q = lambda a: None if a is None else O.from_bf16_bits(O.to_bf16_bits(a))      # noqa: E731
        x, dy, res = q(x), q(dy), q(res)
    f = O.forward(x, w, b, rm, rv, training, eps=eps, act=act, p=p, gamma_mode=gamma_mode, residual=res)
    g = O.backward(f, dy, w, training, eps=eps, act=act, p=p, gamma_mode=gamma_mode)
    ty, tg = (2 ** -7, 2 ** -6) if bf16 else (1e-5, 1e-4)
    if tol:
        tg = tol
    if tol_y:
        ty = tol_y
    _close(r["y"], f["y"], ty, "y")
    _close(r["running_mean"], f["running_mean"], 1e-5, "running_mean")
    _close(r["running_var"], f["running_var"], 1e-5, "running_var")
    _close(r["dx"], g["dx"], tg, "dx", scale=dx_scale(f, g, w, gamma_mode))
    _close(r["dweight"], g["dweight"], tg, "dweight")
    _close(r["dbias"], g["dbias"], tg, "dbias")
    if res is not None:
        _close(r["dresidual"], g["dresidual"], tg, "dresidual")


# shape, activation, slope / alpha, gamma convention, source, residual, training; odd H * W everywhere but the 2 x 2 / 4 x 4
EMU_CASES = {
    "identity_oop": ((2, 3, 9, 11), 0, 0.0, 0, 0, False, True),
    "relu_oop_residual": ((2, 3, 9, 11), 1, 0.0, 0, 0, True, True),
    "leaky_oop": ((3, 2, 7, 13), 2, 0.01, 0, 0, False, True),
    "elu_oop": ((1, 4, 33, 31), 3, 1.0, 0, 0, False, True),
    "c1": ((2, 1, 45, 47), 2, 0.01, 0, 0, False, True),
    "n2_values": ((1, 3, 1, 2), 2, 0.01, 0, 0, False, True),
    "identity_inplace": ((2, 3, 9, 11), 0, 0.0, 1, 1, False, True),
    "leaky_inplace": ((2, 5, 19, 21), 2, 0.01, 1, 1, False, True),
    "elu_inplace_residual": ((2, 3, 9, 11), 3, 1.0, 1, 1, True, True),
    "leaky_inplace_residual": ((1, 2, 67, 65), 2, 0.1, 1, 1, True, True),
    "eval_relu": ((2, 3, 9, 11), 1, 0.0, 0, 0, True, False),
    "eval_leaky_inplace": ((2, 3, 9, 11), 2, 0.01, 1, 1, False, False),
    "big_plane_many_splits": ((1, 1, 130, 131), 0, 0.0, 0, 0, False, True),
}


@pytest.mark.parametrize("name", sorted(EMU_CASES))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_emulated_kernels_match_oracle(emu, name, bf16):
    shape, act, p, gm, source, residual, training = EMU_CASES[name]
    x, w, b, rm, rv, dy, res = _case(shape, seed=len(name), residual=residual)
    r = emu_abn(emu, x, w, b, rm, rv, dy, training=training, act=act, p=p, gamma_mode=gm, residual=res, source=source,
                bf16=bf16)
    # in-place bf16 rebuilds xhat from a bf16-rounded y: the gradient carries that rounding, amplified by 1 / gamma
    check_against_oracle(r, x, w, b, rm, rv, dy, res, training, act, p, gm, bf16=bf16,
                         tol=2 ** -4 if bf16 and source == 1 else None)


def test_emulated_statistics_survive_a_large_mean(emu):
    """a mean 1e4 standard deviations away: shifted fp64 sums keep the variance (E[x^2] - E[x]^2 in fp32 would not)"""
    x, w, b, rm, rv, dy, _ = _case((2, 3, 17, 19), seed=3, mean=1000.0, scale=0.1)
    r = emu_abn(emu, x, w, b, rm, rv, dy)
    f = O.forward(x, w, b, rm, rv, True)
    _close(r["saved"][0], f["mean"], 1e-12, "mean")
    _close(1.0 / r["saved"][1] ** 2, f["var"] + 1e-5, 1e-9, "var")
    # y and dx carry the fp32 rounding of the mean (ulp(1000) / 0.1 = 6e-4 of a standard deviation), as torch's do
    check_against_oracle(r, x, w, b, rm, rv, dy, None, True, 0, 0.0, 0, tol=2e-3, tol_y=1e-3)


def test_emulated_two_ranks_match_one(emu):
    """the rank-order Chan merge of two half batches and the summed backward sums give the whole batch's result"""
    x, w, b, rm, rv, dy, _ = _case((4, 3, 9, 11), seed=5)
    one = emu_abn(emu, x, w, b, rm, rv, dy, act=2)
    two = emu_abn(emu, x, w, b, rm, rv, dy, act=2, ranks=2)
    for k in ("y", "dx", "running_mean", "running_var"):
        _close(two[k], one[k], 1e-6, k)
    _close(two["dweight"], one["dweight"], 1e-6, "dweight")
    assert two["saved"][2][0] == 4 * 99


def test_emulated_weight_zero_gives_finite_gradients_in_place(emu):
    x, w, b, rm, rv, dy, _ = _case((2, 3, 9, 11), seed=7)
    w[1] = 0.0
    r = emu_abn(emu, x, w, b, rm, rv, dy, act=2, gamma_mode=1, source=1)
    assert all(np.isfinite(r[k]).all() for k in ("y", "dx", "dweight", "dbias"))
    assert r["dweight"][1] == 0.0                                 # d|w|/dw = sign(0) = 0
    check_against_oracle(r, x, w, b, rm, rv, dy, None, True, 2, 0.01, 1, tol=1e-2)


def test_emulated_results_repeat_bitwise(emu):
    x, w, b, rm, rv, dy, res = _case((2, 4, 23, 29), seed=11, residual=True)
    a = emu_abn(emu, x, w, b, rm, rv, dy, act=1, residual=res)
    c = emu_abn(emu, x, w, b, rm, rv, dy, act=1, residual=res)
    for k in ("y", "dx", "dweight", "dbias", "dresidual", "running_var"):
        assert np.array_equal(a[k], c[k]), k


def test_emulated_misaligned_pointers_take_the_element_path(emu):
    """a tensor that starts 4 bytes past a 16-byte boundary: the kernels fall back to element accesses, same result"""
    from ccnet_amd._abn_lib import make_desc
    x, w, b, rm, rv, dy, _ = _case((1, 2, 5, 7), seed=13)
    buf = np.zeros(x.size + 8, np.float32)
    off = (16 - buf.ctypes.data % 16) // 4 % 4 + 1
    xm = buf[off:off + x.size]
    xm[:] = x.ravel()
    assert xm.ctypes.data % 16 != 0
    d = make_desc(0, 1, 2, 35, 1, 0, 0.0, 0, 1e-5)
    ws = np.zeros(64)
    loc = np.zeros((3, 2))
    emu.check(emu.ccnet_abn_stats(ctypes.byref(d), xm.ctypes.data, loc.ctypes.data, ws.ctypes.data, ws.nbytes, None))
    saved = np.zeros((3, 2))
    emu.check(emu.ccnet_abn_stats_combine(ctypes.byref(d), loc.ctypes.data, 1, 0.1, None, None, saved.ctypes.data, None))
    y = np.zeros(x.size, np.float32)
    emu.check(emu.ccnet_abn_forward(ctypes.byref(d), xm.ctypes.data, None, y.ctypes.data, saved.ctypes.data, None, None,
                                    w.ctypes.data, b.ctypes.data, None))
    f = O.forward(x, w, b, rm, rv, True)
    _close(y.reshape(x.shape), f["y"], 1e-5, "y")


# ---------------------------------------------------------------------------------------------------------------------
# the shared case table (tests/abn_cases.py) through the emulator; tests/test_gpu_abn_edges.py runs it on the device
# ---------------------------------------------------------------------------------------------------------------------
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])


@DTYPES
@pytest.mark.parametrize("shape,sem", K.GRID_CASES, ids=lambda v: v)
def test_emulated_edge_shapes(emu, shape, sem, bf16):
    K.run_grid_case(emu, K.HostMemory(), shape, sem, bf16)


@DTYPES
@pytest.mark.parametrize("par,shape,sem", K.PARAMETER_CASES, ids=lambda v: v)
def test_emulated_parameter_forms(emu, par, shape, sem, bf16):
    K.run_parameter_case(emu, K.HostMemory(), par, shape, sem, bf16)


@pytest.mark.parametrize("name,shape,bf16", K.NUMERIC_CASES, ids=lambda v: {False: "f32", True: "bf16"}.get(v, v))
def test_emulated_numeric_edges(emu, name, shape, bf16):
    K.run_numeric_case(emu, K.HostMemory(), name, shape, bf16)


@DTYPES
@pytest.mark.parametrize("sem,shape", K.MISALIGNED_CASES, ids=lambda v: v)
def test_emulated_misaligned_tensors_give_the_aligned_result_bitwise(emu, sem, shape, bf16):
    K.run_misaligned_case(emu, K.HostMemory(), sem, shape, bf16)


@pytest.mark.parametrize("N,R,sem", K.RANK_CASES, ids=lambda v: str(v))
def test_emulated_uneven_ranks_match_one(emu, N, R, sem):
    K.run_rank_case(emu, K.HostMemory(), N, R, sem)


@pytest.mark.parametrize("sem", ["oop_relu_res", "ip_leaky01_res"])
def test_emulated_non_finite_input_stays_in_its_channel_and_in_its_statistics(emu, sem):
    K.run_nonfinite_case(emu, K.HostMemory(), sem)


def test_guard_bands_catch_a_store_outside_the_tensor():
    """the driver's own check: a write one element before or after a buffer's data is seen"""
    mem = K.HostMemory()
    for kind, dtype in (("f32", np.float32), ("bf16", np.uint16), ("f64", np.float64)):
        for where in (-1, 5):
            q = K.Buf(mem, "t", kind, 5, offset=1, data=np.zeros(5, dtype))
            assert q.read(dtype)[1]
            q.raw.view(np.uint8)[q.start + where * q.size] ^= 1
            assert not q.read(dtype)[1], (kind, where)


def test_in_place_design_error_is_what_the_header_states():
    """the two oracles alone, no kernel: from-output on the exact y rounded to storage, against the exact gradients"""
    e = {(act, bf16, w): K.in_place_design_error(act, p, float(w), bf16)
         for act, p in ((O.ELU, 1.0), (O.LEAKY_RELU, 0.01)) for bf16 in (False, True) for w in (1, 4, 8, 20)}
    assert all(e[O.LEAKY_RELU, False, w]["dx"] <= 1e-7 for w in (1, 4, 8, 20))         # leaky_relu loses nothing
    assert e[O.ELU, False, 1]["dx"] <= 1e-6 and e[O.ELU, False, 4]["dx"] <= 1e-4       # elu: fine while z > -16 ...
    assert e[O.ELU, False, 4]["min_z"] > -16.6 > e[O.ELU, False, 8]["min_z"]
    assert e[O.ELU, False, 8]["dx"] > 1e-3 and e[O.ELU, False, 20]["dx"] > 1e-3        # ... and off the bar beyond
    assert all(v[k] <= (2 ** -6 if bf16 else 1e-4) for (_, bf16, _), v in e.items() for k in ("dweight", "dbias"))
