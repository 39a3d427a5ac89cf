"""CPU checks of the channels_last device ABN (include/ccnet_abncl.h, ccnet_amd/csrc_abncl/): the shipped gfx950 library's
surface, the Python front end's dispatch, the driver flag, and the kernel sources themselves run in the SIMT emulator
(tests/emu/ + the ABN primitives of tests/emu_abn/) over the case table of tests/abncl_cases.py against the float64 oracle of
tests/abn_oracle.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import abncl_cases as P
import lib_checks as L
from conftest import ROOT

AMD = os.path.join(ROOT, "ccnet_amd")
ABNCL_CSRC, ABN_CSRC = os.path.join(AMD, "csrc_abncl"), os.path.join(AMD, "csrc_abn")


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _abncl_lib
    return _abncl_lib.LIB_PATH


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _abncl_lib
    names = _abncl_lib.declared_symbols()
    assert set(names) == set(_abncl_lib._PROTOTYPES) and len(names) == 10
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"_ZN5abncl20stats_partial_kernel" in blob and b"_ZN5abncl21backward_apply_kernel" in blob


def test_header_constants_match_the_binding_and_ccnet_abn():
    from ccnet_amd import _abn_lib, _abncl_lib
    text = open(_abncl_lib.HEADER_PATH).read()
    consts = dict(re.findall(r"#define (CCNET_ABNCL_\w+) (\d+)", text))
    for name, value in consts.items():
        assert getattr(_abncl_lib, name) == int(value), name
        if name != "CCNET_ABNCL_VERSION":              # the same codes as include/ccnet_abn.h: one Op serves both libraries
            assert getattr(_abn_lib, name.replace("ABNCL", "ABN")) == int(value), name
    assert len(consts) == 11
    fields = re.search(r"typedef struct ccnet_abncl_desc \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f for f, _ in _abncl_lib.AbnClDesc._fields_]


def _desc(dtype=1, M=9409, C=64, act=0, p=0.01, gm=0, eps=1e-5):
    from ccnet_amd._abncl_lib import make_desc
    return make_desc(dtype, M, C, act, p, gm, eps)


def test_version_splits_and_argument_validation_without_a_gpu(lib_path):
    from ccnet_amd import _abncl_lib
    lib = _abncl_lib.AbnClLibrary(lib_path)
    assert lib.ccnet_abncl_version() == 100 and lib.ccnet_abncl_arch() == b"gfx950"
    ws, sp = lib.ccnet_abncl_workspace_bytes, lib.ccnet_abncl_splits
    assert ws(None) == 0 and sp(None) == 0
    for bad in (_desc(M=0), _desc(C=0), _desc(dtype=2), _desc(act=4), _desc(act=2, p=-0.1), _desc(act=3, p=0.0),
                _desc(gm=1, eps=0.0), _desc(M=1 << 31, C=1), _desc(M=1 << 30, C=1 << 10)):
        assert ws(ctypes.byref(bad)) == 0 and sp(ctypes.byref(bad)) == 0
    assert sp(ctypes.byref(_desc(M=(1 << 31) - 1, C=1))) >= 1
    # slabs of at least 256 rows, about 2048 workgroups over tiles of 64 bf16 / 32 fp32 channels, at most 64, none empty
    assert sp(ctypes.byref(_desc(M=385 * 385, C=64))) == 64                    # one tile: 580 slabs of 256 rows fit, 64 are cut
    assert sp(ctypes.byref(_desc(M=64 * 256, C=8))) == 64 and sp(ctypes.byref(_desc(M=63 * 256, C=8))) == 63
    assert sp(ctypes.byref(_desc(M=97 * 97, C=2048))) == 37                    # 32 tiles: 64 wanted, 37 of 256 rows fit
    assert sp(ctypes.byref(_desc(dtype=0, M=97 * 97, C=2048))) == 32           # 64 fp32 tiles: 2048 / 64
    assert sp(ctypes.byref(_desc(M=1000000, C=64))) == 64
    assert sp(ctypes.byref(_desc(M=3970, C=8))) == 16 and sp(ctypes.byref(_desc(M=3856, C=8))) == 16
    assert sp(ctypes.byref(_desc(M=256, C=8))) == 1 and sp(ctypes.byref(_desc(M=257, C=8))) == 2
    assert sp(ctypes.byref(_desc(M=1, C=1))) == 1
    assert ws(ctypes.byref(_desc(M=97 * 97, C=2048))) == 2048 * 37 * 16
    one = ctypes.c_double(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    d = ctypes.byref(_desc())
    n = ws(d)
    assert lib.ccnet_abncl_stats(d, None, p, p, n, None) == -2
    assert lib.ccnet_abncl_stats(d, p, p, p, n - 1, None) == -3
    assert "workspace" in lib.last_error()
    assert lib.ccnet_abncl_stats(ctypes.byref(_desc(C=0)), p, p, p, n, None) == -1
    assert lib.ccnet_abncl_stats(None, p, p, p, n, None) == -2
    assert lib.ccnet_abncl_stats_combine(d, p, 0, 0.1, None, None, p, None) == -1
    assert lib.ccnet_abncl_stats_combine(d, None, 1, 0.1, None, None, p, None) == -2
    assert lib.ccnet_abncl_forward(d, p, None, None, p, None, None, None, None, None) == -2
    assert lib.ccnet_abncl_forward(d, p, None, p, None, None, None, None, None, None) == -2     # eval without running stats
    relu = ctypes.byref(_desc(act=1))
    red, app = lib.ccnet_abncl_backward_reduce, lib.ccnet_abncl_backward_apply
    assert red(relu, 1, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -1   # relu from y
    assert "relu" in lib.last_error()
    assert red(ctypes.byref(_desc(act=2, p=0.0)), 1, p, None, p, None, p, None, None, None, None, p, None, None, p, n,
               None) == -1
    assert red(d, 2, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -1      # bad source
    assert red(relu, 0, p, None, p, None, p, None, None, None, None, p, None, None, p, n, None) == -2   # act' needs y
    assert red(d, 0, p, None, p, None, p, None, None, None, None, p, None, None, p, 8, None) == -3
    assert app(d, 0, p, None, p, None, p, None, None, None, None, None, 1, p, None, None) == -2         # no sums
    assert app(d, 0, p, None, p, None, p, None, None, None, None, p, 1, p, None, None) == -1            # dx aliases dy
    assert lib.last_error().startswith("ccnet_abncl:")


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN5abncl")
    assert len(kernels) == 8, sorted(kernels)               # 4 templates x 2 dtypes
    shared = L.code_object_kernels(lib_path, tmp_path, "_ZN3abn")
    assert len(shared) == 4, sorted(shared)                 # stats_finalize x 2 dtypes, stats_combine, backward_finalize
    bad = L.kernels_using_scratch({**kernels, **shared})
    assert not bad, bad


def test_sources_carry_no_env_knobs_no_emulator_code_and_no_float_atomics():
    files = L.product_sources(ABNCL_CSRC)
    assert sorted(files) == ["abncl_api.hip", "abncl_kernels.hpp"]         # the platform header is csrc_abn/'s
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomic" not in text.lower(), f
        assert "__fdividef" not in text and "fast-math" not in text and "hipDeviceSynchronize" not in text, f
        assert "hipStreamSynchronize" not in text and "hipMemcpy" not in text, f
    py = "".join(open(os.path.join(AMD, f)).read() for f in ("abn.py", "abncl.py", "_abncl_lib.py"))
    assert "environ" not in py and "getenv" not in py


def test_unit_list_adds_one_library_and_leaves_the_pinned_lists_alone():
    import __graft_entry__ as g
    assert [e.name for e in g.CONV_UNITS] == ["conv3"] and [e.name for e in g.NORM_UNITS] == ["abncl"]
    every = g.all_libraries() + g.LATER_UNITS + g.MIXED_UNITS + g.CONV_UNITS + g.NORM_UNITS
    assert len(every) == 15 and len({e.lib for e in every}) == 15
    unit = g.NORM_UNITS[0]
    assert unit.csrc == g.ABNCL_CSRC == ABNCL_CSRC and unit.lib == g.ABNCL_LIB and unit.flags == g.ABNCL_HIPCC_FLAGS
    assert "-I" + ABN_CSRC in unit.flags and "-fvisibility=hidden" in unit.flags
    assert "-Wl,--version-script=" + os.path.join(ABNCL_CSRC, "exports.map") in unit.flags
    srcs = unit.sources()
    assert os.path.join(ABN_CSRC, "abn_kernels.hpp") in srcs and os.path.join(ABN_CSRC, "abn_platform.hpp") in srcs
    assert os.path.join(ABN_CSRC, "abn_api.hip") not in srcs            # read, not compiled
    assert g.ABN_HIPCC_FLAGS == [f for f in g.ABN_HIPCC_FLAGS if "abncl" not in f]


# ---------------------------------------------------------------------------------------------------------------------
# the Python front end without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_convert_abn_channels_last_keeps_parameters_buffers_and_state_dict_keys():
    import torch
    import inplace_abn
    from ccnet_amd import abn
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = {id(p) for p in model.parameters()}
    assert abn.ABN.channels_last is False and abn.InPlaceABNSync.channels_last is False
    for mode, flag in (("device", True), ("inplace", True), ("device", False)):
        abn.convert_abn(model, mode, channels_last=flag)
        dev = [m for m in model.modules() if isinstance(m, inplace_abn.ABN)]
        assert len(dev) == 110 and all(type(m) in (abn.ABN, abn.InPlaceABN, abn.InPlaceABNSync) for m in dev)
        assert all(m.channels_last is flag and m.inplace is (mode == "inplace") for m in dev)
        assert {id(p) for p in model.parameters()} == params
        after = model.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], v) for k, v in before.items())
    abn.convert_abn(model, "device")
    assert not any(m.channels_last for m in model.modules() if isinstance(m, inplace_abn.ABN))


def test_front_end_dispatch_by_layout(monkeypatch):
    """which function a layer enters, on CPU tensors: the two functions are replaced by recorders (and the device check, which
    refuses CPU tensors, by nothing)"""
    import torch
    from ccnet_amd import abn, abncl
    entered = []
    monkeypatch.setattr(abn._DeviceABN, "_check", lambda self, x, activation: None)
    monkeypatch.setattr(abn.ABNFunction, "apply", staticmethod(lambda x, *a: entered.append(("nchw", x)) or x))
    monkeypatch.setattr(abncl.ABNChannelsLastFunction, "apply", staticmethod(lambda x, *a: entered.append(("cl", x)) or x))
    cl = torch.channels_last
    x = torch.randn(2, 6, 5, 7)
    inputs = {
        "nchw": (x, "nchw"),
        "channels_last": (x.contiguous(memory_format=cl), "cl"),
        "c1": (torch.randn(2, 1, 5, 7).contiguous(memory_format=cl), "nchw"),          # both layouts at once
        "hw1": (torch.randn(2, 6, 1, 1).contiguous(memory_format=cl), "nchw"),
        "2d": (torch.randn(4, 6), "nchw"),
        "3d": (torch.randn(4, 6, 5), "nchw"),
        "strided": (torch.randn(2, 12, 5, 7).contiguous(memory_format=cl)[:, :6], "nchw"),   # a channel slice: not dense
        "strided_w": (x[:, :, :, ::2], "nchw"),
    }
    layer = abn.ABN(6)
    one = abn.ABN(1)
    for flag in (True, False):
        layer.channels_last = one.channels_last = flag
        for name, (t, want) in inputs.items():
            entered.clear()
            (one if t.shape[1] == 1 else layer)(t)
            route, got = entered[0]
            assert route == (want if flag else "nchw"), (name, flag)
            if route == "cl":
                assert got.data_ptr() == t.data_ptr() and got.stride() == t.stride()       # as it lies: no copy
            else:
                assert got.is_contiguous()
    # in place: what cannot be overwritten where it lies is refused, in both settings
    ip = abn.InPlaceABN(6)
    with pytest.raises(ValueError, match="contiguous NCHW input"):
        ip(inputs["channels_last"][0])
    ip.channels_last = True
    entered.clear()
    ip(inputs["channels_last"][0])
    ip(inputs["nchw"][0])
    assert [r for r, _ in entered] == ["cl", "nchw"]
    for name in ("strided", "strided_w"):
        with pytest.raises(ValueError, match="dense channels_last"):
            ip(inputs[name][0])
    # a residual follows the input's layout
    entered.clear()
    monkeypatch.setattr(abncl.ABNChannelsLastFunction, "apply",
                        staticmethod(lambda x, w, b, rm, rv, res, cfg: entered.append(res) or x))
    layer.channels_last = True
    layer(inputs["channels_last"][0], residual=torch.randn(2, 6, 5, 7))
    assert abncl.is_dense_channels_last(entered[0]) and not entered[0].is_contiguous()
    with pytest.raises(ValueError, match="residual"):
        layer(inputs["channels_last"][0], residual=torch.randn(2, 6, 5, 6))


def test_function_refuses_an_input_that_is_not_dense_channels_last():
    import torch
    from ccnet_amd.abncl import ABNChannelsLastFunction
    cfg = (True, 0.1, 1e-5, 0, 0.0, False, None)
    with pytest.raises(ValueError, match="dense channels_last"):
        ABNChannelsLastFunction.apply(torch.randn(2, 6, 5, 7), None, None, None, None, None, cfg)


def test_public_names():
    import ccnet_amd
    assert "ABNChannelsLastFunction" in ccnet_amd.__all__ and ccnet_amd.ABNChannelsLastFunction.__module__ == "ccnet_amd.abncl"


def test_driver_flag_refusals_and_acceptances():
    from ccnet_amd import train_synthetic as T
    parse = lambda *a: T.build_parser().parse_args(list(a))                     # noqa: E731
    assert parse().abn_channels_last is False
    refused = (
        (("--abn-channels-last", "--device-conv3", "--bf16-params"), "--abn device"),             # no --abn
        (("--abn-channels-last", "--device-conv3", "--bf16-params", "--abn", "torch"), "--abn device"),
        (("--abn-channels-last", "--abn", "device", "--bf16-params"), "--device-conv3"),
        (("--device-conv3", "--bf16-params", "--abn", "device"), "NCHW"),                         # as before, without the flag
    )
    for argv, word in refused:
        with pytest.raises(ValueError, match=word):
            T.check_args(parse(*argv))
    T.check_args(parse("--device-conv3", "--bf16-params", "--abn", "device", "--abn-channels-last"))
    T.check_args(parse("--device-conv3", "--bf16", "--abn", "inplace", "--abn-channels-last"))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator: tests/emu_abn's platform header in front of csrc_abn/'s
# ---------------------------------------------------------------------------------------------------------------------
def build_emu(force=False):
    emu_abn = os.path.join(ROOT, "tests", "emu_abn")
    return L.build_emu_library(os.path.join(emu_abn, "libabncl_emu.so"), os.path.join(ABNCL_CSRC, "abncl_api.hip"),
                               [emu_abn, L.EMU_DIR, ABNCL_CSRC, ABN_CSRC, L.INCLUDE], reads=(L.EMU_COMMON_DIR, L.COMMON_CSRC),
                               force=force)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._abncl_lib import AbnClLibrary
    return AbnClLibrary(build_emu())


DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])


@DTYPES
def test_case_table_reaches_its_edges(emu, bf16):
    """what the shapes' comments claim, from the library's own plan"""
    V = 8 if bf16 else 4
    C = {name: shape[1] for name, shape in P.SHAPES.items()}
    assert C["c5"] % V and C["odd"] % V and (C["c12"] % V == 0) == (not bf16)
    assert all(C[name] % 8 == 0 for _, name in P.MISALIGNED_CASES)
    S, chunk = P.splits(emu, P.SHAPES["slabs"], bf16)
    M = 2 * 37 * 41
    assert S >= 3 and M % chunk != 0 and (S - 1) * chunk < M, (S, chunk)        # the last slab is partial, none is empty
    assert P.splits(emu, P.SHAPES["row_blocks"], bf16) == (64, 261) and 129 * 129 == 64 * 256 + 257
    assert all(P.splits(emu, P.SHAPES[name], bf16)[0] == 1 for name in P.SHAPES if name not in ("slabs", "row_blocks"))
    sems = {sem for shape in ("c5",) for sem in P.GRID[shape]} & set(P.GRID["slabs"])
    assert sems == set(P.K.SEMANTICS)
    for shape, names in P.GRID.items():
        kinds = [P.K.SEMANTICS[s] for s in names]
        assert any(not k[4] for k in kinds), shape                               # eval mode
        if shape != "m1_eval":
            assert {k[2] for k in kinds} == {0, 1} and any(k[3] for k in kinds), shape     # both modes, a residual
        else:
            assert not any(k[4] for k in kinds)


@DTYPES
@pytest.mark.parametrize("shape,sem", P.GRID_CASES, ids=lambda v: v)
def test_emulated_edge_shapes(emu, shape, sem, bf16):
    P.run_grid_case(emu, P.HostMemory(), shape, sem, bf16)


@DTYPES
@pytest.mark.parametrize("par,shape,sem", P.PARAMETER_CASES, ids=lambda v: v)
def test_emulated_parameter_forms(emu, par, shape, sem, bf16):
    P.run_parameter_case(emu, P.HostMemory(), par, shape, sem, bf16)


@pytest.mark.parametrize("name,shape,bf16", P.NUMERIC_CASES, ids=lambda v: {False: "f32", True: "bf16"}.get(v, v))
def test_emulated_numeric_edges(emu, name, shape, bf16):
    P.run_numeric_case(emu, P.HostMemory(), name, shape, bf16)


@DTYPES
@pytest.mark.parametrize("sem,shape", P.MISALIGNED_CASES, ids=lambda v: v)
def test_emulated_misaligned_tensors_give_the_aligned_result_bitwise(emu, sem, shape, bf16):
    """C % V == 0: the aligned run takes 16-byte accesses (the emulator's load16 aborts on a misaligned one), every offset
    run the element path"""
    P.run_misaligned_case(emu, P.HostMemory(), sem, shape, bf16)


@pytest.mark.parametrize("N,R,sem", P.RANK_CASES, ids=lambda v: str(v))
def test_emulated_uneven_ranks_match_one(emu, N, R, sem):
    P.run_rank_case(emu, P.HostMemory(), N, R, sem)


@pytest.mark.parametrize("sem", P.NONFINITE_CASES)
def test_emulated_non_finite_input_stays_in_its_channel_and_in_its_statistics(emu, sem):
    P.run_nonfinite_case(emu, P.HostMemory(), sem)


@DTYPES
@pytest.mark.parametrize("shape,sem", [("tile_tail", "oop_relu_res"), ("slabs", "ip_leaky01_res")], ids=lambda v: v)
def test_emulated_results_repeat_bitwise(emu, shape, sem, bf16):
    P.run_repeat_case(emu, P.HostMemory(), shape, sem, bf16)


def test_guard_bands_are_checked_by_the_driver(emu):
    """run_abncl asserts every band itself; a library that wrote one element past y would be seen: the check is abn_cases'
    (tests/test_abn_host.py::test_guard_bands_catch_a_store_outside_the_tensor), and the driver here reads every buffer"""
    x, w, b, rm, rv, dy, res = P.K.table_inputs(P.SHAPES["c5"], 1, residual=True)
    r = P.run_abncl(emu, P.HostMemory(), x, w, b, rm, rv, dy, residual=res, act=1)
    assert set(r) >= {"y", "dx", "dresidual", "dweight", "dbias", "saved", "sums"} and r["y"].shape == x.shape
    # the transposition is the driver's own: channel c of the result is channel c of the input
    f = P.O.forward(x, w, b, rm, rv, True, act=1, residual=res)
    assert np.abs(r["y"] - f["y"]).max() < 1e-4 and np.abs(r["saved"][0] - f["mean"]).max() < 1e-6
