"""CPU checks of the mixed-precision optimiser library (include/ccnet_sgdmp.h, ccnet_amd/csrc_sgdmp/, ccnet_amd/optim.py): the
shipped gfx950 library's surface and its place in the build table, the chunk plan against ccnet_sgd_plan's, every refusal without
a device (through the emulator build, on guarded buffers), the rounding to bf16 against hand values and against torch's, and
what DeviceMixedSGD, bf16_parameters and the driver's --bf16-params take and refuse before they touch a device."""
import os
import re

import numpy as np
import pytest
import torch

import lib_checks as L
import sgdmp_oracle as M
from conftest import ROOT
from guarded_memory import HostMemory

CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_sgdmp")
C = M.C


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _sgdmp_lib
    return _sgdmp_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _sgdmp_lib
    return _sgdmp_lib.SgdmpLibrary(lib_path)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._sgdmp_lib import SgdmpLibrary
    return SgdmpLibrary(L.build_shared_scaffold_emu("sgdmp"))


def test_the_library_is_a_unit_of_a_further_list_and_the_pinned_lists_stay():
    import __graft_entry__ as g
    rows = [u for e in g.EXTENSIONS for u in e.libraries()]
    assert len(rows) == 9 and g.all_libraries() == rows + g.SECOND_UNITS
    assert [e.name for e in g.SECOND_UNITS] == ["celovasz", "augment"] and [e.name for e in g.LATER_UNITS] == ["sgd"]
    assert [e.name for e in g.MIXED_UNITS] == ["sgdmp"]
    assert len(g.all_libraries() + g.LATER_UNITS + g.MIXED_UNITS) == 13
    unit = g.MIXED_UNITS[0]
    assert unit.csrc == CSRC and unit.binding == "_sgdmp_lib" and unit.exports == os.path.join(CSRC, "exports.map")
    assert unit.unit == os.path.join(CSRC, "sgdmp_api.hip") and unit.header.endswith("ccnet_sgdmp.h")
    assert g.SGDMP_CSRC == CSRC and g.SGDMP_LIB == os.path.join(CSRC, "libccnet_sgdmp.so")
    assert g.SGDMP_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-I" + CSRC,
                                                   "-I" + os.path.join(ROOT, "include")]
    assert g.SGDMP_HIPCC_FLAGS[3:] == [f.replace("csrc_sgd", "csrc_sgdmp") for f in g.SGD_HIPCC_FLAGS[3:]]     # the same rule
    assert os.path.join(ROOT, "ccnet_amd", "csrc_common", "ccnet_host.hpp") in unit.sources()


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _sgdmp_lib
    names = _sgdmp_lib.declared_symbols()
    assert names == sorted(["ccnet_sgdmp_version", "ccnet_sgdmp_arch", "ccnet_sgdmp_last_error_string", "ccnet_sgdmp_plan",
                            "ccnet_sgdmp_step"])
    assert set(names) == set(_sgdmp_lib._PROTOTYPES)
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code_and_the_binding_mirrors_the_header(lib_path, lib):
    from ccnet_amd import _sgd_lib
    from ccnet_amd import _sgdmp_lib as m
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"_ZN5sgdmp11step_kernel" in blob and b"_ZN5sgdmp14advance_kernel" in blob
    assert lib.ccnet_sgdmp_version() == 100 == m.CCNET_SGDMP_VERSION and lib.ccnet_sgdmp_arch() == b"gfx950"
    header = open(m.HEADER_PATH).read()
    for name, value in (("VERSION", 100), ("TENSOR_WORDS", m.TENSOR_WORDS), ("P", m.P), ("G", m.G), ("B", m.B),
                        ("NUMEL", m.NUMEL), ("GROUP", m.GROUP), ("M", m.M)):
        assert re.search(rf"#define CCNET_SGDMP_{name}\s+{value}\b", header), name
    assert (m.P, m.G, m.B, m.NUMEL, m.GROUP, m.M, m.TENSOR_WORDS) == (0, 1, 2, 3, 4, 5, 6)
    # the chunk size and the limits are ccnet_sgd.h's, which the header includes
    assert '#include "ccnet_sgd.h"' in header
    assert (m.CHUNK, m.MAX_GROUPS, m.MAX_TENSORS, m.DEFAULT_CAP) == (_sgd_lib.CHUNK, _sgd_lib.MAX_GROUPS, _sgd_lib.MAX_TENSORS,
                                                                     _sgd_lib.DEFAULT_CAP)


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_the_kernels_use_no_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN5sgdmp")
    assert len(kernels) == 2, sorted(kernels)
    assert not L.kernels_using_scratch(kernels)


def test_sources_carry_no_env_knobs_no_emulator_code_no_atomics_and_no_copies():
    files = L.product_sources(CSRC)
    assert set(files) == {"sgdmp_api.hip", "sgdmp_kernels.hpp", "sgdmp_platform.hpp"}
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomicAdd" not in text and "__shared__" not in text and "asm volatile" not in text, f
        assert "hipMemcpy" not in text and "Synchronize" not in text and "hipMalloc" not in text, f       # nothing is read back
    assert "#pragma clang fp contract(off)" in files["sgdmp_kernels.hpp"]
    assert "address_space(1)" in files["sgdmp_platform.hpp"]


def test_binding_refuses_a_missing_library_and_another_abi_version(lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _sgdmp_lib as m
    assert issubclass(m.SgdmpError, RuntimeError)
    with pytest.raises(m.SgdmpError, match="not found"):
        m.SgdmpLibrary(str(tmp_path / "libccnet_missing.so"))
    monkeypatch.setattr(m, "CCNET_SGDMP_VERSION", m.CCNET_SGDMP_VERSION + 1)
    with pytest.raises(m.SgdmpError, match="rebuild"):
        m.SgdmpLibrary(m.LIB_PATH)


def test_plan_equals_ccnet_sgd_plan_on_the_case_sizes(lib, lib_path):
    import __graft_entry__ as g
    from ccnet_amd import _sgd_lib
    stock = _sgd_lib.SgdLibrary(g.SGD_LIB)
    for name in M.CASES:
        sizes = M.build_case(name)["sizes"]
        got = lib.plan(sizes)
        assert got.dtype == np.int32 and np.array_equal(got, stock.plan(sizes)) and np.array_equal(got, M.S.plan(sizes)), name
    from ctypes import c_int64
    n = c_int64(-7)
    numel = np.array([5, 3 * C, 2 ** 31 - 1], np.int64)
    assert lib.ccnet_sgdmp_plan(numel.ctypes.data, 3, None, 0, n) == 0 and n.value == 1 + 3 + (2 ** 31 - 1 + C - 1) // C
    small = np.zeros((2, 2), np.int32)
    assert lib.ccnet_sgdmp_plan(numel.ctypes.data, 2, small.ctypes.data, 2, n) == -5 and "room for 2" in lib.last_error()
    assert not small.any()
    numel[1] = 2 ** 31
    assert lib.ccnet_sgdmp_plan(numel.ctypes.data, 3, None, 0, n) == -3 and "outside 1..2^31-1" in lib.last_error()
    assert lib.ccnet_sgdmp_plan(numel.ctypes.data, 0, None, 0, n) == -1 and lib.ccnet_sgdmp_plan(None, 1, None, 0, n) == -2
    assert lib.last_error().startswith("ccnet_sgdmp: plan")


def set_(key, value):
    def mutate(args):
        args[key] = value
    return mutate


def table(row, col, value):
    def mutate(args):
        args["tensors_host"] = args["tensors_host"].copy()
        args["tensors_host"][row, col] = value
    return mutate


def add_to_table(row, col, delta):
    def mutate(args):
        args["tensors_host"] = args["tensors_host"].copy()
        args["tensors_host"][row, col] += delta
    return mutate


def chunk(row, col, value):
    def mutate(args):
        args["chunks_host"] = args["chunks_host"].copy()
        args["chunks_host"][row, col] = value
    return mutate


def nine_groups(args):
    args.update(lr=np.zeros(9, np.float32), wd=np.zeros(9, np.float32), mu=np.zeros(9, np.float32), n_groups=9)


# ("interleaved": rows 0, 2, 4, 7 are float32 rows, the others master rows)
REFUSALS = [
    ("null_tensors_host", "one_to_17", set_("tensors_host", None), -2, "NULL tensor table"),
    ("null_tensors_device", "one_to_17", set_("tensors_device", None), -2, "NULL tensor table"),
    ("null_chunks_host", "one_to_17", set_("chunks_host", None), -2, "NULL tensor table or chunk table"),
    ("null_chunks_device", "one_to_17", set_("chunks_device", None), -2, "NULL tensor table or chunk table"),
    ("null_lr", "one_to_17", set_("lr", None), -2, "NULL lr"),
    ("null_mu", "one_to_17", set_("mu", None), -2, "NULL lr, wd or mu"),
    ("no_tensors", "one_to_17", set_("n_tensors", 0), -1, "0 tensors"),
    ("too_many_tensors", "one_to_17", set_("n_tensors", 65536), -1, "65536 tensors"),
    ("negative_cap", "one_to_17", set_("cap", -1), -1, "cap -1 is negative"),
    ("numel_zero", "one_to_17", table(2, 3, 0), -3, "tensor 2 has 0 elements"),
    ("numel_negative", "one_to_17", table(2, 3, -4), -3, "tensor 2 has -4 elements"),
    ("numel_2_31", "one_to_17", table(7, 3, 2 ** 31), -3, "tensor 7 has 2147483648 elements"),
    ("chunks_short", "chunk_edges", set_("n_chunks", 6), -5, "chunk table"),
    ("chunks_long", "chunk_edges", set_("n_chunks", 8), -5, "chunk table has 8 entries, the plan 7"),
    ("chunk_wrong_tensor", "chunk_edges", chunk(3, 0, 1), -5, "differs from the plan at entry 3"),
    ("chunk_wrong_index", "chunk_edges", chunk(6, 1, 3), -5, "differs from the plan at entry 6"),
    ("numel_not_the_plans", "chunk_edges", table(1, 3, C + 1), -5, "differs from the plan"),
    ("group_outside", "groups", table(3, 4, 3), -6, "tensor 3 is in group 3 of 3"),
    ("group_negative", "groups", table(0, 4, -1), -6, "tensor 0 is in group -1"),
    ("nine_groups", "groups", nine_groups, -6, "9 groups"),
    ("no_groups", "groups", set_("n_groups", 0), -6, "0 groups"),
    ("schedule_without_counter", "schedule_0", set_("counter", None), -7, "needs a counter"),
    ("schedule_empty", "schedule_0", set_("schedule_len", 0), -7, "schedule of length 0"),
    ("null_p", "interleaved", table(3, 0, 0), -8, "tensor 3 has a NULL parameter"),
    ("null_b", "interleaved", table(5, 2, 0), -8, "tensor 5 has a NULL parameter or momentum buffer"),
    ("master_m_misaligned", "interleaved", add_to_table(1, 5, 2), -8, "tensor 1 has a master or momentum buffer that is not 4-byte"),
    ("master_b_misaligned", "interleaved", add_to_table(3, 2, 1), -8, "tensor 3 has a master or momentum buffer that is not 4-byte"),
    ("master_p_misaligned", "interleaved", add_to_table(6, 0, 1), -8, "tensor 6 has a bf16 parameter or gradient that is not 2-byte"),
    ("master_g_misaligned", "interleaved", add_to_table(8, 1, 3), -8, "tensor 8 has a bf16 parameter or gradient that is not 2-byte"),
    ("float_p_misaligned", "interleaved", add_to_table(2, 0, 2), -8, "tensor 2 has a parameter, gradient or momentum buffer that is not 4-byte"),
    ("float_g_misaligned", "interleaved", add_to_table(7, 1, 2), -8, "tensor 7 has a parameter, gradient or momentum buffer that is not 4-byte"),
]


@pytest.mark.parametrize("case_name,mutate,code,words", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_every_refusal_has_its_code_and_text_and_writes_nothing(emu, case_name, mutate, code, words):
    case = M.build_case(case_name)
    got_code, got, intact = M.run_raw(emu, HostMemory(), case, mutate)
    assert got_code == code, emu.last_error()
    assert emu.last_error().startswith("ccnet_sgdmp: step: ") and words in emu.last_error(), emu.last_error()
    assert intact and M.unchanged(case, got)


def test_a_master_row_two_bytes_off_is_taken_where_a_float_row_is_refused(emu):
    # (the same 2-byte offset of p: legal in bf16, refused in float32)
    case = M.build_case("misaligned")
    assert case["offsets"][0] == (1, 0, 0, 0) and case["master"][0]
    code, got, intact = M.run_raw(emu, HostMemory(), case)
    assert code == 0 and intact


def nan_aware_equal(a, b):
    nan = M.is_nan16(b)
    return np.array_equal(M.is_nan16(a), nan) and np.array_equal(a[~nan], b[~nan])


def test_bf16_rne_gives_the_hand_values_and_equals_torchs_cast():
    bits = np.array([u for u, _ in M.ROUNDING], np.uint32)
    assert M.bf16_rne(bits).tolist() == [h for _, h in M.ROUNDING]
    nans = np.array([0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF, 0xFF800001], np.uint32)
    assert M.is_nan16(M.bf16_rne(nans)).all()                                   # a NaN gives some NaN, never an infinity
    rng = np.random.default_rng(20240)
    sample = np.concatenate([bits, nans, rng.integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)])
    theirs = torch.from_numpy(sample.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert nan_aware_equal(M.bf16_rne(sample), theirs)
    # and back: widening is exact
    assert np.array_equal(M.bf16_of(M.float_of(theirs[~M.is_nan16(theirs)])), theirs[~M.is_nan16(theirs)])


def test_the_point_of_a_master_in_the_oracle():
    # p = 1, g = 1, lr = 2^-11, 32 steps: the master reaches 1 - 2^-6 exactly, while every single update, 2^-11, is below half a
    # bf16 ulp below 1.0 (2^-10), so that rounding after every step would still hold 1.0
    m, b = np.ones(1, np.float32), np.zeros(1, np.float32)
    g = M.bf16_of(np.ones(1, np.float32))
    lossy = np.ones(1, np.float32)
    for _ in range(32):
        m, b, p = M.master_step(g, m, b, 2.0 ** -11, 0.0, 0.0)
        lossy = M.float_of(M.bf16_of(lossy - np.float32(2.0 ** -11)))
    assert float(m[0]) == 1 - 2.0 ** -6 == float(M.float_of(p)[0]) and float(lossy[0]) == 1.0


def param(dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(3, dtype=dtype))


def test_device_mixed_sgd_refuses_cpu_tensors_other_dtypes_and_what_device_sgd_refuses():
    import ccnet_amd
    from ccnet_amd.optim import DeviceMixedSGD, DeviceSGD
    assert ccnet_amd.DeviceMixedSGD is DeviceMixedSGD and issubclass(DeviceMixedSGD, torch.optim.Optimizer)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match="DeviceMixedSGD needs parameters on a HIP device .*no CPU fallback"):
            DeviceMixedSGD([param(dtype)], lr=0.1)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(ValueError, match="DeviceMixedSGD takes float32 and bfloat16 parameters, got " + str(dtype)):
            DeviceMixedSGD([param(dtype)], lr=0.1)
    with pytest.raises(ValueError, match="DeviceMixedSGD takes at most 8 parameter groups, got 9"):
        DeviceMixedSGD([{"params": [param()]} for _ in range(9)], lr=0.1)
    for kw in ({"dampening": 0.1}, {"nesterov": True}, {"maximize": True}):
        with pytest.raises(ValueError, match="DeviceMixedSGD does not offer"):
            DeviceMixedSGD([param()], lr=0.1, **kw)
    for kw in ({"lr": -1.0}, {"lr": 0.1, "momentum": -0.5}, {"lr": 0.1, "weight_decay": -1e-4}):
        with pytest.raises(ValueError, match="Invalid"):
            DeviceMixedSGD([param()], **kw)
    # a gradient of another dtype than its parameter's
    p, g32, g16 = param(torch.bfloat16), torch.zeros(3), torch.zeros(3, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="gradient of its parameter's dtype, got torch.float32 for a torch.bfloat16"):
        DeviceMixedSGD._check_grad(p, g32)
    with pytest.raises(ValueError, match="gradient of its parameter's dtype, got torch.bfloat16 for a torch.float32"):
        DeviceMixedSGD._check_grad(param(), g16)
    DeviceMixedSGD._check_grad(p, g16)
    # DeviceSGD is as it was
    with pytest.raises(ValueError, match=r"DeviceSGD takes float32 parameters, got torch.bfloat16 \(bf16 parameters with fp32 "
                                         "masters are not offered\\)"):
        DeviceSGD([param(torch.bfloat16)], lr=0.1)
    with pytest.raises(ValueError, match="DeviceSGD takes at most 8 parameter groups, got 9"):
        DeviceSGD([{"params": [param()]} for _ in range(9)], lr=0.1)
    with pytest.raises(ValueError, match="DeviceSGD does not offer"):
        DeviceSGD([param()], lr=0.1, nesterov=True)


class SmallNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        import inplace_abn
        from ccnet_amd import abn
        self.conv = torch.nn.Conv2d(3, 4, 3, bias=True)
        self.shim = inplace_abn.InPlaceABNSync(4)
        self.device_abn = abn.ABN(4)
        self.device_inplace = abn.InPlaceABNSync(4)
        self.bn = torch.nn.BatchNorm2d(4)
        self.linear = torch.nn.Linear(4, 2)
        self.scale = torch.nn.Parameter(torch.ones(1))
        self.register_buffer("steps", torch.zeros(1))
        self.index = torch.nn.Parameter(torch.zeros(2, dtype=torch.int64), requires_grad=False)


def test_bf16_parameters_casts_all_but_the_normalisation_layers_in_place():
    import ccnet_amd
    from ccnet_amd.optim import bf16_parameters
    assert ccnet_amd.bf16_parameters is bf16_parameters
    net = SmallNet()
    before = dict(net.named_parameters())
    net.conv.weight.grad = torch.zeros_like(net.conv.weight)
    assert bf16_parameters(net) is net
    after = dict(net.named_parameters())
    assert all(after[k] is before[k] for k in before)                           # the Parameter objects stay
    for name, p in after.items():
        norm = name.split(".")[0] in ("shim", "device_abn", "device_inplace", "bn")
        want = torch.int64 if name == "index" else torch.float32 if norm else torch.bfloat16
        assert p.dtype == want, name
    assert {"shim.weight", "device_abn.bias", "device_inplace.weight", "bn.bias", "conv.bias", "linear.weight", "scale"} <= set(after)
    assert all(b.dtype == torch.float32 for n, b in net.named_buffers() if "running" in n or n == "steps")
    assert net.conv.weight.grad is None and net.conv.weight.requires_grad and not net.index.requires_grad
    assert bf16_parameters(net) is net and net.linear.weight.dtype == torch.bfloat16          # a second call changes nothing


def test_train_driver_takes_bf16_params_and_refuses_bf16_device_sgd_and_the_cpu(capsys):
    from ccnet_amd.train_synthetic import build_parser, check_args, parse_args, run
    assert build_parser().parse_args([]).bf16_params is False
    for flags in ([], ["--ohem"], ["--lovasz"], ["--fused-dsn"], ["--fused-ohem"], ["--fused-lovasz"], ["--abn", "device"],
                  ["--abn", "inplace"], ["--device-augment"]):
        assert parse_args(["--bf16-params"] + flags).bf16_params
    for other, words in ((["--bf16"], "cannot be combined with --bf16"), (["--device-sgd"], "cannot be combined with --device-sgd"),
                         (["--cpu"], "cannot be combined with --cpu")):
        with pytest.raises(ValueError, match=words):
            check_args(build_parser().parse_args(["--bf16-params"] + other))
        with pytest.raises(SystemExit):
            parse_args(["--bf16-params"] + other)
        assert words in capsys.readouterr().err
    with pytest.raises(ValueError, match="no CPU fallback"):
        run(build_parser().parse_args(["--bf16-params", "--cpu", "--steps", "1", "--warmup", "0"]),
            model_factory=lambda: torch.nn.Linear(2, 2))
    # without the flag nothing of it is in the way
    assert parse_args(["--bf16", "--device-sgd"]).bf16_params is False
