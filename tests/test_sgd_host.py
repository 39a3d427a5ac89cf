"""CPU checks of the optimiser library (include/ccnet_sgd.h, ccnet_amd/csrc_sgd/, ccnet_amd/optim.py): the shipped gfx950
library's surface and its place in the build table, the chunk plan against hand values, every refusal without a device (through
the emulator build, on guarded buffers), the poly schedule bit for bit, and what DeviceSGD refuses before it touches a device."""
import os
import re

import numpy as np
import pytest
import torch

import lib_checks as L
import sgd_oracle as S
from conftest import ROOT
from guarded_memory import HostMemory

CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_sgd")
C = S.C


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _sgd_lib
    return _sgd_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _sgd_lib
    return _sgd_lib.SgdLibrary(lib_path)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._sgd_lib import SgdLibrary
    return SgdLibrary(L.build_shared_scaffold_emu("sgd"))


def test_build_table_keeps_its_pinned_lists_and_the_library_is_a_later_unit():
    import __graft_entry__ as g
    rows = [u for e in g.EXTENSIONS for u in e.libraries()]
    assert len(g.EXTENSIONS) == 7 and len(rows) == 9
    assert [e.name for e in g.SECOND_UNITS] == ["celovasz", "augment"] and g.all_libraries() == rows + g.SECOND_UNITS
    assert [e.name for e in g.LATER_UNITS] == ["sgd"] and "sgd" not in [u.name for u in g.all_libraries()]
    unit = g.LATER_UNITS[0]
    assert unit.csrc == CSRC and unit.binding == "_sgd_lib" and unit.exports == os.path.join(CSRC, "exports.map")
    assert unit.unit == os.path.join(CSRC, "sgd_api.hip") and unit.header.endswith("ccnet_sgd.h")
    assert g.SGD_CSRC == CSRC and g.SGD_LIB == os.path.join(CSRC, "libccnet_sgd.so")
    assert g.SGD_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-I" + CSRC,
                                                 "-I" + os.path.join(ROOT, "include")]
    assert os.path.join(ROOT, "ccnet_amd", "csrc_common", "ccnet_host.hpp") in unit.sources()


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _sgd_lib
    names = _sgd_lib.declared_symbols()
    assert names == sorted(["ccnet_sgd_version", "ccnet_sgd_arch", "ccnet_sgd_last_error_string", "ccnet_sgd_plan",
                            "ccnet_sgd_step"])
    assert set(names) == set(_sgd_lib._PROTOTYPES)
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code_and_the_binding_mirrors_the_header(lib_path, lib):
    from ccnet_amd import _sgd_lib as m
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"_ZN3sgd11step_kernel" in blob and b"_ZN3sgd14advance_kernel" in blob
    assert lib.ccnet_sgd_version() == 100 == m.CCNET_SGD_VERSION and lib.ccnet_sgd_arch() == b"gfx950"
    header = open(m.HEADER_PATH).read()
    for name, value in (("VERSION", 100), ("CHUNK", m.CHUNK), ("MAX_GROUPS", m.MAX_GROUPS), ("MAX_TENSORS", m.MAX_TENSORS),
                        ("DEFAULT_CAP", m.DEFAULT_CAP), ("TENSOR_WORDS", m.TENSOR_WORDS), ("P", m.P), ("G", m.G), ("B", m.B),
                        ("NUMEL", m.NUMEL), ("GROUP", m.GROUP)):
        assert re.search(rf"#define CCNET_SGD_{name}\s+{value}\b", header), name
    assert (m.MAX_GROUPS, m.MAX_TENSORS, m.TENSOR_WORDS) == (8, 65535, 5) and m.CHUNK in (4096, 16384)
    assert (m.P, m.G, m.B, m.NUMEL, m.GROUP) == (0, 1, 2, 3, 4)


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_the_kernels_use_no_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN3sgd")
    assert len(kernels) == 2, sorted(kernels)
    assert not L.kernels_using_scratch(kernels)


def test_sources_carry_no_env_knobs_no_emulator_code_no_atomics_and_no_copies():
    files = L.product_sources(CSRC)
    assert set(files) == {"sgd_api.hip", "sgd_kernels.hpp", "sgd_platform.hpp"}
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomicAdd" not in text and "__shared__" not in text and "asm volatile" not in text, f
        assert "hipMemcpy" not in text and "Synchronize" not in text and "hipMalloc" not in text, f       # nothing is read back
    assert "#pragma clang fp contract(off)" in files["sgd_kernels.hpp"]


def test_binding_refuses_a_missing_library_and_another_abi_version(lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _sgd_lib as m
    assert issubclass(m.SgdError, RuntimeError)
    with pytest.raises(m.SgdError, match="not found"):
        m.SgdLibrary(str(tmp_path / "libccnet_missing.so"))
    monkeypatch.setattr(m, "CCNET_SGD_VERSION", m.CCNET_SGD_VERSION + 1)
    with pytest.raises(m.SgdError, match="rebuild"):
        m.SgdLibrary(m.LIB_PATH)


HAND_PLANS = [([1], [(0, 0)]), ([C], [(0, 0)]), ([C + 1], [(0, 0), (0, 1)]),
              ([1, 3, 2 * C + 3], [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)])]


@pytest.mark.parametrize("sizes,want", HAND_PLANS, ids=["1", "C", "C+1", "model-like"])
def test_plan_against_hand_values(lib, sizes, want):
    got = lib.plan(sizes)
    assert got.dtype == np.int32 and got.tolist() == [list(w) for w in want]
    assert np.array_equal(S.plan(sizes), got)


def test_plan_counts_without_a_table_and_refuses_its_limits(lib):
    from ctypes import c_int64
    n = c_int64(-7)
    numel = np.array([5, 3 * C, 2 ** 31 - 1], np.int64)
    assert lib.ccnet_sgd_plan(numel.ctypes.data, 3, None, 0, n) == 0 and n.value == 1 + 3 + (2 ** 31 - 1 + C - 1) // C
    small = np.zeros((2, 2), np.int32)
    assert lib.ccnet_sgd_plan(numel.ctypes.data, 2, small.ctypes.data, 2, n) == -5 and "room for 2" in lib.last_error()
    assert not small.any()
    for bad in (0, -1, 2 ** 31):
        numel[1] = bad
        assert lib.ccnet_sgd_plan(numel.ctypes.data, 3, None, 0, n) == -3 and "outside 1..2^31-1" in lib.last_error()
    assert lib.ccnet_sgd_plan(numel.ctypes.data, 0, None, 0, n) == -1 and lib.ccnet_sgd_plan(numel.ctypes.data, 65536, None, 0, n) == -1
    assert lib.ccnet_sgd_plan(None, 1, None, 0, n) == -2 and lib.ccnet_sgd_plan(numel.ctypes.data, 1, None, 0, None) == -2
    assert lib.last_error().startswith("ccnet_sgd: plan")


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


REFUSALS = [
    ("null_tensors_host", "tails", set_("tensors_host", None), -2, "NULL tensor table"),
    ("null_tensors_device", "tails", set_("tensors_device", None), -2, "NULL tensor table"),
    ("null_chunks_host", "tails", set_("chunks_host", None), -2, "NULL tensor table or chunk table"),
    ("null_chunks_device", "tails", set_("chunks_device", None), -2, "NULL tensor table or chunk table"),
    ("null_lr", "tails", set_("lr", None), -2, "NULL lr"),
    ("no_tensors", "tails", set_("n_tensors", 0), -1, "0 tensors"),
    ("too_many_tensors", "tails", set_("n_tensors", 65536), -1, "65536 tensors"),
    ("numel_zero", "tails", table(2, 3, 0), -3, "tensor 2 has 0 elements"),
    ("numel_negative", "tails", table(2, 3, -4), -3, "tensor 2 has -4 elements"),
    ("numel_2_31", "tails", table(7, 3, 2 ** 31), -3, "tensor 7 has 2147483648 elements"),
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
    ("null_p", "tails", table(4, 0, 0), -8, "tensor 4 has a NULL parameter"),
    ("null_b", "tails", table(5, 2, 0), -8, "tensor 5 has a NULL parameter or momentum buffer"),
    ("p_misaligned", "tails", add_to_table(1, 0, 2), -8, "tensor 1 has a parameter, gradient or momentum buffer that is not 4-byte"),
    ("b_misaligned", "tails", add_to_table(6, 2, 1), -8, "tensor 6 has a parameter, gradient or momentum buffer that is not 4-byte"),
]


@pytest.mark.parametrize("case_name,mutate,code,words", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_every_refusal_has_its_code_and_text_and_writes_nothing(emu, case_name, mutate, code, words):
    case = S.build_case(case_name)
    got_code, got, intact = S.run_raw(emu, HostMemory(), case, mutate)
    assert got_code == code, emu.last_error()
    assert emu.last_error().startswith("ccnet_sgd: step: ") and words in emu.last_error(), emu.last_error()
    assert intact and S.unchanged(case, got)


def test_poly_schedule_is_lr_poly_rounded_once():
    from ccnet_amd.optim import poly_schedule
    from ccnet_amd.train_synthetic import lr_poly
    table = poly_schedule(1e-2, 100)
    assert table.dtype == torch.float32 and tuple(table.shape) == (100,) and table.device.type == "cpu"
    for it in (0, 50, 99):
        assert table[it].numpy().view(np.uint32) == np.float32(lr_poly(1e-2, it, 100)).view(np.uint32), it
    assert np.array_equal(table.numpy(), np.array([np.float32(lr_poly(1e-2, it, 100)) for it in range(100)]))
    assert float(poly_schedule(0.5, 1)[0]) == 0.5 and float(poly_schedule(1e-2, 4, power=1.0)[2]) == float(np.float32(0.005))
    with pytest.raises(ValueError, match="max_iter"):
        poly_schedule(1e-2, 0)


def test_device_sgd_refuses_cpu_tensors_other_dtypes_and_a_ninth_group():
    import ccnet_amd
    from ccnet_amd.optim import DeviceSGD
    assert ccnet_amd.DeviceSGD is DeviceSGD and issubclass(DeviceSGD, torch.optim.Optimizer)
    param = lambda dtype=torch.float32: torch.nn.Parameter(torch.zeros(3, dtype=dtype))          # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        DeviceSGD([param()], lr=0.1)
    with pytest.raises(ValueError, match="float32 parameters"):
        DeviceSGD([param(torch.bfloat16)], lr=0.1)
    with pytest.raises(ValueError, match="at most 8 parameter groups, got 9"):
        DeviceSGD([{"params": [param()]} for _ in range(9)], lr=0.1)
    for kw in ({"dampening": 0.1}, {"nesterov": True}, {"maximize": True}):
        with pytest.raises(ValueError, match="does not offer"):
            DeviceSGD([param()], lr=0.1, **kw)
    with pytest.raises(ValueError, match="Invalid"):
        DeviceSGD([param()], lr=-1.0)


def test_train_driver_takes_device_sgd_with_every_other_flag_and_refuses_the_cpu():
    from ccnet_amd.train_synthetic import build_parser, parse_args, run
    assert build_parser().parse_args([]).device_sgd is False
    for flags in ([], ["--ohem"], ["--lovasz"], ["--fused-dsn"], ["--fused-ohem"], ["--fused-lovasz"], ["--abn", "device"],
                  ["--bf16"], ["--device-augment"]):
        assert parse_args(["--device-sgd"] + flags).device_sgd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(build_parser().parse_args(["--device-sgd", "--cpu", "--steps", "1", "--warmup", "0"]),
            model_factory=lambda: torch.nn.Linear(2, 2))
