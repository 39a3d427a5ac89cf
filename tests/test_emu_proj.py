"""libccnet_proj.so's kernels in the SIMT emulator: ccnet_amd/csrc_proj/proj_api.hip compiled for the host against tests/emu/ and
tests/emu_proj/ (the emulator twins of the platform headers, first on the include path), driven through the same binding as
the device library on numpy buffers.  The case table and its bars live in tests/proj_cases.py; tests/test_gpu_proj.py runs the
same table on the device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import proj_cases as K  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402
from lib_checks import INCLUDE, build_emu_library  # noqa: E402

ROOT = os.path.dirname(HERE)
EMU_DIR, EMU_PROJ_DIR = os.path.join(HERE, "emu"), os.path.join(HERE, "emu_proj")
CSRC, PROJ_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc"), os.path.join(ROOT, "ccnet_amd", "csrc_proj")
EMU_LIB = os.path.join(EMU_PROJ_DIR, "libproj_emu.so")


def build_emu():
    return build_emu_library(EMU_LIB, os.path.join(PROJ_CSRC, "proj_api.hip"),
                             [EMU_DIR, EMU_PROJ_DIR, PROJ_CSRC, CSRC, INCLUDE])            # the emulator's headers FIRST


@pytest.fixture(scope="module")
def lib():
    from ccnet_amd._proj_lib import ProjLibrary
    return ProjLibrary(build_emu())


@pytest.fixture(scope="module")
def mem():
    return HostMemory()


@pytest.mark.parametrize("cid,variant", K.gemm_ids(), ids=lambda v: v)
def test_gemm_case_table(lib, mem, cid, variant):
    K.run_gemm(lib, mem, cid, variant)


@pytest.mark.parametrize("M,n", K.PLACEMENT_CASES)
def test_gemm_with_identity_weight_copies_its_input(lib, mem, M, n):
    K.run_placement(lib, mem, M, n)


@pytest.mark.parametrize("mnk", K.EPILOGUE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_gemm_of_zero_rows_is_the_rounded_bias_plus_addend(lib, mem, mnk):
    K.run_epilogue(lib, mem, mnk)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("C,cq", K.PACK_CASES)
def test_pack_matches_numpy(lib, mem, C, cq, f32):
    K.run_pack(lib, mem, C, cq, f32)


@pytest.mark.parametrize("M,N,extra", K.COLSUM_CASES)
def test_column_sums(lib, mem, M, N, extra):
    K.run_colsum(lib, mem, M, N, extra)
