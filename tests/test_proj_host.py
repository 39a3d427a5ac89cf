"""CPU-side checks of libccnet_proj.so (include/ccnet_proj.h) and of the module route built on it: the build step, the exported
symbol set, the gfx950 code object and its resource metadata, argument validation (which happens before any launch, so it needs
no device), the row planner and the routing table."""
import ctypes
import os

import pytest
import torch

import lib_checks as L
from conftest import ROOT

KERNELS = ("gemm_bf16_kernel", "pack_kernel", "colsum_slab_kernel", "colsum_finish_kernel")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()                      # hipcc cross-compiles gfx950 without a GPU
    from ccnet_amd import _proj_lib
    assert os.path.exists(_proj_lib.LIB_PATH)
    return _proj_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _proj_lib
    return _proj_lib.ProjLibrary(lib_path)


def test_build_produces_the_library_with_exactly_the_declared_symbols(lib_path, lib):
    from ccnet_amd import _proj_lib
    names = _proj_lib.declared_symbols()
    assert len(names) == 7 and set(names) == set(_proj_lib._PROTOTYPES)
    exported = L.exported_symbols(lib_path)
    assert exported == sorted(names), sorted(set(exported) ^ set(names))
    assert lib.ccnet_proj_version() == _proj_lib.CCNET_PROJ_VERSION == 100 and lib.ccnet_proj_arch() == b"gfx950"


def test_build_leaves_the_attention_library_alone(lib_path):
    """a library of its own: nothing of it is a symbol of libccnet_cca.so, whose sources it only reads"""
    from ccnet_amd import _lib
    assert not any("ccnet_proj" in name for name in L.exported_symbols(_lib.LIB_PATH))
    import __graft_entry__ as g
    assert g.PROJ_LIB == lib_path and g.PROJ_CSRC not in g.HIPCC_FLAGS


def test_library_contains_the_gfx950_kernels(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


def test_new_kernels_have_no_scratch_and_no_spilled_vgprs(lib_path, tmp_path):
    assert L.HAVE_LLVM_BINUTILS, "the LLVM binutils of the ROCm installation are needed"
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN4proj")
    for k in KERNELS:
        assert any(k in n for n in kernels), (k, sorted(kernels))
    assert sum("gemm_bf16_kernel" in n for n in kernels) == 2              # with and without the K tail
    for n, meta in kernels.items():
        assert meta.get("private_segment_fixed_size", 0) == 0 and meta.get("vgpr_spill_count", 0) == 0, (n, meta)
        if "gemm_bf16_kernel" in n:
            assert meta["vgpr_count"] <= 256, meta                              # one workgroup of 8 wavefronts per CU: 2 per SIMD


def test_contract_violations_are_errors_before_any_launch(lib):
    """no device is needed: every call below is refused by the argument checks"""
    from ccnet_amd import _proj_lib as P
    a = (ctypes.c_uint16 * 64)()
    p = ctypes.addressof(a)
    gemm = lib.ccnet_proj_gemm_bf16
    assert gemm(None, p, None, None, p, 8, 8, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_NULLPTR
    assert gemm(p, None, None, None, p, 8, 8, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_NULLPTR
    assert gemm(p, p, None, None, None, 8, 8, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_NULLPTR
    assert "ccnet_proj" in lib.last_error() and "null" in lib.last_error()
    assert gemm(p, p, None, None, p, 8, 8, 12, 16, 16, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE          # K % 8
    assert gemm(p, p, None, None, p, 8, 6, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE             # N % 4
    assert gemm(p, p, None, None, p, 8, 8, 8, 12, 8, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE            # lda % 8
    assert gemm(p, p, None, None, p, 8, 8, 8, 8, 20, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE            # ldw % 8
    assert gemm(p, p, None, None, p, 8, 8, 8, 8, 8, 0, 10, None) == P.CCNET_PROJ_E_BADSHAPE            # ldo % 4
    assert gemm(p, p, None, p, p, 8, 8, 8, 8, 8, 10, 8, None) == P.CCNET_PROJ_E_BADSHAPE               # ldadd % 4
    assert gemm(p, p, None, None, p, 8, 16, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE            # ldo < N
    assert gemm(p, p, None, None, p, 0, 8, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE
    assert gemm(p + 2, p, None, None, p, 8, 8, 8, 8, 8, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE         # a 2-byte aligned pointer
    # byte offsets: M * lda = 2^30 elements is one too many, for each of the row-strided operands
    assert gemm(p, p, None, None, p, 1 << 21, 8, 512, 512, 512, 0, 8, None) == P.CCNET_PROJ_E_BADSHAPE
    assert "2^31" in lib.last_error()
    assert gemm(p, p, None, None, p, 1 << 21, 8, 8, 8, 8, 0, 512, None) == P.CCNET_PROJ_E_BADSHAPE
    assert gemm(p, p, None, p, p, 1 << 21, 8, 8, 8, 8, 512, 8, None) == P.CCNET_PROJ_E_BADSHAPE
    assert gemm(p, p, None, None, p, 8, 1 << 21, 512, 512, 512, 0, 1 << 21, None) == P.CCNET_PROJ_E_BADSHAPE
    pack = lib.ccnet_proj_pack
    assert pack(p, p, p, p, p, None, 0, p, p, p, 8, 1, None) == P.CCNET_PROJ_E_NULLPTR
    assert pack(p, p, p, p, p, p, 2, p, p, p, 8, 1, None) == P.CCNET_PROJ_E_BADFLAGS
    assert pack(p, p, p, p, p, p, 0, p, p, p, 0, 1, None) == P.CCNET_PROJ_E_BADSHAPE
    colsum = lib.ccnet_proj_colsum_bf16
    need = lib.ccnet_proj_colsum_workspace_bytes(4097, 80)
    assert need > 0 and need % (80 * 8) == 0 and lib.ccnet_proj_colsum_workspace_bytes(0, 80) == 0
    assert lib.ccnet_proj_colsum_workspace_bytes(4097, 80) == need                                      # a function of the shape alone
    assert colsum(None, p, 8, 8, 8, p, 1 << 20, None) == P.CCNET_PROJ_E_NULLPTR
    assert colsum(p, p, 8, 6, 8, p, 1 << 20, None) == P.CCNET_PROJ_E_BADSHAPE
    assert colsum(p, p, 8, 8, 10, p, 1 << 20, None) == P.CCNET_PROJ_E_BADSHAPE
    assert colsum(p, p, 1 << 21, 8, 512, p, 1 << 30, None) == P.CCNET_PROJ_E_BADSHAPE
    assert colsum(p, p, 4097, 80, 80, None, need, None) == P.CCNET_PROJ_E_WORKSPACE
    assert colsum(p, p, 4097, 80, 80, p, need - 8, None) == P.CCNET_PROJ_E_WORKSPACE
    assert "workspace" in lib.last_error()


def test_row_planner_cuts_whole_tiles_under_the_offset_limit():
    from ccnet_amd._proj_lib import MAX_ELEMS, TILE_ROWS, gemm_contract_ok, plan_rows
    assert plan_rows(266256, 512, 640) == [(0, 266256)]                      # BASELINE configs[4]: one launch
    assert plan_rows(1, 8, 8) == [(0, 1)] and plan_rows(0, 8, 8) == []
    for M, lda, ldo, ldadd in [(5_000_000, 512, 640, 0), (5_000_000, 640, 512, 512), (3_000_001, 2048, 8, 0), (1 << 22, 8, 8, 1 << 12)]:
        plan = plan_rows(M, lda, ldo, ldadd)
        assert len(plan) > 1 and plan[0][0] == 0 and sum(r for _, r in plan) == M
        for i, (m0, rows) in enumerate(plan):
            assert rows > 0 and rows * max(lda, ldo, ldadd) < MAX_ELEMS
            assert m0 == sum(r for _, r in plan[:i])
            assert rows % TILE_ROWS == 0 or i == len(plan) - 1
        assert plan[0][1] + TILE_ROWS > (MAX_ELEMS - 1) // max(lda, ldo, ldadd) - TILE_ROWS     # ... and no smaller than they must be
    assert plan_rows(1000, 1 << 23, 8) == []                                 # not even one tile fits: the caller's error
    assert gemm_contract_ok(640, 512, 512, 512, 640) and gemm_contract_ok(512, 640, 640, 640, 512, 512)
    assert not gemm_contract_ok(44, 36, 36, 36, 44)                          # C = 36: K % 8
    assert not gemm_contract_ok(640, 512, 512, 512, 642) and not gemm_contract_ok(640, 512, 516, 512, 640)


def test_route_takes_the_library_projections_only_when_asked_and_covered(lib_path):
    from ccnet_amd import CrissCrossAttention
    assert CrissCrossAttention.library_bf16_projections is False
    assert len(CrissCrossAttention.ROUTES) == 5 and "bf16-pixel-major-lib" in CrissCrossAttention.ROUTES
    m = CrissCrossAttention(64).to(torch.bfloat16)
    cl = torch.empty(2, 64, 129, 129, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    nchw = torch.empty(2, 64, 20, 24, dtype=torch.bfloat16)
    assert m.route(cl) == "bf16-pixel-major" and m.route(nchw) == "bf16-pixel-major"
    m.library_bf16_projections = True
    assert m.route(cl) == "bf16-pixel-major-lib" and m.route(nchw) == "bf16-pixel-major-lib"
    assert CrissCrossAttention.library_bf16_projections is False                          # (an instance attribute)
    # everything else keeps its route with the attribute on
    assert m.route(torch.empty(1, 64, 129, 257, dtype=torch.bfloat16)) == "f32-planes-cast"
    assert m.route(torch.empty(1, 64, 600, 9, dtype=torch.bfloat16)) == "separate-strips"
    m.fuse_projections = False
    assert m.route(cl) == "separate-strips"
    m.fuse_projections = True
    m.float()
    assert m.route(torch.empty(2, 64, 20, 24)) == "f32-planes"
    assert m.route(torch.empty(2, 64, 20, 24, dtype=torch.bfloat16)) != "bf16-pixel-major-lib"      # fp32 parameters without autocast
    # C = 36 is outside the GEMM's contract (K % 8): what the attribute-off module returns
    off, on = CrissCrossAttention(36).to(torch.bfloat16), CrissCrossAttention(36).to(torch.bfloat16)
    on.library_bf16_projections = True
    for x in (torch.empty(1, 36, 9, 7, dtype=torch.bfloat16), torch.empty(2, 36, 20, 24, dtype=torch.bfloat16)):
        assert on.route(x) == off.route(x) != "bf16-pixel-major-lib"
