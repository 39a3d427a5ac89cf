"""CPU-side checks of libccnet_conv3.so (include/ccnet_conv3.h) and of the layer built on it (ccnet_amd/conv3.py): the oracle
against torch in fp64, the build row, the exported symbol set, the gfx950 code object and its resource metadata, the hazard walk
over its assembly, argument validation (before any launch, so it needs no device), the image planner, the eligibility table of
``convert_conv3x3`` on the full model, ``state_dict`` parity and what the function and the driver refuse."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv3_oracle as O
import isa_hazards as H
import lib_checks as L
from conftest import ROOT

CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_conv3")
KERNELS = ("conv3_bf16_kernel", "conv3_wgrad_kernel", "pack_kernel", "wgrad_finish_kernel")


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4, 1), (1, 6, 4, 5, 2, 2), (2, 3, 9, 2, 3, 4)], ids=lambda s: "x".join(map(str, s)))
def test_oracle_matches_torch_conv2d_and_autograd_in_fp64(shape):
    B, H, W, ci, co, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, ci, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(co, ci, 3, 3, dtype=torch.float64, generator=g, requires_grad=True)
    b = torch.randn(co, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(B, co, H, W, dtype=torch.float64, generator=g)
    y = F.conv2d(x, w, b, stride=1, padding=d, dilation=d)
    y.backward(dy)
    pm = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().numpy()          # noqa: E731
    xn, dyn, wn = pm(x), pm(dy), w.detach().numpy()
    for name, got, want in (("y", O.forward(xn, wn, b.detach().numpy(), d), pm(y)), ("dx", O.input_grad(dyn, wn, d), pm(x.grad)),
                            ("dW", O.weight_grad(dyn, xn, d), w.grad.numpy()), ("db", O.bias_grad(dyn), b.grad.numpy())):
        err = float(np.abs(got - want).max())
        print(name, f"{err:.3e}")
        assert got.shape == want.shape and err <= 1e-12 * max(1.0, float(np.abs(want).max())), (name, err)


def test_packs_are_the_index_permutations_the_header_states():
    w = np.arange(5 * 3 * 9).reshape(5, 3, 3, 3)
    fwd, adj = O.pack_forward(w), O.pack_adjoint(w)
    assert fwd.shape == (5, 27) and adj.shape == (3, 45)
    for n, c, t in [(0, 0, 0), (4, 2, 8), (2, 1, 5), (3, 0, 7)]:
        assert fwd[n, t * 3 + c] == w[n, c, t // 3, t % 3] and adj[c, t * 5 + n] == w[n, c, (8 - t) // 3, (8 - t) % 3]


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()                      # hipcc cross-compiles gfx950 without a GPU
    from ccnet_amd import _conv3_lib
    assert os.path.exists(_conv3_lib.LIB_PATH)
    return _conv3_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _conv3_lib
    return _conv3_lib.Conv3Library(lib_path)


def test_the_library_is_a_row_like_projs_and_the_pinned_lists_stay():
    import __graft_entry__ as g
    assert [e.name for e in g.CONV_UNITS] == ["conv3"] and "conv3" not in [u.name for u in g.all_libraries() + g.LATER_UNITS + g.MIXED_UNITS]
    assert len(g.all_libraries() + g.LATER_UNITS + g.MIXED_UNITS) == 13
    unit = g.CONV_UNITS[0]
    assert unit.csrc == CSRC and unit.binding == "_conv3_lib" and unit.exports == os.path.join(CSRC, "exports.map")
    assert unit.unit == os.path.join(CSRC, "conv3_api.hip") and unit.header.endswith("ccnet_conv3.h")
    assert g.CONV3_CSRC == CSRC and g.CONV3_LIB == os.path.join(CSRC, "libccnet_conv3.so")
    assert g.CONV3_HIPCC_FLAGS == [f.replace("csrc_proj", "csrc_conv3") for f in g.PROJ_HIPCC_FLAGS]          # the same rule
    assert "-I" + g.CSRC in g.CONV3_HIPCC_FLAGS and "-I" + os.path.join(ROOT, "include") in g.CONV3_HIPCC_FLAGS
    assert os.path.join(g.CSRC, "cca_gemm.hpp") in unit.sources() and os.path.join(g.CSRC, "cca_platform.hpp") in unit.sources()
    assert g.CONV3_CSRC not in g.HIPCC_FLAGS and g.CONV3_CSRC not in " ".join(g.PROJ_HIPCC_FLAGS)


def test_build_produces_the_library_with_exactly_the_declared_symbols(lib_path, lib):
    from ccnet_amd import _conv3_lib
    names = _conv3_lib.declared_symbols()
    assert len(names) == 9 and set(names) == set(_conv3_lib._PROTOTYPES)
    exported = L.exported_symbols(lib_path)                                       # nm -D, both ways
    assert exported == sorted(names), sorted(set(exported) ^ set(names))
    assert lib.ccnet_conv3_version() == _conv3_lib.CCNET_CONV3_VERSION == 100 and lib.ccnet_conv3_arch() == b"gfx950"


def test_build_leaves_the_other_libraries_alone(lib_path):
    from ccnet_amd import _lib, _proj_lib
    for other in (_lib.LIB_PATH, _proj_lib.LIB_PATH):
        assert not any("ccnet_conv3" in name for name in L.exported_symbols(other))
    files = L.product_sources(CSRC)
    assert set(files) == {"conv3_api.hip", "conv3_kernels.hpp", "conv3_platform.hpp"}
    for f, text in files.items():
        assert "getenv" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomic" not in text and "hipMemcpy" not in text and "Synchronize" not in text and "hipMalloc" not in text, f


def test_library_contains_the_gfx950_kernels(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


def test_kernels_have_no_scratch_and_no_spilled_registers(lib_path, tmp_path):
    assert L.HAVE_LLVM_BINUTILS, "the LLVM binutils of the ROCm installation are needed"
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN5conv3")
    for k in KERNELS:
        assert any(k in n for n in kernels), (k, sorted(kernels))
    assert sum("conv3_bf16_kernel" in n for n in kernels) == 2                 # with and without the K tail
    assert len(kernels) == 7, sorted(kernels)
    assert not L.kernels_using_scratch(kernels), L.kernels_using_scratch(kernels)
    # csrc/cca_gemm.hpp, which the kernels read for the tile geometry, defines non-template kernels of the attention library
    # (its weight-gradient GEMM, its layout producers); they are compiled into this code object too, as into libccnet_proj.so,
    # and never launched from here.  They are held to the same condition: every kernel of the code object
    every = L.code_object_kernels(lib_path, tmp_path, "_Z")
    assert set(kernels) <= set(every) and all(n.startswith(("_ZN5conv3", "_ZN3cca")) for n in every), sorted(every)
    assert not L.kernels_using_scratch(every), L.kernels_using_scratch(every)
    for n, meta in kernels.items():
        if "conv3_bf16_kernel" in n or "conv3_wgrad_kernel" in n:
            assert meta["vgpr_count"] <= 256, meta                              # one workgroup of 8 wavefronts per CU: 2 per SIMD


def test_no_instruction_touches_an_outstanding_lds_destination(tmp_path):
    """the existing hazard walk (tests/isa_hazards.py) over the new library's assembly: zero findings, and the convolution
    kernel's two KTAIL instantiations are among the kernels walked, with their uncounted fragment reads"""
    import __graft_entry__ as g
    flags = [f for f in g.CONV3_HIPCC_FLAGS if f not in ("-shared", "-fPIC") and not f.startswith("-Wl,")]
    out = str(tmp_path / "conv3.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, "conv3_api.hip"), "-o", out], check=True, cwd=CSRC)
    with open(out) as f:
        funcs = H.functions(f.read())
    assert funcs
    bad = {name: H.analyse(name, lines)[0] for name, lines in funcs.items()}
    bad = {name: r for name, r in bad.items() if r}
    assert not bad, {name: [(v.block, v.text, v.regs) for v in r[:4]] for name, r in bad.items()}
    for inst in ("ILb0E", "ILb1E"):
        names = [n for n in funcs if "conv3_bf16_kernel" + inst in n]
        assert len(names) == 1, (inst, sorted(funcs))
        assert H.count_mnemonic(funcs[names[0]], "ds_read_b128") >= 16, names[0]
    assert any("conv3_wgrad_kernel" in n for n in funcs)


def test_contract_violations_are_errors_before_any_launch(lib):
    """no device is needed: every call below is refused by the argument checks"""
    from ccnet_amd import _conv3_lib as P
    a = (ctypes.c_uint16 * 64)()
    p = ctypes.addressof(a)
    conv = lib.ccnet_conv3_bf16
    ok = dict(B=1, H=2, W=2, K=8, N=8, d=1, lda=8, ldadd=0, ldo=8)

    def call(a_=p, wt=p, bias=None, add=None, out=p, **kw):
        v = dict(ok, **kw)
        return conv(a_, wt, bias, add, out, v["B"], v["H"], v["W"], v["K"], v["N"], v["d"], v["lda"], v["ldadd"], v["ldo"], None)

    assert call(a_=None) == call(wt=None) == call(out=None) == P.CCNET_CONV3_E_NULLPTR
    assert "ccnet_conv3" in lib.last_error() and "null" in lib.last_error()
    for kw in (dict(K=12, lda=16), dict(N=6), dict(lda=12), dict(ldo=10), dict(ldo=4), dict(lda=0), dict(B=0), dict(H=0), dict(W=-1),
               dict(d=0), dict(add=p, ldadd=10), dict(add=p, ldadd=4), dict(a_=p + 2), dict(bias=p + 2)):
        assert call(**kw) == P.CCNET_CONV3_E_BADSHAPE, kw
    # byte offsets: B H W * stride = 2^30 elements is one too many, for each row-strided operand and for the weight
    assert call(B=1 << 10, H=1 << 6, W=1 << 5, K=512, lda=512) == P.CCNET_CONV3_E_BADSHAPE and "2^31" in lib.last_error()
    assert call(B=1 << 10, H=1 << 6, W=1 << 5, ldo=512) == P.CCNET_CONV3_E_BADSHAPE
    assert call(B=1 << 10, H=1 << 6, W=1 << 5, add=p, ldadd=512) == P.CCNET_CONV3_E_BADSHAPE
    assert call(K=1 << 14, lda=1 << 14, N=1 << 13, ldo=1 << 13) == P.CCNET_CONV3_E_BADSHAPE
    pack = lib.ccnet_conv3_pack
    assert pack(None, 0, p, p, 8, 8, None) == pack(p, 0, None, p, 8, 8, None) == pack(p, 0, p, None, 8, 8, None) == P.CCNET_CONV3_E_NULLPTR
    assert pack(p, 2, p, p, 8, 8, None) == P.CCNET_CONV3_E_BADFLAGS and pack(p, 0, p, p, 0, 8, None) == P.CCNET_CONV3_E_BADSHAPE
    wgrad, need = lib.ccnet_conv3_wgrad_bf16, lib.ccnet_conv3_wgrad_workspace_bytes
    assert need(2, 9, 15, 64, 64, 2) == 2 * 9 * 64 * 64 * 4 and need(0, 9, 15, 64, 64, 2) == 0 and need(2, 9, 15, 60, 64, 2) == 0
    S = lib.ccnet_conv3_wgrad_slabs(2, 9, 15, 64, 64)
    assert S == 5 and need(2, 9, 15, 64, 64, 0) == S * 9 * 64 * 64 * 4                   # 270 rows: at least 64 rows per slab
    assert lib.ccnet_conv3_wgrad_slabs(1, 97, 97, 256, 256) == 14 and lib.ccnet_conv3_wgrad_slabs(1, 97, 97, 512, 2560) == 1
    nb = need(1, 2, 2, 8, 8, 1)
    assert wgrad(None, p, p, nb, 1, 2, 2, 8, 8, 1, 8, 8, 1, None) == P.CCNET_CONV3_E_NULLPTR
    assert wgrad(p, p, p, nb, 1, 2, 2, 12, 8, 1, 16, 8, 1, None) == P.CCNET_CONV3_E_BADSHAPE
    assert wgrad(p, p, p, nb, 1, 2, 2, 8, 8, 0, 8, 8, 1, None) == P.CCNET_CONV3_E_BADSHAPE
    assert wgrad(p, p, p, nb, 1, 2, 2, 8, 8, 1, 12, 8, 1, None) == P.CCNET_CONV3_E_BADSHAPE
    assert wgrad(p, p, p, nb, 1, 2, 2, 8, 8, 1, 8, 8, -1, None) == P.CCNET_CONV3_E_BADFLAGS
    assert wgrad(p, p, None, nb, 1, 2, 2, 8, 8, 1, 8, 8, 1, None) == P.CCNET_CONV3_E_WORKSPACE
    assert wgrad(p, p, p, nb - 4, 1, 2, 2, 8, 8, 1, 8, 8, 1, None) == P.CCNET_CONV3_E_WORKSPACE and "workspace" in lib.last_error()
    finish = lib.ccnet_conv3_wgrad_finish
    assert finish(None, p, 0, 8, 8, 1, None) == P.CCNET_CONV3_E_NULLPTR and finish(p, p, 3, 8, 8, 1, None) == P.CCNET_CONV3_E_BADFLAGS
    assert finish(p, p, 0, 8, 8, 0, None) == P.CCNET_CONV3_E_BADSHAPE


def test_image_planner_cuts_at_image_boundaries_under_the_offset_limit():
    from ccnet_amd._conv3_lib import MAX_ELEMS, plan_images
    assert plan_images(8, 97 * 97, 2560) == [(0, 8)] and plan_images(0, 4, 8) == []
    plan = plan_images(100, 97 * 97, 2560)
    assert len(plan) > 1 and plan[0][0] == 0 and sum(n for _, n in plan) == 100
    for i, (b0, n) in enumerate(plan):
        assert n > 0 and n * 97 * 97 * 2560 < MAX_ELEMS and b0 == sum(m for _, m in plan[:i])
    assert (plan[0][1] + 1) * 97 * 97 * 2560 >= MAX_ELEMS                  # ... and no smaller than they must be
    assert plan_images(2, 1 << 20, 1 << 11) == []                          # not even one image fits: the caller's error


# ---------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------
def test_eligibility_table_on_the_full_model():
    from ccnet_amd.conv3 import DeviceConv3x3, convert_conv3x3, eligible
    from ccnet_amd.segmodel import _RESNET101_STAGES, Seg_Model
    model = Seg_Model(19, recurrence=2)
    keys = list(model.state_dict().keys())
    # the stem's second and third convolution, every block's 3x3 but a stride-2 first block's, conva, convb, the bottleneck's, the DSN head's
    want = 2 + sum(blocks - (stride != 1) for _, blocks, stride, _ in _RESNET101_STAGES) + 3 + 1
    assert want == 38 and convert_conv3x3(model) == want
    assert type(model.conv1) is nn.Conv2d and type(model.layer2[0].conv2) is nn.Conv2d          # stride 2: stock
    assert all(type(m) is DeviceConv3x3 for m in (model.conv2, model.conv3, model.layer2[1].conv2, model.head.conva[0],
                                                  model.head.convb[0], model.head.bottleneck[0], model.dsn[0]))
    assert all(type(b.conv2) is DeviceConv3x3 and type(b.conv1) is nn.Conv2d and type(b.conv3) is nn.Conv2d
               for layer in (model.layer1, model.layer3, model.layer4) for b in layer)
    assert [b.conv2.dilation for b in model.layer3] == [(2, 2)] * 23 and [b.conv2.dilation for b in model.layer4] == [(4, 4)] * 3
    assert type(model.head.bottleneck[3]) is nn.Conv2d and model.dsn[0].bias is not None
    assert list(model.state_dict().keys()) == keys and convert_conv3x3(model) == 0            # nothing left to swap
    for bad in (nn.Conv2d(8, 8, 3, padding=1, stride=2), nn.Conv2d(8, 8, 3, padding=2), nn.Conv2d(8, 8, 3, padding=(1, 2), dilation=(1, 2)),
                nn.Conv2d(8, 8, 3, padding=1, groups=2), nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect"), nn.Conv2d(12, 8, 3, padding=1),
                nn.Conv2d(8, 12, 3, padding=1), nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 3, padding="same"), nn.Conv2d(8, 8, 5, padding=2)):
        assert not eligible(bad) and convert_conv3x3(bad) == 0, bad
    assert eligible(nn.Conv2d(8, 16, 3, padding=3, dilation=3)) and convert_conv3x3(nn.Sequential(nn.Conv2d(8, 16, 3, padding=1))) == 1


def test_state_dict_parity_with_conv2d_and_strict_loading_both_ways():
    from ccnet_amd.conv3 import DeviceConv3x3
    for bias in (True, False):
        stock, ours = nn.Conv2d(16, 24, 3, padding=2, dilation=2, bias=bias), DeviceConv3x3(16, 24, 3, padding=2, dilation=2, bias=bias)
        assert list(stock.state_dict().keys()) == list(ours.state_dict().keys())
        assert [n for n, _ in stock.named_parameters()] == [n for n, _ in ours.named_parameters()]
        assert ours.weight.shape == stock.weight.shape and isinstance(ours, nn.Conv2d)
        ours.load_state_dict(stock.state_dict(), strict=True)
        assert torch.equal(ours.weight, stock.weight)
        other = nn.Conv2d(16, 24, 3, padding=2, dilation=2, bias=bias)
        other.load_state_dict(ours.state_dict(), strict=True)
        assert torch.equal(other.weight, stock.weight)


def test_function_refuses_what_is_outside_its_contract_by_name():
    from ccnet_amd.conv3 import DeviceConv3x3, conv3x3
    bf = torch.bfloat16
    x, w = torch.zeros(1, 8, 4, 4, dtype=bf), torch.zeros(8, 8, 3, 3, dtype=bf)
    with pytest.raises(TypeError, match="float32"):
        conv3x3(x.float(), w)
    with pytest.raises(TypeError, match="weight is torch.float32"):
        conv3x3(x, w.float())                                               # fp32 parameters without autocast
    with pytest.raises(TypeError, match="bias"):
        conv3x3(x, w, torch.zeros(8))
    with pytest.raises(ValueError, match="Cin = 12"):
        conv3x3(torch.zeros(1, 12, 4, 4, dtype=bf), torch.zeros(8, 12, 3, 3, dtype=bf))
    with pytest.raises(ValueError, match="3, 3"):
        conv3x3(x, torch.zeros(8, 8, 1, 1, dtype=bf))
    with pytest.raises(ValueError, match="channels"):
        conv3x3(x, torch.zeros(8, 16, 3, 3, dtype=bf))
    with pytest.raises(ValueError, match="dilation"):
        conv3x3(x, w, dilation=0)
    with pytest.raises(ValueError, match="no CPU route"):
        conv3x3(x, w)
    with pytest.raises(ValueError, match="stride"):
        DeviceConv3x3(8, 8, 3, stride=2, padding=1).to(bf)(x)


def test_driver_flag_needs_bf16_and_refuses_device_abn_and_cpu():
    from ccnet_amd import train_synthetic as T
    parse = lambda *a: T.build_parser().parse_args(list(a))                     # noqa: E731
    for argv, word in ((("--device-conv3",), "--bf16"), (("--device-conv3", "--bf16", "--abn", "device"), "NCHW"),
                       (("--device-conv3", "--bf16-params", "--abn", "inplace"), "NCHW"), (("--device-conv3", "--bf16", "--cpu"), "--cpu")):
        with pytest.raises(ValueError, match=word):
            T.check_args(parse(*argv))
    T.check_args(parse("--device-conv3", "--bf16"))
    T.check_args(parse("--device-conv3", "--bf16-params", "--abn", "torch"))
    assert parse().device_conv3 is False


def test_native_batch_norm_swap_takes_only_the_observed_case_and_leaves_every_other_call_alone(monkeypatch):
    """the class swap ``--device-conv3`` applies to the stock normalisation layers: the predicate is bf16 + channels_last +
    float32 affine and nothing wider; off a HIP device, and for every other input, the layer makes inplace_abn's own
    F.batch_norm call and returns its bits; inplace_abn itself is untouched"""
    import inplace_abn

    from ccnet_amd import conv3
    bf, cl = torch.bfloat16, torch.channels_last
    w32 = torch.ones(8)
    x = torch.randn(2, 8, 5, 7)
    case = conv3.bf16_channels_last_fp32_affine
    assert case(x.to(bf).contiguous(memory_format=cl), w32)
    assert not case(x.to(bf), w32)                                              # NCHW
    assert not case(x.contiguous(memory_format=cl), w32)                        # float32
    assert not case(x.half().contiguous(memory_format=cl), w32)                 # fp16 was never seen to fault
    assert not case(x.to(bf).contiguous(memory_format=cl), w32.to(bf))          # bf16 affine parameters
    assert not case(x.to(bf).contiguous(memory_format=cl), None) and not case(x.to(bf)[0], w32)
    assert not case(torch.randn(2, 8, 1, 1).to(bf).contiguous(memory_format=cl), w32)      # also NCHW-contiguous
    src = open(inplace_abn.__file__).read()
    assert "cudnn" not in src and "channels_last" not in src
    for kind in ("ABN", "InPlaceABN", "InPlaceABNSync"):
        torch.manual_seed(1)
        stock, ours = (getattr(inplace_abn, kind)(8).train() for _ in range(2))
        assert conv3.native_batch_norm_for_bf16_channels_last(ours) == 1 and conv3.native_batch_norm_for_bf16_channels_last(ours) == 0
        assert isinstance(ours, getattr(inplace_abn, kind)) and type(ours).__name__ == kind + "NativeChannelsLast"
        assert list(ours.state_dict().keys()) == list(stock.state_dict().keys())
        calls = []
        real, flags = F.batch_norm, torch.backends.cudnn.flags
        monkeypatch.setattr(inplace_abn.F, "batch_norm", lambda *a, **k: (calls.append("F"), real(*a, **k))[1])
        monkeypatch.setattr(torch.backends.cudnn, "flags", lambda *a, **k: (calls.append("native"), flags(*a, **k))[1])
        try:
            for inp in (x, x.contiguous(memory_format=cl), x.to(bf).contiguous(memory_format=cl)):      # (CPU: never the new call)
                calls.clear()
                got, want = ours(inp), stock(inp)
                assert calls == ["F", "F"] and torch.equal(got, want)                     # no flag touched, the old call made
        finally:
            monkeypatch.undo()
    from ccnet_amd.abn import convert_abn
    dev_abn = convert_abn(torch.nn.Sequential(inplace_abn.InPlaceABNSync(8)), "device")
    assert conv3.native_batch_norm_for_bf16_channels_last(dev_abn) == 0          # the device ABN layers are not stock layers
