"""libccnet_proj.so and the module route built on it (``bf16-pixel-major-lib``, ``CrissCrossPMBF16ModuleFunction``) on the device.

1. the case table of tests/proj_cases.py on guarded device buffers (the emulator runs the same table: tests/test_emu_proj.py);
2. the node against its parts, bit for bit: the kernels are each pinned by (1) and by the existing tests of the pixel-major core
   and of the weight-gradient GEMM, so this pins the node with no tolerance;
3. the route end to end against the CPU oracle, next to the stock route on the same inputs;
4. memory formats, 5. autocast with fp32 parameters, 6. no host synchronisation, 7. reproducibility, graph replay and
   ``recompute_attention``."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import proj_cases as K  # noqa: E402
from guarded_memory import DeviceMemory  # noqa: E402
from oracle import cca_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PARAM_NAMES = ("query_conv.weight", "query_conv.bias", "key_conv.weight", "key_conv.bias", "value_conv.weight", "value_conv.bias")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from ccnet_amd import _proj_lib
    return _proj_lib.get_lib()               # raises when the extension has not been built: no fallback


@pytest.fixture(scope="module")
def mem(dev):
    return DeviceMemory()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case table
# ---------------------------------------------------------------------------------------------------------------------
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


# ---------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------
def make_module(C, dev, dtype=BF16, seed=0, library=True):
    """a module with gamma = 0.5 whose parameters are bf16-representable whatever ``dtype`` it keeps them in.  gamma stays an fp32
    parameter (0.5 either way; both bf16 routes read it through ``.float()``): a bf16 gamma would have torch round its scalar
    gradient to 8 bits on the way back, 2^-9 relative, which is the whole of the 2e-3 bar on dgamma before any kernel is looked at."""
    from ccnet_amd import CrissCrossAttention
    torch.manual_seed(seed)
    m = CrissCrossAttention(C)
    with torch.no_grad():
        for c in (m.query_conv, m.key_conv, m.value_conv):
            c.bias.copy_(torch.randn_like(c.bias) * 0.1)
        m.gamma.fill_(0.5)
    m = m.to(dev).to(BF16).to(dtype)
    m.gamma = torch.nn.Parameter(torch.full((1,), 0.5, device=dev))
    m.library_bf16_projections = library
    return m


def step(f, m, x, dy):
    """one forward + backward -> [y, dx, six weight / bias gradients, dgamma] (clones)"""
    m.zero_grad(set_to_none=True)
    x.grad = None
    y = f(x)
    y.backward(dy)
    p = dict(m.named_parameters())
    return [y.detach().clone(), x.grad.clone()] + [p[n].grad.clone() for n in PARAM_NAMES] + [m.gamma.grad.clone()]


def parts(m, xp, dyp, recompute=False):
    """what the node must compute, from its parts: pack, the library GEMM, the pixel-major core node, the library GEMM with the
    residual gradient as addend, the weight-gradient GEMM, the column sums"""
    from ccnet_amd import _lib
    from ccnet_amd.functions import CrissCrossPMBF16Function, _proj_colsum, _proj_gemm, _proj_pack, _projection_wgrad_gemm
    B, H, W, C = xp.shape
    cq, M = m.query_conv.out_channels, B * H * W
    ct = 2 * cq + C
    p = dict(m.named_parameters())
    w, wt, b = _proj_pack(*(p[n] for n in PARAM_NAMES))
    qkv = _proj_gemm(xp.reshape(M, C), w, b).view(B, H, W, ct).requires_grad_(True)
    xr = xp.detach().clone().requires_grad_(True)
    gamma = m.gamma.detach().float().clone().requires_grad_(True)
    y = CrissCrossPMBF16Function.apply(qkv, xr, gamma, cq, recompute)
    y.backward(dyp)
    dqkv = qkv.grad.reshape(M, ct)
    dx = _proj_gemm(dqkv, wt, None, xr.grad.reshape(M, C)).view(B, H, W, C)
    dw = _projection_wgrad_gemm(_lib.get_lib(), dqkv, xp.reshape(M, C))
    db = _proj_colsum(dqkv)
    return dict(y=y.detach(), dx=dx, dw=dw, db=db, dgamma=gamma.grad, qkv=qkv.detach())


def pm_inputs(shape, dev, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    xp = torch.randn(B, H, W, C, generator=g).to(dev).to(BF16)
    dyp = torch.randn(B, H, W, C, generator=g).to(dev).to(BF16)
    return xp, dyp


@pytest.mark.parametrize("shape", [(2, 64, 20, 24), (1, 512, 17, 19), (1, 64, 1, 9)], ids=lambda s: "x".join(map(str, s)))
def test_node_equals_its_parts_bit_for_bit(lib, dev, shape):
    from ccnet_amd.functions import CrissCrossPMBF16ModuleFunction
    B, C, H, W = shape
    m = make_module(C, dev)
    cq = C // 8
    xp, dyp = pm_inputs(shape, dev, seed=5)
    want = parts(m, xp, dyp)
    p = dict(m.named_parameters())
    xn = xp.detach().clone().requires_grad_(True)
    gamma = m.gamma.detach().float().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = CrissCrossPMBF16ModuleFunction.apply(xn, *(p[n] for n in PARAM_NAMES), gamma, False)
    y.backward(dyp)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and torch.equal(y, want["y"])
    assert xn.grad.dtype == BF16 and torch.equal(xn.grad, want["dx"])
    dw, db = want["dw"], want["db"]
    for name, ref in (("query_conv.weight", dw[:cq]), ("key_conv.weight", dw[cq:2 * cq]), ("value_conv.weight", dw[2 * cq:]),
                      ("query_conv.bias", db[:cq]), ("key_conv.bias", db[cq:2 * cq]), ("value_conv.bias", db[2 * cq:])):
        g = p[name].grad
        assert g.dtype == BF16 and g.shape == p[name].shape and torch.equal(g, ref.to(BF16).reshape(g.shape)), name
    assert torch.equal(gamma.grad, want["dgamma"])


def test_route_against_the_oracle_next_to_the_stock_route(lib, dev):
    """(2,64,20,24), bf16-rounded inputs and parameters.  Both routes make the same roundings (q | k | v, y, dqkv, dx and the
    gradients to bf16) in a different summation order; the stock route is the parent's code, not the code under test.  y within the
    smoke test's 2.5e-2; dx and each weight / bias gradient: library error <= 2 x stock error + 2^-8 max |ref| (the factor for the
    fluctuation of a maximum over >= 64 elements, the term for one final bf16 ulp); dgamma within 2e-3 max(1, |ref|)."""
    B, C, H, W = 2, 64, 20, 24
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W).to(BF16)
    dy = torch.randn(B, C, H, W).to(BF16)
    errs = {}
    for route, library in (("bf16-pixel-major", False), ("bf16-pixel-major-lib", True)):
        m = make_module(C, dev, library=library)
        xd = x.to(dev).requires_grad_(True)
        assert m.route(xd) == route
        got = step(m, m, xd, dy.to(dev))
        torch.cuda.synchronize()
        f = lambda t: t.detach().float().cpu()                                  # noqa: E731
        params = {n: f(t) for n, t in m.state_dict().items()}
        yr, dxr, gr = O.cca_module_forward_backward(f(x), params, f(dy))
        refs = [yr, dxr] + [gr[n] for n in PARAM_NAMES] + [gr["gamma"]]
        errs[route] = {n: float((f(g) - r.reshape(g.shape)).abs().max()) for n, g, r in zip(("y", "dx") + PARAM_NAMES + ("gamma",), got, refs)}
        print(route, {n: f"{e:.3e}" for n, e in errs[route].items()})
    mags = {n: float(r.abs().max()) for n, r in zip(("y", "dx") + PARAM_NAMES + ("gamma",), refs)}
    print("max |ref|", {n: f"{e:.3e}" for n, e in mags.items()})
    stock, ours = errs["bf16-pixel-major"], errs["bf16-pixel-major-lib"]
    assert ours["y"] < 2.5e-2
    for n in ("dx",) + PARAM_NAMES:
        assert ours[n] <= 2.0 * stock[n] + 2.0 ** -8 * mags[n], (n, ours[n], stock[n], mags[n])
    assert ours["gamma"] < 2e-3 * max(1.0, mags["gamma"]), (ours["gamma"], mags["gamma"])


def test_output_follows_the_input_memory_format(lib, dev):
    m = make_module(64, dev)
    torch.manual_seed(1)
    x = torch.randn(2, 64, 20, 24, device=dev).to(BF16)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert m.route(cl) == m.route(x) == "bf16-pixel-major-lib"
    y_cl, y = m(cl.requires_grad_(True)), m(x.clone().requires_grad_(True))
    assert y_cl.is_contiguous(memory_format=torch.channels_last) and not y_cl.is_contiguous()
    assert y.is_contiguous()
    assert y.shape == x.shape and y.dtype == BF16 and torch.equal(y_cl, y)
    with torch.no_grad():                                   # inference keeps nothing and takes the same route
        assert torch.equal(m(cl), y)


def test_autocast_with_fp32_parameters(lib, dev):
    """what an autocast training run hands the module: fp32 parameters, bf16 activations.  The new route is chosen, the gradients
    are fp32, and dW is the fp32 sum of the weight-gradient GEMM's partials, not a bf16-rounded copy of it."""
    shape = (2, 64, 20, 24)
    B, C, H, W = shape
    cq = C // 8
    m = make_module(C, dev, dtype=torch.float32)
    xp, dyp = pm_inputs(shape, dev, seed=9)
    x = xp.permute(0, 3, 1, 2).detach().requires_grad_(True)            # channels_last
    with torch.autocast(device_type="cuda", dtype=BF16):
        assert m.route(x) == "bf16-pixel-major-lib"
        got = step(m, m, x, dyp.permute(0, 3, 1, 2))
    assert m.route(x) != "bf16-pixel-major-lib"                          # fp32 parameters without autocast: not this route
    want = parts(m, xp, dyp)
    torch.cuda.synchronize()
    assert got[0].dtype == BF16 and torch.equal(got[0].permute(0, 2, 3, 1), want["y"])
    assert torch.equal(got[1].permute(0, 2, 3, 1), want["dx"])
    dw, db = want["dw"], want["db"]
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    for g, ref in zip(got[2:8], (dw[:cq], db[:cq], dw[cq:2 * cq], db[cq:2 * cq], dw[2 * cq:], db[2 * cq:])):
        assert g.dtype == torch.float32 and torch.equal(g, ref.reshape(g.shape))
    assert bool((dw != dw.to(BF16).float()).any())                       # (unrounded: not every sum is a bf16 number)


def test_forward_and_backward_make_no_host_synchronisation(lib, dev):
    m = make_module(64, dev)
    xp, dyp = pm_inputs((2, 64, 20, 24), dev, seed=3)
    x, dy = xp.permute(0, 3, 1, 2).detach().requires_grad_(True), dyp.permute(0, 3, 1, 2)
    step(m, m, x, dy)                                       # (libraries loaded, workspaces of the allocator warm)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.zero_grad(set_to_none=True)
        x.grad = None
        y = m(x)
        y.backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert x.grad is not None and m.value_conv.weight.grad is not None


def test_reproducible_graph_capturable_and_recompute_neutral(lib, dev):
    """(1,512,17,19): two eager runs, an eager run and a ``graph_module`` replay, ``recompute_attention`` on and off -- the
    same bits each time"""
    from ccnet_amd import graph_module
    shape = (1, 512, 17, 19)
    m = make_module(512, dev)
    xp, dyp = pm_inputs(shape, dev, seed=7)
    x, dy = xp.permute(0, 3, 1, 2).detach().requires_grad_(True), dyp.permute(0, 3, 1, 2)
    assert m.route(x) == "bf16-pixel-major-lib"
    a, b = step(m, m, x, dy), step(m, m, x, dy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    m.recompute_attention = True
    c = step(m, m, x, dy)
    m.recompute_attention = False
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    g = graph_module(m, x.detach().clone().requires_grad_(True))
    d = step(g, m, x, dy)
    torch.cuda.synchronize()
    for u, v in zip(a, d):
        assert torch.equal(u, v)
