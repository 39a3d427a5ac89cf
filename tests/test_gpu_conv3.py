"""libccnet_conv3.so and the layer built on it (ccnet_amd/conv3.py) on the device.

1. the case table of tests/conv3_cases.py on guarded device buffers (the emulator runs the same table: tests/test_emu_conv3.py);
2. every entry point twice: the same bits; contract violations: error codes, nothing launched;
3. the autograd function against its parts, bit for bit, eager and as one captured graph replayed twice;
4. ``DeviceConv3x3`` next to stock ``F.conv2d`` (bf16, channels_last, same device), both against the fp64 oracle; a converted
   two-block bottleneck stack next to the stock stack;
5. memory formats, autocast with fp32 parameters, no host synchronisation, one ``train_synthetic --bf16-params --device-conv3`` run."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conv3_cases as K  # noqa: E402
import conv3_oracle as O  # noqa: E402
from guarded_memory import DeviceMemory  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from ccnet_amd import _conv3_lib
    return _conv3_lib.get_lib()              # raises when the extension has not been built: no fallback


@pytest.fixture(scope="module")
def mem(dev):
    return DeviceMemory()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,direction,variant", K.conv_ids(), ids=lambda v: v)
def test_conv_case_table(lib, mem, cid, direction, variant):
    K.run_conv(lib, mem, cid, direction, variant)


@pytest.mark.parametrize("case", K.TAP_CASES, ids=lambda v: "x".join(map(str, v)))
def test_one_hot_tap_shifts_the_image_bit_for_bit(lib, mem, case):
    K.run_tap_shift(lib, mem, case)


@pytest.mark.parametrize("case", K.EPILOGUE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_conv_of_zero_rows_is_the_rounded_bias_plus_addend(lib, mem, case):
    K.run_epilogue(lib, mem, case)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("co,ci", K.PACK_CASES)
def test_pack_matches_numpy(lib, mem, co, ci, f32):
    K.run_pack(lib, mem, co, ci, f32)


@pytest.mark.parametrize("case", K.WGRAD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_weight_gradient_case_table(lib, mem, case):
    K.run_wgrad(lib, mem, case)


@pytest.mark.parametrize("case", K.ONEHOT_CASES, ids=lambda v: "x".join(map(str, v[:6])) + "@" + "x".join(map(str, v[6])))
def test_one_hot_dy_picks_the_shifted_row_bit_for_bit(lib, mem, case):
    K.run_wgrad_onehot(lib, mem, case)


# ---------------------------------------------------------------------------------------------------------------------
# 2. reproducibility and the contract
# ---------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_same_bits_twice(lib, mem):
    for cid, direction, variant in (("2x9x15-64-64-d2", "fwd", "bias-add-dense"), ("1x6x10-512-512-d4", "adj", "add-packed")):
        a, b = K.conv_bits(lib, mem, cid, direction, variant), K.conv_bits(lib, mem, cid, direction, variant)
        assert np.array_equal(a, b), (cid, direction)
    rng = np.random.default_rng(3)
    dy, x = (K.bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((2, 9, 15, 64), (2, 9, 15, 72)))
    runs = [K.launch_wgrad(lib, mem, "dense", dy, x, 2, 0, zero=zero) for zero in (False, True, False)]     # NaN, zero, NaN workspaces
    for r in runs[1:]:
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(runs[0][:3], r[:3]))
    from ccnet_amd.conv3 import _pack
    for dtype in (BF16, torch.float32):
        w = torch.randn(136, 72, 3, 3, generator=torch.Generator().manual_seed(1)).to(mem.device).to(dtype)
        first, second = _pack(w), _pack(w)
        torch.cuda.synchronize()
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), dtype


def test_contract_violations_come_back_as_error_codes_with_no_launch(lib, dev):
    from ccnet_amd import _conv3_lib as P
    t = torch.full((4096,), float("nan"), device=dev, dtype=BF16)
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    conv = lib.ccnet_conv3_bf16
    assert conv(p, p, None, None, p, 1, 2, 2, 12, 8, 1, 16, 0, 8, s) == P.CCNET_CONV3_E_BADSHAPE            # K % 8
    assert conv(p, p, None, None, p, 1, 2, 2, 8, 6, 1, 8, 0, 8, s) == P.CCNET_CONV3_E_BADSHAPE              # N % 4
    assert conv(p, p, None, None, p, 1, 2, 2, 8, 8, 0, 8, 0, 8, s) == P.CCNET_CONV3_E_BADSHAPE              # dilation
    assert conv(p, p, None, None, p, 1, 2, 2, 8, 8, 1, 8, 0, 4, s) == P.CCNET_CONV3_E_BADSHAPE              # ldo < N
    assert conv(p, None, None, None, p, 1, 2, 2, 8, 8, 1, 8, 0, 8, s) == P.CCNET_CONV3_E_NULLPTR
    assert lib.ccnet_conv3_pack(p, 7, p, p, 8, 8, s) == P.CCNET_CONV3_E_BADFLAGS
    assert lib.ccnet_conv3_wgrad_bf16(p, p, p, 16, 1, 2, 2, 8, 8, 1, 8, 8, 1, s) == P.CCNET_CONV3_E_WORKSPACE
    assert lib.ccnet_conv3_wgrad_finish(p, p, 0, 8, 8, 0, s) == P.CCNET_CONV3_E_BADSHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())                                                                       # nothing was written


# ---------------------------------------------------------------------------------------------------------------------
# 3. the autograd function
# ---------------------------------------------------------------------------------------------------------------------
def tensors(shape, dev, seed, bias=True, dtype=BF16):
    """channels_last x and dy, a weight and a bias that are bf16-representable whatever ``dtype`` keeps them in"""
    B, ci, co, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, ci, generator=g).to(dev).to(BF16).permute(0, 3, 1, 2)
    dy = torch.randn(B, H, W, co, generator=g).to(dev).to(BF16).permute(0, 3, 1, 2)
    w = (torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)).to(dev).to(BF16).to(dtype)
    b = (torch.randn(co, generator=g) * 0.1).to(dev).to(BF16).to(dtype) if bias else None
    return x, dy, w, b


def run_function(x, dy, w, b, d):
    from ccnet_amd.conv3 import conv3x3
    xr, wr = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
    br = None if b is None else b.detach().requires_grad_(True)
    y = conv3x3(xr, wr, br, d)
    y.backward(dy)
    return [y.detach(), xr.grad, wr.grad] + ([] if b is None else [br.grad])


def run_parts(x, dy, w, b, d):
    """what the function must compute, from the entry points: pack, the launch, the launch on dy, wgrad + finish, the column sums"""
    from ccnet_amd.conv3 import _launch, _pack, _wgrad
    from ccnet_amd.functions import _proj_colsum
    B, co, H, W = dy.shape
    fwd, adj = _pack(w)
    y = _launch(x, x.stride(3), fwd, None if b is None else b.float(), d)
    dx = _launch(dy, dy.stride(3), adj, None, d)
    dw = _wgrad(dy, dy.stride(3), x, x.stride(3), d, w.dtype, tuple(w.shape))
    out = [y, dx, dw]
    if b is not None:
        out.append(_proj_colsum(dy.permute(0, 2, 3, 1).reshape(B * H * W, co)).to(b.dtype))
    return out


@pytest.mark.parametrize("shape,d,bias", [((2, 64, 72, 9, 15), 2, True), ((1, 8, 8, 1, 20), 1, False), ((1, 256, 256, 6, 10), 2, True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_function_equals_its_parts_bit_for_bit(lib, dev, shape, d, bias):
    x, dy, w, b = tensors(shape, dev, seed=5, bias=bias)
    got, want = run_function(x, dy, w, b, d), run_parts(x, dy, w, b, d)
    torch.cuda.synchronize()
    for name, u, v in zip(("y", "dx", "dW", "db"), got, want):
        assert u.dtype == BF16 and u.shape == v.shape and torch.equal(u, v), name
    assert got[0].is_contiguous(memory_format=torch.channels_last) and got[1].is_contiguous(memory_format=torch.channels_last)
    assert got[2].is_contiguous()


def test_eager_equals_one_captured_graph_replayed_twice(lib, dev):
    from ccnet_amd.conv3 import conv3x3
    x, dy, w, b = tensors((2, 64, 64, 9, 15), dev, seed=7)
    eager = run_function(x, dy, w, b, 2)
    xs, ws, bs = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # (library loaded, allocator warm)
        for _ in range(2):
            conv3x3(xs, ws, bs, 2).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    xs.grad = ws.grad = bs.grad = None
    with torch.cuda.graph(graph):
        ys = conv3x3(xs, ws, bs, 2)
        ys.backward(dy)
    for _ in range(2):
        for t in (ys, xs.grad, ws.grad, bs.grad):
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, u, v in zip(("y", "dx", "dW", "db"), eager, (ys.detach(), xs.grad, ws.grad, bs.grad)):
            assert torch.equal(u, v), name


def test_forward_and_backward_make_no_host_synchronisation(lib, dev):
    x, dy, w, b = tensors((2, 64, 64, 9, 15), dev, seed=3)
    run_function(x, dy, w, b, 2)                                    # (libraries loaded, workspaces of the allocator warm)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run_function(x, dy, w, b, 2)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(t is not None for t in got)


def test_an_nchw_input_costs_one_counted_copy_and_gives_the_same_bits(lib, dev):
    from ccnet_amd import conv3
    x, dy, w, b = tensors((2, 64, 64, 9, 15), dev, seed=11)
    before = conv3.layout_copies
    want = run_function(x, dy, w, b, 2)
    assert conv3.layout_copies == before                            # channels_last in, channels_last gradient: no copy
    got = run_function(x.contiguous(), dy, w, b, 2)
    assert conv3.layout_copies == before + 1
    got2 = run_function(x.contiguous(), dy.contiguous(), w, b, 2)
    assert conv3.layout_copies == before + 3
    # a channel slice of a wider channels_last tensor is taken as it is
    wide = torch.zeros(2, 9, 15, 80, device=dev, dtype=BF16)
    wide[..., 8:72] = x.permute(0, 2, 3, 1)
    got3 = run_function(wide[..., 8:72].permute(0, 3, 1, 2), dy, w, b, 2)
    assert conv3.layout_copies == before + 3
    torch.cuda.synchronize()
    for other in (got, got2, got3):
        assert other[0].is_contiguous(memory_format=torch.channels_last)
        for u, v in zip(want, other):
            assert torch.equal(u, v)


def test_autocast_with_fp32_parameters_returns_unrounded_fp32_gradients(lib, dev):
    shape, d = (2, 64, 72, 9, 15), 2
    x, dy, w, b = tensors(shape, dev, seed=9, dtype=torch.float32)
    with torch.autocast(device_type="cuda", dtype=BF16):
        got = run_function(x, dy, w, b, d)
        got32 = run_function(x.float(), dy, w, b, d)                # an fp32 input is cast as autocast's own convolution casts it
    want = run_parts(x, dy, w, b, d)
    torch.cuda.synchronize()
    assert got[0].dtype == BF16 and got[2].dtype == torch.float32 and got[3].dtype == torch.float32
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert got32[1].dtype == torch.float32 and torch.equal(got32[0], got[0]) and torch.equal(got32[2], got[2])
    assert bool((got[2] != got[2].to(BF16).float()).any())          # (unrounded: not every sum is a bf16 number)
    # db against the fp64 sum at the column sums' bar: a double accumulation and one rounding to fp32
    d64 = dy.permute(0, 2, 3, 1).reshape(-1, shape[2]).double().cpu().numpy()
    ref, mag = d64.sum(0), np.abs(d64).sum(0)
    err = np.abs(got[3].double().cpu().numpy() - ref)
    assert bool((err <= 2.0 ** -23 * np.abs(ref) + 1e-12 * mag).all()), float(err.max())
    with pytest.raises(TypeError, match="float32"):
        run_function(x, dy, w, b, d)                                # fp32 parameters without autocast


# ---------------------------------------------------------------------------------------------------------------------
# 4. next to the stock convolution
# ---------------------------------------------------------------------------------------------------------------------
def within_the_end_to_end_rule(names, ours, stock, refs):
    """library error <= 2 x stock error + 2^-8 max |ref| (the factor for the fluctuation of a maximum over many
    elements, the term for one final bf16 ulp); every figure is printed before it is asserted"""
    f = lambda t: t.detach().double().cpu().numpy()                             # noqa: E731
    rows = []
    for n, a, s, r in zip(names, ours, stock, refs):
        ea, es, mr = float(np.abs(f(a) - r).max()), float(np.abs(f(s) - r).max()), float(np.abs(r).max())
        rows.append((n, ea, es, mr))
        print(f"{n}: library {ea:.3e}, stock {es:.3e}, max |ref| {mr:.3e}")
    for n, ea, es, mr in rows:
        assert ea <= 2.0 * es + 2.0 ** -8 * mr, (n, ea, es, mr)


@pytest.mark.parametrize("ci,co,d", [(256, 256, 2), (512, 512, 4)])
def test_layer_next_to_stock_conv2d_against_the_fp64_oracle(lib, dev, ci, co, d):
    from ccnet_amd.conv3 import DeviceConv3x3
    x, dy, w, b = tensors((2, ci, co, 12, 20), dev, seed=ci + d)
    layer = DeviceConv3x3(ci, co, 3, padding=d, dilation=d).to(dev).to(BF16)
    with torch.no_grad():
        layer.weight.copy_(w), layer.bias.copy_(b)
    xr = x.detach().requires_grad_(True)
    y = layer(xr)
    y.backward(dy)
    ours = [y, xr.grad, layer.weight.grad, layer.bias.grad]
    xs, ws, bs = x.detach().requires_grad_(True), w.detach().requires_grad_(True), b.detach().requires_grad_(True)
    ys = F.conv2d(xs, ws, bs, stride=1, padding=d, dilation=d)
    ys.backward(dy)
    stock = [ys, xs.grad, ws.grad, bs.grad]
    torch.cuda.synchronize()
    pm = lambda t: t.detach().permute(0, 2, 3, 1).double().cpu().numpy()        # noqa: E731
    xn, dyn, wn = pm(x), pm(dy), w.double().cpu().numpy()
    refs = [O.forward(xn, wn, b.double().cpu().numpy(), d).transpose(0, 3, 1, 2), O.input_grad(dyn, wn, d).transpose(0, 3, 1, 2),
            O.weight_grad(dyn, xn, d), O.bias_grad(dyn)]
    within_the_end_to_end_rule(("y", "dx", "dW", "db"), ours, stock, refs)


class TwoBlocks(nn.Module):
    """two bottleneck units (1x1 -> 3x3 dilated -> 1x1, residual), the second 3x3 with a bias; no normalisation"""

    def __init__(self):
        super().__init__()
        self.a1, self.a2, self.a3 = nn.Conv2d(64, 16, 1, bias=False), nn.Conv2d(16, 16, 3, padding=2, dilation=2, bias=False), nn.Conv2d(16, 64, 1, bias=False)
        self.b1, self.b2, self.b3 = nn.Conv2d(64, 16, 1, bias=False), nn.Conv2d(16, 16, 3, padding=4, dilation=4, bias=True), nn.Conv2d(16, 64, 1, bias=False)

    def forward(self, x):
        x = F.relu(x + self.a3(F.relu(self.a2(F.relu(self.a1(x))))))
        return F.relu(x + self.b3(F.relu(self.b2(F.relu(self.b1(x))))))


def test_converted_bottleneck_stack_next_to_the_stock_stack(lib, dev):
    from ccnet_amd.conv3 import DeviceConv3x3, convert_conv3x3
    torch.manual_seed(0)
    ref = TwoBlocks().double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(BF16).double())                                        # bf16-representable parameters
    x = torch.randn(2, 64, 12, 20).to(BF16)
    target = torch.randn(2, 64, 12, 20)
    nets = {}
    for name in ("stock", "ours"):
        net = TwoBlocks()
        net.load_state_dict(ref.state_dict(), strict=True)
        net = net.to(dev).to(BF16)
        if name == "ours":
            assert convert_conv3x3(net) == 2 and type(net.a2) is DeviceConv3x3 and type(net.b2) is DeviceConv3x3 and type(net.a1) is nn.Conv2d
            state = net.state_dict()
            assert list(state.keys()) == list(ref.state_dict().keys())
            back = TwoBlocks()
            back.load_state_dict(state, strict=True)                             # ... and round-trips into a stock stack
            assert all(torch.equal(u.double(), v) for u, v in zip(back.state_dict().values(), ref.state_dict().values()))
        nets[name] = net
    outs = {}
    for name, net in nets.items():
        xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        loss = ((net(xd).float() - target.to(dev)) ** 2).mean()
        loss.backward()
        outs[name] = [loss.detach(), xd.grad] + [p.grad for p in net.parameters()]
    xr = x.double().requires_grad_(True)
    loss = ((ref(xr) - target.double()) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    refs = [t.detach().numpy() for t in [loss, xr.grad] + [p.grad for p in ref.parameters()]]
    names = ["loss", "dx"] + [n for n, _ in ref.named_parameters()]
    within_the_end_to_end_rule(names, outs["ours"], outs["stock"], refs)


# ---------------------------------------------------------------------------------------------------------------------
# what --device-conv3 changes around the layers: the stock normalisation layers on bf16 channels_last input, and the attention
# module's two casting routes, which keep a channels_last input's format
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,activation", [("InPlaceABNSync", "identity"), ("InPlaceABNSync", "leaky_relu"), ("ABN", "leaky_relu")])
def test_normalisation_layer_on_bf16_channels_last_input_against_the_fp32_layer(dev, kind, activation):
    """The swapped layer (bf16 NHWC input, fp32 affine, training) against the SAME stock layer on the same values in fp32 NCHW.
    Bars from the formats: y and dx are one bf16 rounding of an fp32 result, 2^-8 |ref|, plus 2^-8 of the largest magnitude for
    the cancellation inside x - mean; the fp32 sums (dweight, dbias, running statistics) over n = B H W = 570 terms differ by
    summation order only, n 2^-24 < 4e-5 of the sum of magnitudes; twice that is allowed."""
    import inplace_abn

    from ccnet_amd.conv3 import native_batch_norm_for_bf16_channels_last
    C, shape = 24, (2, 15, 19)
    torch.manual_seed(3)
    layers = []
    for _ in range(2):
        m = getattr(inplace_abn, kind)(C, activation=activation)
        with torch.no_grad():
            m.weight.copy_(torch.linspace(0.5, 1.5, C)), m.bias.copy_(torch.linspace(-0.3, 0.3, C))
        layers.append(m.to(dev).train())
    ref, ours = layers
    assert native_batch_norm_for_bf16_channels_last(ours) == 1 and isinstance(ours, getattr(inplace_abn, kind))
    assert list(ours.state_dict().keys()) == list(ref.state_dict().keys())
    x = (torch.randn(shape[0], *shape[1:], C) * 2 + 0.5).to(dev).to(BF16).permute(0, 3, 1, 2)
    dy = torch.randn(shape[0], *shape[1:], C).to(dev).to(BF16).permute(0, 3, 1, 2)
    xo = x.detach().requires_grad_(True)
    yo = ours(xo)
    yo.backward(dy)
    xr = x.float().contiguous().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.float().contiguous())
    torch.cuda.synchronize()
    assert yo.dtype == BF16 and yo.is_contiguous(memory_format=torch.channels_last) and xo.grad.is_contiguous(memory_format=torch.channels_last)
    f = lambda t: t.detach().double().cpu()                                     # noqa: E731
    for name, got, want in (("y", yo, yr), ("dx", xo.grad, xr.grad)):
        err, bar = (f(got) - f(want)).abs(), 2.0 ** -8 * f(want).abs() + 2.0 ** -8 * float(f(want).abs().max())
        print(name, f"max err {float(err.max()):.3e}, worst err/bar {float((err / bar).max()):.3f}")
        assert bool((err <= bar).all()), name
    n = shape[0] * shape[1] * shape[2]
    xhat = (f(xr) - f(xr).mean((0, 2, 3), keepdim=True)) / f(xr).var((0, 2, 3), unbiased=False, keepdim=True).add(ref.eps).sqrt()
    slope = torch.where(f(yr) >= 0, 1.0, ref.activation_param) if activation == "leaky_relu" else torch.ones_like(f(yr))
    mags = {"dweight": (f(dy) * slope * xhat).abs().sum((0, 2, 3)), "dbias": (f(dy) * slope).abs().sum((0, 2, 3)),
            "running_mean": 0.1 * f(xr).abs().mean((0, 2, 3)) + 1.0, "running_var": 0.1 * (f(xr) ** 2).mean((0, 2, 3)) + 1.0}
    for name, got, want in (("dweight", ours.weight.grad, ref.weight.grad), ("dbias", ours.bias.grad, ref.bias.grad),
                            ("running_mean", ours.running_mean, ref.running_mean), ("running_var", ours.running_var, ref.running_var)):
        err, bar = (f(got) - f(want)).abs(), 2 * n * 2.0 ** -24 * mags[name]
        print(name, f"max err {float(err.max()):.3e}, worst err/bar {float((err / bar).max()):.3f}")
        assert got.dtype == torch.float32 and bool((err <= bar).all()), name


@pytest.mark.parametrize("shape,route", [((1, 16, 9, 11), "separate-strips"), ((1, 64, 2, 140), "f32-planes-cast")], ids=lambda v: str(v))
def test_attention_casting_routes_keep_a_channels_last_input_format(dev, shape, route):
    """bf16 inputs: the route's final cast is written in the input's memory format; the values are those of the NCHW call"""
    from ccnet_amd import CrissCrossAttention
    torch.manual_seed(0)
    m = CrissCrossAttention(shape[1]).to(dev).to(BF16)
    with torch.no_grad():
        m.gamma.fill_(0.5)
    x = torch.randn(*shape, device=dev).to(BF16)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert m.route(cl) == m.route(x) == route
    with torch.no_grad():
        y, ycl = m(x), m(cl)
    assert y.is_contiguous() and ycl.is_contiguous(memory_format=torch.channels_last) and not ycl.is_contiguous()
    assert ycl.dtype == BF16 and torch.equal(y, ycl)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the driver
# ---------------------------------------------------------------------------------------------------------------------
def test_train_driver_with_device_conv3_runs_channels_last_without_a_copy(lib, dev):
    """two steps of ``--bf16-params --device-conv3`` at size 129 on the smallest stage table of the model tests: finite losses, every
    eligible convolution converted, and not one layout copy: the network stays channels_last from the images to the heads"""
    from ccnet_amd import conv3
    from ccnet_amd import train_synthetic as T
    from ccnet_amd.segmodel import CriterionDSN, ResNetCCNet
    stages = ((8, 1, 1, 1), (8, 1, 2, 1), (8, 1, 1, 2), (16, 1, 1, 4))
    # (--abn torch keeps the stock normalisation layers and has the driver report every step's loss)
    args = T.parse_args(["--bf16-params", "--device-conv3", "--abn", "torch", "--size", "129", "--num-classes", "5", "--steps", "1",
                         "--warmup", "1"])
    seen = {}

    def factory():
        seen["model"] = ResNetCCNet(5, CriterionDSN(), recurrence=2, stages=stages)
        return seen["model"]

    before = conv3.layout_copies
    res = T.run(args, model_factory=factory, quiet=True)
    print("layout copies:", conv3.layout_copies - before, "losses:", res["step_losses"])
    assert len(res["step_losses"]) == 2 and all(math.isfinite(v) and v > 0 for v in res["step_losses"])
    assert conv3.layout_copies - before == 0
    assert res["config"]["conv3"] == "device" and res["dtype"] == "bf16-params"
    # the stem's second and third convolution, three of the four blocks' 3x3 (layer2's has stride 2), conva, convb, the bottleneck's, the DSN head's
    assert res["config"]["conv3_layers"] == 2 + 3 + 3 + 1
    model = seen["model"]
    assert type(model.conv1) is nn.Conv2d and type(model.layer2[0].conv2) is nn.Conv2d and type(model.layer3[0].conv2) is conv3.DeviceConv3x3
