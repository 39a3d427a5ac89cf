"""GPU checks of the device ABN (ccnet_amd.abn over libccnet_abn.so): out-of-place parity with the inplace_abn restatement at
the backbone's shapes, in-place behaviour against the float64 oracle, the fused residual unit, cross-rank statistics over a
world-2 gloo group, determinism, no host sync, and the training driver."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inplace_abn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import abn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _rel(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    s = max(b.abs().max().item(), scale or 0.0, 1e-30)
    return (a - b).abs().max().item() / s


def _randomise(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.weight.copy_(torch.rand(m.num_features, generator=g) * 2 - 0.5)
        m.bias.copy_(torch.rand(m.num_features, generator=g) - 0.5)
        m.running_mean.copy_(torch.rand(m.num_features, generator=g) * 0.2)
        m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)


def _run(m, x, dy, residual=None):
    """y and the gradients of one forward + backward (x is cloned: an in-place layer writes over its input)"""
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    xa = xi * 1.0 if getattr(m, "inplace", False) else xi                  # an in-place layer cannot overwrite a leaf
    if residual is None:
        y = m(xa)
    else:
        r = residual.clone().requires_grad_(True)
        y = m(xa, residual=r)
    y.backward(dy)
    out = {"y": y.detach().clone(), "dx": xi.grad, "dw": m.weight.grad, "db": m.bias.grad,
           "rm": m.running_mean.clone(), "rv": m.running_var.clone()}
    if residual is not None:
        out["dres"] = r.grad
    return out


SHAPES = [(1, 64, 385, 385), (1, 256, 193, 193), (1, 256, 97, 97), (1, 1024, 97, 97), (1, 2048, 97, 97),
          (2, 256, 97, 97)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cls,act", [("ABN", "identity"), ("InPlaceABNSync", "leaky_relu")])
def test_out_of_place_parity_with_the_torch_restatement(shape, dtype, training, cls, act):
    """The yardstick is the inplace_abn restatement itself, run in float64 on the CPU on the same (for bf16: the same
    bf16-rounded) inputs.  Its fp32 run on the GPU is not one: on MI355X its training-mode gradients differ from its own
    float64 result by up to about 2 % (dbias against the exact sum of dy), the device layer's by 1e-7."""
    from ccnet_amd import abn
    torch.manual_seed(0)
    ref = getattr(inplace_abn, cls)(shape[1], activation=act)
    _randomise(ref, 1)
    dev = getattr(abn, cls)(shape[1], activation=act)
    dev.load_state_dict(ref.state_dict())
    dev.inplace = False
    ref, dev = ref.double().train(training), dev.to(DEV).train(training)
    x = (torch.randn(shape, device=DEV) * 2 + 0.5).to(dtype)
    dy = torch.randn(shape, device=DEV).to(dtype)
    a, b = _run(dev, x, dy), _run(ref, x.double().cpu(), dy.double().cpu())
    # the header's bar; bf16: one bf16 rounding of y and dx, sums over the same bf16 inputs
    ty, tg = (1e-5, 1e-4) if dtype == torch.float32 else (2 ** -7, 2 ** -6)
    assert a["y"].dtype == dtype and a["dx"].dtype == dtype
    assert _rel(a["y"], b["y"]) <= ty
    for k in ("rm", "rv"):
        assert _rel(a[k], b[k]) <= 1e-5, k
    var = x.double().var(dim=(0, 2, 3), unbiased=False) if training else dev.running_var.double()
    k_dz = (dev.weight.detach().abs().max().item() / (var.min().item() + dev.eps) ** 0.5) * dy.abs().max().item()
    assert _rel(a["dx"], b["dx"], scale=k_dz) <= tg
    assert _rel(a["dw"], b["dw"]) <= tg and _rel(a["db"], b["db"]) <= tg


def _oracle_check(m, x, dy, residual=None, act=O.LEAKY_RELU, p=0.01, tol=1e-4):
    w, b = m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()
    rm, rv = m.running_mean.cpu().numpy().copy(), m.running_var.cpu().numpy().copy()
    r = _run(m, x, dy, residual)
    res = None if residual is None else residual.double().cpu().numpy()
    f = O.forward(x.double().cpu().numpy(), w, b, rm, rv, m.training, act=act, p=p, gamma_mode=1, residual=res)
    g = O.backward(f, dy.double().cpu().numpy(), w, m.training, act=act, p=p, gamma_mode=1)
    assert _rel(r["y"], torch.from_numpy(f["y"])) <= 1e-5
    assert _rel(r["rm"], torch.from_numpy(f["running_mean"])) <= 1e-5
    assert _rel(r["rv"], torch.from_numpy(f["running_var"])) <= 1e-5
    k = np.abs(O.gamma_of(w, len(w), 1, 1e-5) * f["invstd"]).max() * float(dy.abs().max())
    assert _rel(r["dx"], torch.from_numpy(g["dx"]), scale=k) <= tol
    assert _rel(r["dw"], torch.from_numpy(g["dweight"])) <= tol
    assert _rel(r["db"], torch.from_numpy(g["dbias"])) <= tol
    if residual is not None:
        assert _rel(r["dres"], torch.from_numpy(g["dresidual"])) <= tol
    return r


@pytest.mark.parametrize("act,p", [("leaky_relu", 0.01), ("elu", 1.0), ("identity", 0.0)])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_in_place_matches_the_float64_oracle(act, p, training):
    from ccnet_amd.abn import InPlaceABN
    m = InPlaceABN(256, activation=act, activation_param=p)
    _randomise(m, 2)
    m = m.to(DEV).train(training)
    x = torch.randn(2, 256, 97, 97, device=DEV) * 1.5 + 0.3
    dy = torch.randn_like(x)
    code = {"leaky_relu": O.LEAKY_RELU, "elu": O.ELU, "identity": O.IDENTITY}[act]
    _oracle_check(m, x, dy, act=code, p=p, tol=1e-3 if act == "elu" else 1e-4)


def test_in_place_with_a_residual_matches_the_oracle():
    from ccnet_amd.abn import InPlaceABN
    m = InPlaceABN(64, activation="leaky_relu", activation_param=0.1)
    _randomise(m, 3)
    m = m.to(DEV).train()
    x = torch.randn(2, 64, 65, 63, device=DEV)
    _oracle_check(m, x, torch.randn_like(x), residual=torch.randn_like(x), p=0.1)


def test_in_place_output_shares_the_input_storage_and_misuse_raises():
    from ccnet_amd.abn import InPlaceABNSync
    m = InPlaceABNSync(32).to(DEV).train()
    leaf = torch.randn(2, 32, 17, 19, device=DEV, requires_grad=True)
    x = leaf * 1.0
    v0, ptr = x._version, x.data_ptr()
    y = m(x)
    assert y.data_ptr() == ptr and x._version > v0
    y.sum().backward()
    assert torch.isfinite(leaf.grad).all()
    # the overwritten input is needed by another branch's backward: autograd's version counter catches it
    x = leaf * 1.0
    other = (x * x).sum()
    y = m(x)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (other + y.sum()).backward()
    with pytest.raises(ValueError, match="relu"):
        InPlaceABNSync(32, activation="relu").to(DEV)(leaf * 1.0)


def test_in_place_weight_zero_gives_finite_gradients():
    from ccnet_amd.abn import InPlaceABN
    m = InPlaceABN(16)
    _randomise(m, 4)
    with torch.no_grad():
        m.weight[3] = 0.0
    m = m.to(DEV).train()
    x = torch.randn(2, 16, 33, 31, device=DEV)
    r = _oracle_check(m, x, torch.randn_like(x), tol=1e-2)
    assert all(torch.isfinite(r[k]).all() for k in ("y", "dx", "dw", "db")) and r["dw"][3].item() == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("project", [False, True], ids=["identity", "downsample"])
def test_fused_bottleneck_matches_the_stock_one(dtype, project):
    """The fused residual unit against the stock one run in float64 on the CPU: within 1e-3 of every quantity's scale in
    fp32; under bf16 autocast (bf16 convolutions) no further from it than twice the stock unit on the GPU, or 3e-2."""
    from ccnet_amd.abn import convert_abn
    from ccnet_amd.segmodel import Bottleneck
    torch.manual_seed(0)
    cin = 128 if project else 256
    stock = Bottleneck(cin, 64, stride=1, dilation=2, project=project)
    for m in stock.modules():
        if isinstance(m, inplace_abn.ABN):
            _randomise(m, m.num_features)
    fused = convert_abn(copy.deepcopy(stock), "device").to(DEV).train()
    exact = copy.deepcopy(stock).double().train()
    assert fused.bn3.fused_epilogues
    stock = stock.to(DEV).train()
    x = torch.randn(2, cin, 49, 47, device=DEV)
    dy = torch.randn(2, 256, 49, 47, device=DEV)
    outs = []
    for net, xx, dd in ((fused, x, dy), (stock, x, dy), (exact, x.double().cpu(), dy.double().cpu())):
        xi = xx.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16 and xx.is_cuda):
            y = net(xi)
        y.backward(dd.to(y.dtype))
        got = {"y": y.detach(), "dx": xi.grad}
        got.update({"grad." + n: p.grad for n, p in net.named_parameters()})
        got.update({"buf." + n: b.clone() for n, b in net.named_buffers()})
        outs.append(got)
    fz, st, ex = outs
    assert fz.keys() == ex.keys()
    err_f = {k: _rel(fz[k], ex[k]) for k in ex}
    err_s = {k: _rel(st[k], ex[k]) for k in ex}
    if dtype == torch.float32:
        assert all(v <= 1e-3 for v in err_f.values()), err_f
    else:
        assert all(err_f[k] <= max(2 * err_s[k], 3e-2) for k in ex), (err_f, err_s)


def test_results_repeat_bitwise_and_make_no_host_sync():
    from ccnet_amd.abn import ABN, InPlaceABN
    torch.manual_seed(0)
    x = torch.randn(2, 256, 97, 97, device=DEV)
    dy = torch.randn_like(x)
    res = torch.randn_like(x)
    for m in (ABN(256, activation="identity"), InPlaceABN(256)):
        _randomise(m, 5)
        m = m.to(DEV).train()
        runs = []
        for _ in range(2):
            m.running_mean.zero_()
            m.running_var.fill_(1)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                r = _run(m, x, dy, res if not m.inplace else None)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            runs.append(r)
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), k


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[4])
from ccnet_amd.abn import InPlaceABNSync
rank, rdv, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=2)
torch.cuda.set_device(0)
res = {}
for mode in ("oop", "inplace"):
    torch.manual_seed(0)
    m = InPlaceABNSync(64, activation="leaky_relu")
    with torch.no_grad():
        m.weight.uniform_(-1, 1); m.bias.uniform_(-0.5, 0.5)
    m.inplace = mode == "inplace"
    m = m.cuda().train()
    x = torch.randn(4, 64, 33, 35) * 2 + 1
    dy = torch.randn(4, 64, 33, 35)
    xi = x[2 * rank:2 * rank + 2].cuda().requires_grad_(True)
    y = m(xi * 1.0)
    y.backward(dy[2 * rank:2 * rank + 2].cuda())
    res[mode] = {"y": y.detach().cpu(), "dx": xi.grad.cpu(), "dw": m.weight.grad.cpu(), "db": m.bias.grad.cpu(),
                 "rm": m.running_mean.cpu(), "rv": m.running_var.cpu()}
torch.save(res, out)
dist.destroy_process_group()
"""


def test_cross_rank_statistics_over_two_gloo_ranks_match_one_process(tmp_path):
    from ccnet_amd.abn import InPlaceABNSync
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    root = os.path.dirname(HERE)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / "rdv"), str(tmp_path / f"r{r}.pt"), root])
             for r in range(2)]
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0, 0], codes
    halves = [torch.load(tmp_path / f"r{r}.pt") for r in range(2)]
    for mode in ("oop", "inplace"):
        torch.manual_seed(0)
        m = InPlaceABNSync(64, activation="leaky_relu")
        with torch.no_grad():
            m.weight.uniform_(-1, 1)
            m.bias.uniform_(-0.5, 0.5)
        m.inplace = mode == "inplace"
        m = m.to(DEV).train()
        x = torch.randn(4, 64, 33, 35) * 2 + 1
        dy = torch.randn(4, 64, 33, 35)
        whole = _run(m, x.to(DEV), dy.to(DEV))
        h = [hv[mode] for hv in halves]
        assert _rel(torch.cat([h[0]["y"], h[1]["y"]]), whole["y"]) <= 1e-5
        assert _rel(torch.cat([h[0]["dx"], h[1]["dx"]]), whole["dx"]) <= 1e-4
        assert _rel(h[0]["dw"] + h[1]["dw"], whole["dw"]) <= 1e-4 and _rel(h[0]["db"] + h[1]["db"], whole["db"]) <= 1e-4
        for k in ("rm", "rv"):
            assert torch.equal(h[0][k], h[1][k]) and _rel(h[0][k], whole[k]) <= 1e-5, k


def test_train_driver_losses_match_the_torch_layers():
    """--abn device and --abn inplace at 129^2: the first step's loss within 1e-4 relative of --abn torch (same weights and
    data; fp32 rounding only), the next two within 2e-3 (after SGD steps on slightly different gradients)"""
    from ccnet_amd import train_synthetic as TS
    out = {}
    for mode in ("torch", "device", "inplace"):
        args = TS.build_parser().parse_args(["--steps", "3", "--warmup", "0", "--size", "129", "--abn", mode])
        out[mode] = TS.run(args, quiet=True)
        assert out[mode]["abn"] == mode and out[mode]["max_memory_allocated_mb"] > 0
    ref = out["torch"]["step_losses"]
    assert len(ref) == 3 and all(np.isfinite(ref))
    for mode in ("device", "inplace"):
        got = out[mode]["step_losses"]
        assert abs(got[0] - ref[0]) <= 1e-4 * abs(ref[0]), (mode, got, ref)
        assert all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(got, ref)), (mode, got, ref)
