"""GPU checks of the channels_last device ABN (libccnet_abncl.so, ccnet_amd.abncl): the case table of tests/abncl_cases.py --
the one tests/test_abncl_host.py runs in the SIMT emulator -- through the gfx950 library on guarded device buffers, then the
Python layers: the backbone's shapes against the float64 oracle, in-place behaviour, agreement with the NCHW route,
determinism, graph capture, no host sync, two gloo ranks, and a training step with the converted convolutions.

The yardstick for values is the float64 CPU oracle (tests/abn_oracle.py).  Nothing here calls a stock batch norm on a bf16
channels_last device tensor directly: where a stock result on the device is wanted (the driver's --abn torch run) it goes
through conv3.NativeChannelsLast."""
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

import abn_cases as K  # noqa: E402
import abn_oracle as O  # noqa: E402
import abncl_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
CL = torch.channels_last


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _abncl_lib
    return _abncl_lib.get_lib()


@pytest.fixture(scope="module")
def mem(lib):
    return P.DeviceMemory()


# ---------------------------------------------------------------------------------------------------------------------
# the shared table over the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_slabs_case_splits_with_a_partial_last_slab(lib, bf16):
    S, chunk = P.splits(lib, P.SHAPES["slabs"], bf16)
    assert S >= 3 and 3034 % chunk != 0 and (S - 1) * chunk < 3034, (S, chunk)


@DTYPES
@pytest.mark.parametrize("shape,sem", P.GRID_CASES, ids=lambda v: v)
def test_edge_shapes(lib, mem, shape, sem, bf16):
    P.run_grid_case(lib, mem, shape, sem, bf16)


@DTYPES
@pytest.mark.parametrize("par,shape,sem", P.PARAMETER_CASES, ids=lambda v: v)
def test_parameter_forms(lib, mem, par, shape, sem, bf16):
    P.run_parameter_case(lib, mem, par, shape, sem, bf16)


@pytest.mark.parametrize("name,shape,bf16", P.NUMERIC_CASES, ids=lambda v: {False: "f32", True: "bf16"}.get(v, v))
def test_numeric_edges(lib, mem, name, shape, bf16):
    P.run_numeric_case(lib, mem, name, shape, bf16)


@DTYPES
@pytest.mark.parametrize("sem,shape", P.MISALIGNED_CASES, ids=lambda v: v)
def test_misaligned_tensors_give_the_aligned_result_bitwise(lib, mem, sem, shape, bf16):
    P.run_misaligned_case(lib, mem, sem, shape, bf16)


@pytest.mark.parametrize("N,R,sem", P.RANK_CASES, ids=lambda v: str(v))
def test_uneven_ranks_match_one(lib, mem, N, R, sem):
    P.run_rank_case(lib, mem, N, R, sem)


@pytest.mark.parametrize("sem", P.NONFINITE_CASES)
def test_non_finite_input_stays_in_its_channel_and_in_its_statistics(lib, mem, sem):
    P.run_nonfinite_case(lib, mem, sem)


@DTYPES
def test_c_abi_results_repeat_bitwise(lib, mem, bf16):
    P.run_repeat_case(lib, mem, "slabs", "ip_leaky01_res", bf16)


# ---------------------------------------------------------------------------------------------------------------------
# through ccnet_amd.abn / ccnet_amd.abncl
# ---------------------------------------------------------------------------------------------------------------------
ACTS = {"identity": (O.IDENTITY, 0.0), "relu": (O.RELU, 0.0), "leaky_relu": (O.LEAKY_RELU, 0.01), "elu": (O.ELU, 1.0)}
CLASSES = {"ABN": "relu", "InPlaceABNSync": "leaky_relu"}           # out of place with relu + residual; in place, leaky_relu


def _layer(cls, inputs, activation, training=True, channels_last=True):
    from ccnet_amd import abn
    _, w, b, rm, rv, _, _ = inputs
    m = getattr(abn, cls)(len(rm), activation=activation, activation_param=ACTS[activation][1] or 0.01)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w))
        m.bias.copy_(torch.from_numpy(b))
        m.running_mean.copy_(torch.from_numpy(rm))
        m.running_var.copy_(torch.from_numpy(rv))
    m.channels_last = channels_last
    return m.to(DEV).train(training)


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _dev(a, dtype=torch.float32, channels_last=True):
    if a is None:
        return None
    t = torch.from_numpy(a).to(DEV).to(dtype)
    return t.contiguous(memory_format=CL) if channels_last else t


def _dense_cl(t):
    return t.is_contiguous(memory_format=CL) and (not t.is_contiguous() or t.shape[1] == 1 or t.shape[2] * t.shape[3] == 1)


def _run(m, x, dy, residual=None):
    """one forward + backward of layer ``m`` on copies of the device tensors; the tensors themselves"""
    m.zero_grad(set_to_none=True)
    xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    xa = xi * 1.0 if m.inplace else xi                                     # an in-place layer cannot overwrite a leaf
    r = None if residual is None else residual.clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = m(xa, residual=r)
    if m.inplace:
        assert y.data_ptr() == xa.data_ptr()
    y.backward(dy)
    return {"y": y.detach(), "dx": xi.grad, "dresidual": None if r is None else r.grad, "dweight": m.weight.grad,
            "dbias": m.bias.grad, "running_mean": m.running_mean.clone(), "running_var": m.running_var.clone()}


def _check(r, inputs, m, activation, bf16):
    x, w, b, rm, rv, dy, res = inputs
    act, p = ACTS[activation]
    K.check_case({k: _np(v) for k, v in r.items()}, x, w, b, rm, rv, dy, res, training=m.training, act=act, p=p,
                 source=int(m.inplace), bf16=bf16, record=("gpu", "channels_last front end"))


_INPUTS = {}


def _inputs(shape):
    """one draw per shape, shared by the tests that use it and left unchanged"""
    if shape not in _INPUTS:
        _INPUTS[shape] = K.table_inputs(shape, K._seed("front end", *shape), residual=True)
    return _INPUTS[shape]


BACKBONE = [(2, 256, 33, 33), (1, 2048, 97, 97)]


@pytest.mark.parametrize("shape", BACKBONE, ids=lambda s: "x".join(map(str, s)))
@DTYPES
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_layers_on_channels_last_input_match_the_float64_oracle(lib, shape, bf16, training, cls):
    """the header's bars (abn_cases.check_case: fp32 1e-5 / 1e-4, bf16 2^-7 / 2^-6, the from-output oracle in place); y, dx and
    dresidual dense channels_last and of the input's dtype"""
    inputs = _inputs(shape)
    dt = torch.bfloat16 if bf16 else torch.float32
    m = _layer(cls, inputs, CLASSES[cls], training)
    x, dy, res = (_dev(inputs[i], dt) for i in (0, 5, 6))
    assert _dense_cl(x) and not x.is_contiguous()
    r = _run(m, x, dy, res)
    for k in ("y", "dx", "dresidual"):
        assert r[k].dtype == dt and r[k].shape == x.shape and _dense_cl(r[k]) and r[k].stride() == x.stride(), k
    _check(r, inputs, m, CLASSES[cls], bf16)


def test_in_place_output_shares_the_input_storage_and_misuse_raises(lib):
    from ccnet_amd.abn import InPlaceABNSync
    m = InPlaceABNSync(32).to(DEV).train()
    m.channels_last = True
    leaf = torch.randn(2, 32, 17, 19, device=DEV).contiguous(memory_format=CL).requires_grad_(True)
    x = leaf * 1.0
    assert _dense_cl(x) and not x.is_contiguous()
    v0, ptr = x._version, x.data_ptr()
    y = m(x)
    assert y.data_ptr() == ptr and x._version > v0 and y.stride() == x.stride()
    y.sum().backward()
    assert torch.isfinite(leaf.grad).all()
    x = leaf * 1.0
    other = (x * x).sum()
    y = m(x)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (other + y.sum()).backward()
    with pytest.raises(ValueError, match="dense channels_last"):
        m((leaf * 1.0)[:, :, :, ::2])


@DTYPES
@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_both_routes_meet_the_oracle_on_the_same_values(lib, cls, bf16):
    """the same values as NCHW through libccnet_abn.so and as channels_last through libccnet_abncl.so: every output of both
    routes within the header's bar of the oracle (not bit equality: the sums run in another order)"""
    shape = BACKBONE[0]
    inputs = _inputs(shape)
    dt = torch.bfloat16 if bf16 else torch.float32
    outs = {}
    for route, flag in (("nchw", False), ("channels_last", True)):
        m = _layer(cls, inputs, CLASSES[cls], channels_last=flag)
        x, dy, res = (_dev(inputs[i], dt, channels_last=flag) for i in (0, 5, 6))
        outs[route] = _run(m, x, dy, res)
        assert outs[route]["y"].is_contiguous() == (not flag)
        _check(outs[route], inputs, m, CLASSES[cls], bf16)
    # the two routes' statistics differ by summation order only
    for k in ("running_mean", "running_var"):
        K.close(_np(outs["channels_last"][k]), _np(outs["nchw"][k]), 1e-6, k)


def test_results_repeat_bitwise_make_no_host_sync_and_equal_a_replayed_graph(lib):
    inputs = _inputs(BACKBONE[0])
    x, dy, res = (_dev(inputs[i], torch.bfloat16) for i in (0, 5, 6))
    keys = ("y", "dx", "dresidual", "dweight", "dbias")
    for cls in sorted(CLASSES):
        m = _layer(cls, inputs, CLASSES[cls])
        _run(m, x, dy, res)                                         # (library loaded, allocator warm)
        runs = []
        for _ in range(2):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                runs.append(_run(m, x, dy, res))
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(runs[0][k], runs[1][k]), (cls, k)
        # one captured graph of forward + backward, replayed twice
        xs = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        rs = res.clone(memory_format=torch.preserve_format).requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                m(xs * 1.0, residual=rs).backward(dy)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        xs.grad = rs.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ys = m(xs * 1.0, residual=rs)
            ys.backward(dy)
        captured = {"y": ys.detach(), "dx": xs.grad, "dresidual": rs.grad, "dweight": m.weight.grad, "dbias": m.bias.grad}
        for _ in range(2):
            for t in captured.values():
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(captured[k], runs[0][k]), (cls, k)


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[4])
from ccnet_amd.abn import InPlaceABNSync
rank, rdv, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=2)
torch.cuda.set_device(0)
cl = torch.channels_last
res = {}
for mode in ("oop", "inplace"):
    torch.manual_seed(0)
    m = InPlaceABNSync(72, activation="leaky_relu")
    with torch.no_grad():
        m.weight.uniform_(-1, 1); m.bias.uniform_(-0.5, 0.5)
    m.inplace = mode == "inplace"
    m.channels_last = True
    m = m.cuda().train()
    x = torch.randn(4, 72, 33, 35) * 2 + 1
    dy = torch.randn(4, 72, 33, 35)
    xi = x[2 * rank:2 * rank + 2].cuda().contiguous(memory_format=cl).requires_grad_(True)
    y = m(xi * 1.0)
    assert y.is_contiguous(memory_format=cl) and not y.is_contiguous()
    y.backward(dy[2 * rank:2 * rank + 2].cuda().contiguous(memory_format=cl))
    res[mode] = {"y": y.detach().cpu(), "dx": xi.grad.cpu(), "dw": m.weight.grad.cpu(), "db": m.bias.grad.cpu(),
                 "rm": m.running_mean.cpu(), "rv": m.running_var.cpu()}
torch.save(res, out)
dist.destroy_process_group()
"""


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def test_cross_rank_statistics_over_two_gloo_ranks_match_one_process(lib, tmp_path):
    """as tests/test_gpu_abn.py's, on channels_last halves: the exchange and the Chan merge are the NCHW route's own"""
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
        m = InPlaceABNSync(72, activation="leaky_relu")
        with torch.no_grad():
            m.weight.uniform_(-1, 1)
            m.bias.uniform_(-0.5, 0.5)
        m.inplace = mode == "inplace"
        m.channels_last = True
        m = m.to(DEV).train()
        x = torch.randn(4, 72, 33, 35) * 2 + 1
        dy = torch.randn(4, 72, 33, 35)
        whole = _run(m, x.to(DEV).contiguous(memory_format=CL), dy.to(DEV).contiguous(memory_format=CL))
        h = [hv[mode] for hv in halves]
        assert _rel(torch.cat([h[0]["y"], h[1]["y"]]), whole["y"]) <= 1e-5
        assert _rel(torch.cat([h[0]["dx"], h[1]["dx"]]), whole["dx"]) <= 1e-4
        assert _rel(h[0]["dw"] + h[1]["dw"], whole["dweight"]) <= 1e-4
        assert _rel(h[0]["db"] + h[1]["db"], whole["dbias"]) <= 1e-4
        for k, name in (("rm", "running_mean"), ("rv", "running_var")):
            assert torch.equal(h[0][k], h[1][k]) and _rel(h[0][k], whole[name]) <= 1e-5, k


def test_segmodel_step_with_device_convolutions_and_channels_last_abn(lib, monkeypatch):
    """One Seg_Model step at 65 x 65 under bf16 parameters with convert_conv3x3 + convert_abn(model, 'device',
    channels_last=True), through the training driver: not one layout copy, no stock normalisation layer left, the fused
    epilogues reach the pixel-major function with a channels_last residual, and the loss is finite and within the margin of
    tests/test_gpu_abn.py::test_train_driver_losses_match_the_torch_layers of ``--abn torch --device-conv3`` (the stock
    layers through conv3.NativeChannelsLast) on the same seed.  That test holds every step to 2e-3 relative and, on top,
    its first step to 1e-4 because there the routes differ by "fp32 rounding only".  This run is bf16: the stock layer rounds
    its output to bf16 before the activation and again after the residual add where the fused layer rounds once, one bf16
    unit (2^-9 = 2e-3) per element and layer, so the first figure's premise does not hold and the margin here is that
    test's 2e-3.  Measured on an MI355X, two sessions: 8.8e-6 (4.208248 against 4.208211) and 4.5e-4 (4.211128 against
    4.209213); the stock route's own loss differed by 2.4e-4 between those sessions."""
    from ccnet_amd import abn, abncl, conv3
    from ccnet_amd import train_synthetic as T
    from ccnet_amd.segmodel import CriterionDSN, Seg_Model
    base = ["--bf16-params", "--device-conv3", "--size", "65", "--steps", "1", "--warmup", "0"]
    out, seen = {}, {}

    def factory():
        seen["model"] = Seg_Model(19, criterion=CriterionDSN(), recurrence=2)
        return seen["model"]

    residuals = []
    apply = abncl.ABNChannelsLastFunction.apply

    def recording(x, w, b, rm, rv, residual, cfg):
        if residual is not None:
            residuals.append(abncl.is_dense_channels_last(residual) and not residual.is_contiguous()
                             and abncl.is_dense_channels_last(x))
        return apply(x, w, b, rm, rv, residual, cfg)

    monkeypatch.setattr(abncl.ABNChannelsLastFunction, "apply", staticmethod(recording))
    for name, extra in (("torch", ["--abn", "torch"]), ("device", ["--abn", "device", "--abn-channels-last"])):
        before = conv3.layout_copies
        out[name] = T.run(T.parse_args(base + extra), model_factory=factory, quiet=True)
        print(name, "layout copies:", conv3.layout_copies - before, "losses:", out[name]["step_losses"])
        assert conv3.layout_copies - before == 0, name
        layers = [m for m in seen["model"].modules() if isinstance(m, inplace_abn.ABN)]
        assert len(layers) == 110
        if name == "device":
            twins = (abn.ABN, abn.InPlaceABN, abn.InPlaceABNSync)                          # no stock layer, no NativeChannelsLast
            assert all(type(m) in twins and m.channels_last and not m.inplace for m in layers)
            assert out[name]["abn_channels_last"] is True and out[name]["config"]["conv3"] == "device"
            assert out[name]["layout_copies"] == 0
            assert len(residuals) == 33 and all(residuals)                               # bn3 of the 33 residual units
        else:
            assert "abn_channels_last" not in out[name] and not residuals
    ref, got = out["torch"]["step_losses"], out["device"]["step_losses"]
    assert len(got) == 1 and np.isfinite(got[0]) and np.isfinite(ref[0]) and got[0] > 0
    assert abs(got[0] - ref[0]) <= 2e-3 * abs(ref[0]), (got, ref)
