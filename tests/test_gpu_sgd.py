"""The optimiser kernels on the device (libccnet_sgd.so): the case table of tests/sgd_oracle.py through the C ABI on guarded
buffers, bit-exactly against the float32 oracle; ccnet_amd.optim.DeviceSGD against the oracle (bit-exact) and against
torch.optim.SGD (within a derived bound); skipped gradients and version counters; the state_dict round trip; graph capture with
the schedule moving on; the training driver's --device-sgd."""
import copy
import math

import numpy as np
import pytest
import torch

import sgd_oracle as S
from guarded_memory import DeviceMemory

pytestmark = pytest.mark.gpu

C = S.C
LR, MU, WD = S.DEFAULT
SIZES = [1, 2, 3, 5, 7, 9, 37, 300, C - 1, C, C + 1, 2 * C + 3]          # twelve parameters; the 37 sits one element off 16 bytes
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from ccnet_amd import _sgd_lib
    return _sgd_lib.get_lib()


@pytest.fixture(scope="module")
def expected():
    """The oracle's answer per case, computed once and left unchanged"""
    return {name: S.expected(S.build_case(name)) for name in S.CASES}


@pytest.mark.parametrize("name", list(S.CASES))
def test_c_abi_matches_the_oracle_bit_exactly_on_guarded_buffers(lib, expected, name):
    case = S.build_case(name)
    code, got, intact = S.run_raw(lib, DeviceMemory(), case)
    assert code == 0, lib.last_error()
    assert intact
    S.assert_matches(case, got, expected[name])
    code, again, intact = S.run_raw(lib, DeviceMemory(), case)               # a second run from the same inputs
    assert code == 0 and intact and again[3] == got[3]
    for mine, theirs in zip(got[:3], again[:3]):
        assert all(a is b is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(mine, theirs))


def test_a_refused_call_launches_nothing(lib):
    case = S.build_case("chunk_edges")

    def wrong_chunk(args):
        args["chunks_host"] = args["chunks_host"].copy()
        args["chunks_host"][3, 0] = 1
    code, got, intact = S.run_raw(lib, DeviceMemory(), case, wrong_chunk)
    assert code == -5 and "differs from the plan at entry 3" in lib.last_error()
    assert intact and S.unchanged(case, got)


def make_params(seed=0, sizes=SIZES):
    """Seeded parameters on the device; the one of 37 elements starts 4 bytes past a 16-byte boundary"""
    params = []
    for t, n in enumerate(sizes):
        data = torch.from_numpy(S.make_data(n, 7000 + seed * 100 + t))
        if n == 37:
            base = torch.zeros(n + 1, device="cuda")
            base[1:].copy_(data)
            params.append(torch.nn.Parameter(base[1:]))
            assert params[-1].data_ptr() % 16 == 4
        else:
            params.append(torch.nn.Parameter(data.cuda()))
    return params


def grads_of(step, sizes=SIZES):
    return [S.make_data(n, 9000 + step * 100 + t) for t, n in enumerate(sizes)]


def numpy_of(tensors):
    return [t.detach().cpu().numpy().copy() for t in tensors]


def buffers(opt, params):
    return [opt.state[p]["momentum_buffer"] for p in params]


@pytest.mark.parametrize("zero_grads", [True, False], ids=["zeroing", "keeping"])
def test_device_sgd_runs_four_steps_bit_exactly_against_the_oracle(zero_grads):
    from ccnet_amd.optim import DeviceSGD
    params = make_params()
    opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=zero_grads)
    assert all(not b.any() for b in buffers(opt, params))
    p, b = numpy_of(params), [np.zeros(n, np.float32) for n in SIZES]
    ptrs = None
    for step in range(4):
        g = grads_of(step)
        for q, x in zip(params, g):
            if zero_grads and q.grad is not None:
                q.grad.copy_(torch.from_numpy(x))                       # (zeroing: the .grad tensors stay where they are)
            else:
                q.grad = torch.from_numpy(x).cuda()                     # (keeping: new tensors every step, the tables follow)
        ptrs = [q.grad.data_ptr() for q in params] if ptrs is None else ptrs
        opt.step()
        for t in range(len(SIZES)):
            p[t], b[t] = S.sgd_step(p[t], g[t], b[t], LR, MU, WD)
        if zero_grads:
            assert all(not q.grad.any() for q in params) and [q.grad.data_ptr() for q in params] == ptrs
        else:
            assert all(S.same_bits(q.grad.cpu().numpy(), x) for q, x in zip(params, g))
    for t, (q, buf) in enumerate(zip(params, buffers(opt, params))):
        assert S.same_bits(q.detach().cpu().numpy(), p[t]), f"parameter {t} ({SIZES[t]} elements)"
        assert S.same_bits(buf.cpu().numpy(), b[t]), f"buffer {t} ({SIZES[t]} elements)"


def bound_ratio(p0, g, b0, p1, b1, q1, c1, lr=LR, mu=MU, wd=WD):
    """The largest |difference| / bound over one tensor for (b, p): per element |db| <= 4 u (|g| + wd |p| + mu |b|) and
    |dp| <= 4 u (|p| + lr |b'|) + lr tol_b, u = 2^-24.  Each of the three multiply-adds may differ by the rounding of its
    product plus one neighbour at the final rounding (2 u of the larger operand), doubled for margin."""
    p0, g, b0, p1, b1, q1, c1 = (np.asarray(a, np.float64) for a in (p0, g, b0, p1, b1, q1, c1))
    tol_b = 4 * U * (np.abs(g) + wd * np.abs(p0) + mu * np.abs(b0))
    tol_p = 4 * U * (np.abs(p0) + lr * np.abs(b1)) + lr * tol_b
    rb = np.abs(b1 - c1) / np.maximum(tol_b, 1e-300)
    rp = np.abs(p1 - q1) / np.maximum(tol_p, 1e-300)
    return float(rb.max()), float(rp.max())


def stock_twin(params, **kw):
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    return twins, torch.optim.SGD(twins, lr=LR, momentum=MU, weight_decay=WD, **kw)


@pytest.mark.parametrize("foreach", [True, False], ids=["foreach", "single_tensor"])
def test_device_sgd_agrees_with_torch_sgd_within_the_derived_bound(foreach):
    from ccnet_amd.optim import DeviceSGD
    params = make_params(seed=1)
    twins, stock = stock_twin(params, foreach=foreach)
    for q, x in zip(twins, grads_of(10)):                                     # a first step through stock, so that buffers exist
        q.grad = torch.from_numpy(x).cuda()
    stock.step()
    opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD)
    with torch.no_grad():
        for p, q in zip(params, twins):
            p.copy_(q)
            opt.state[p]["momentum_buffer"].copy_(stock.state[q]["momentum_buffer"])
    g = grads_of(11)
    p0, b0 = numpy_of(params), numpy_of(buffers(opt, params))
    for p, q, x in zip(params, twins, g):
        p.grad, q.grad = torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda()
    opt.step()
    stock.step()
    worst = (0.0, 0.0)
    for t, (p, q) in enumerate(zip(params, twins)):
        r = bound_ratio(p0[t], g[t], b0[t], p.detach().cpu().numpy(), opt.state[p]["momentum_buffer"].cpu().numpy(),
                        q.detach().cpu().numpy(), stock.state[q]["momentum_buffer"].cpu().numpy())
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"DeviceSGD against torch.optim.SGD(foreach={foreach}): worst |db| / bound {worst[0]:.3f}, worst |dp| / bound {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


def test_parameters_without_a_gradient_are_left_alone_and_versions_rise_by_one():
    from ccnet_amd.optim import DeviceSGD
    params = make_params(seed=2)
    opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=True)
    skipped = {1, 6, 9}
    for t, (p, x) in enumerate(zip(params, grads_of(20))):
        p.grad = None if t in skipped else torch.from_numpy(x).cuda()
    with torch.no_grad():
        for b in buffers(opt, params):
            b.fill_(0.25)
    before = numpy_of(params)
    versions = [(p._version, b._version) for p, b in zip(params, buffers(opt, params))]
    opt.step()
    for t, (p, b) in enumerate(zip(params, buffers(opt, params))):
        if t in skipped:
            assert S.same_bits(p.detach().cpu().numpy(), before[t]) and bool((b == 0.25).all()) and p.grad is None
            assert (p._version, b._version) == versions[t]
        else:
            assert not S.same_bits(p.detach().cpu().numpy(), before[t])
            assert (p._version, b._version) == (versions[t][0] + 1, versions[t][1] + 1)


def test_state_dict_loads_into_torch_sgd_and_back():
    from ccnet_amd.optim import DeviceSGD
    params = make_params(seed=3)
    opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD)
    for p, x in zip(params, grads_of(30)):
        p.grad = torch.from_numpy(x).cuda()
    opt.step()
    # into stock, and one further step from each
    twins, stock = stock_twin(params)
    stock.load_state_dict(copy.deepcopy(opt.state_dict()))              # (load_state_dict may keep the tensors it is given)
    assert all(torch.equal(stock.state[q]["momentum_buffer"], opt.state[p]["momentum_buffer"]) for p, q in zip(params, twins))
    g = grads_of(31)
    p0, b0 = numpy_of(params), numpy_of(buffers(opt, params))
    for p, q, x in zip(params, twins, g):
        p.grad, q.grad = torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda()
    opt.step()
    stock.step()
    for t, (p, q) in enumerate(zip(params, twins)):
        r = bound_ratio(p0[t], g[t], b0[t], p.detach().cpu().numpy(), opt.state[p]["momentum_buffer"].cpu().numpy(),
                        q.detach().cpu().numpy(), stock.state[q]["momentum_buffer"].cpu().numpy())
        assert max(r) <= 1.0, (t, r)
    # and back: stock's state into a fresh DeviceSGD over stock's parameters, one further step from each
    mine = [torch.nn.Parameter(q.detach().clone()) for q in twins]
    back = DeviceSGD(mine, lr=LR, momentum=MU, weight_decay=WD)
    back.load_state_dict(copy.deepcopy(stock.state_dict()))
    assert all(torch.equal(back.state[m]["momentum_buffer"], stock.state[q]["momentum_buffer"]) for m, q in zip(mine, twins))
    g = grads_of(32)
    p0, b0 = numpy_of(mine), numpy_of(buffers(back, mine))
    for m, q, x in zip(mine, twins, g):
        m.grad, q.grad = torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda()
    back.step()
    stock.step()
    for t, (m, q) in enumerate(zip(mine, twins)):
        r = bound_ratio(p0[t], g[t], b0[t], m.detach().cpu().numpy(), back.state[m]["momentum_buffer"].cpu().numpy(),
                        q.detach().cpu().numpy(), stock.state[q]["momentum_buffer"].cpu().numpy())
        assert max(r) <= 1.0, (t, r)
    # a state without buffers (a stock optimiser that has not stepped) loads as zeros
    fresh = [torch.nn.Parameter(q.detach().clone()) for q in twins]
    empty = DeviceSGD(fresh, lr=LR, momentum=MU, weight_decay=WD)
    empty.load_state_dict(torch.optim.SGD([torch.nn.Parameter(q.detach().clone()) for q in twins], lr=LR, momentum=MU,
                                          weight_decay=WD).state_dict())
    start = numpy_of(fresh)
    for m, x in zip(fresh, g):
        m.grad = torch.from_numpy(x).cuda()
    empty.step()
    for b, p_, x in zip(buffers(empty, fresh), start, g):
        assert S.same_bits(b.cpu().numpy(), S.sgd_step(p_, x, np.zeros_like(x), LR, MU, WD)[1])


def test_a_captured_step_replays_with_the_schedule_moving_on_and_a_moved_gradient_raises():
    from ccnet_amd.optim import DeviceSGD, SgdError, poly_schedule
    sizes = [1, 5, 37, 300, C + 1, 2 * C + 3]
    kw = dict(lr=1e-2, momentum=MU, weight_decay=WD, zero_grads=True)
    params, twins = make_params(seed=4, sizes=sizes), make_params(seed=4, sizes=sizes)
    opt = DeviceSGD(params, schedule=poly_schedule(1e-2, 8), **kw)
    twin = DeviceSGD(twins, schedule=poly_schedule(1e-2, 8), **kw)
    source = [torch.zeros(n, device="cuda") for n in sizes]
    for p, q in zip(params, twins):
        p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    keep = [p.detach().clone() for p in params]
    torch.cuda.synchronize()

    def step():
        for p, x in zip(params, source):
            p.grad.copy_(x)
        opt.step()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                                # warm-up: builds the tables
        with torch.no_grad():                                                 # and the state goes back to where it was
            for p, k in zip(params, keep):
                p.copy_(k)
                opt.state[p]["momentum_buffer"].zero_()
            opt.counter.zero_()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()                                                                # copies, the update, the counter: one chain
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == 0 and all(torch.equal(p, k) for p, k in zip(params, keep))      # captured, not run
    for k in range(3):
        g = grads_of(40 + k, sizes)
        for x, q, data in zip(source, twins, g):
            x.copy_(torch.from_numpy(data))
            q.grad.copy_(torch.from_numpy(data))
        graph.replay()
        twin.step()
        torch.cuda.synchronize()
    assert int(opt.counter.item()) == 3 == int(twin.counter.item())
    for t, (p, q) in enumerate(zip(params, twins)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), t
        assert torch.equal(opt.state[p]["momentum_buffer"].view(torch.int32), twin.state[q]["momentum_buffer"].view(torch.int32)), t
        assert not p.grad.any()
    # the twin's three eager steps are the oracle's at the table's first three entries
    table = poly_schedule(1e-2, 8).numpy()
    p0, b0 = keep[4].cpu().numpy(), np.zeros(sizes[4], np.float32)
    for k in range(3):
        p0, b0 = S.sgd_step(p0, grads_of(40 + k, sizes)[4], b0, table[k], MU, WD)
    assert S.same_bits(params[4].detach().cpu().numpy(), p0)
    # a .grad that has moved cannot be followed during capture
    old = params[1].grad
    params[1].grad = torch.zeros_like(old)
    assert params[1].grad.data_ptr() != old.data_ptr()
    scratch = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    other = torch.cuda.CUDAGraph()
    with pytest.raises(SgdError, match="during stream capture"):
        with torch.cuda.graph(other, stream=s):
            scratch.add_(1.0)
            opt.step()
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == 3


class ToySegmenter(torch.nn.Module):
    """Two 1/8-resolution heads and the stock CriterionDSN: the shape of the real model's output, nothing of its cost"""

    def __init__(self):
        super().__init__()
        from ccnet_amd.segmodel import CriterionDSN
        self.main = torch.nn.Linear(3, 19)
        self.aux = torch.nn.Linear(3, 19)
        self.criterion = CriterionDSN()

    def forward(self, images, labels):
        x = torch.nn.functional.avg_pool2d(images, 8).permute(0, 2, 3, 1)                  # (B, h, w, 3)
        return self.criterion([self.main(x).permute(0, 3, 1, 2), self.aux(x).permute(0, 3, 1, 2)], labels)


def test_train_driver_with_device_sgd_takes_the_oracles_first_step_and_runs_on(monkeypatch):
    from ccnet_amd import train_synthetic as T
    from ccnet_amd.optim import DeviceSGD, poly_schedule
    argv = ["--device-sgd", "--size", "33", "--warmup", "0", "--batch-per-gpu", "2", "--lr", "1e-2", "--weight-decay", "5e-4"]
    res = T.run(T.parse_args(argv + ["--steps", "3"]), model_factory=ToySegmenter, quiet=True)
    assert res["steps"] == 3 and math.isfinite(res["final_loss"]) and res["final_loss"] > 0
    assert res["config"]["optimizer"] == "device-sgd+poly"
    plain = T.run(T.parse_args([a for a in argv if a != "--device-sgd"] + ["--steps", "1"]), model_factory=ToySegmenter, quiet=True)
    assert plain["config"]["optimizer"] == "sgd+poly"
    seen = {}
    real = DeviceSGD.step

    def spy(self, closure=None):
        seen["params"] = [p for group in self.param_groups for p in group["params"]]
        seen["start"], seen["grads"] = numpy_of(seen["params"]), numpy_of([p.grad for p in seen["params"]])
        return real(self, closure)
    monkeypatch.setattr(DeviceSGD, "step", spy)
    T.run(T.parse_args(argv + ["--steps", "1"]), model_factory=ToySegmenter, quiet=True)
    lr = poly_schedule(1e-2, 1).numpy()[0]
    assert len(seen["params"]) == 4 and all(g.any() for g in seen["grads"])
    for p, start, g in zip(seen["params"], seen["start"], seen["grads"]):
        want, _ = S.sgd_step(start.reshape(-1), g.reshape(-1), np.zeros(g.size, np.float32), lr, 0.9, 5e-4)
        assert S.same_bits(p.detach().cpu().numpy().reshape(-1), want)
        assert not p.grad.any()
