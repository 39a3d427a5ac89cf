"""The mixed-precision optimiser kernels on the device (libccnet_sgdmp.so): the case table of tests/sgdmp_oracle.py through the
C ABI on guarded buffers, bit-exactly against the oracle; float32 rows against libccnet_sgd.so; ccnet_amd.optim.DeviceMixedSGD
against the oracle (bit-exact) and its masters against torch.optim.SGD over float32 copies (within DESIGN §22's bound); what a
master is for, in exact numbers; skipped gradients and version counters; the state_dict round trip; graph capture with the
schedule moving on; the training driver's --bf16-params."""
import copy
import math

import numpy as np
import pytest
import torch

import sgd_oracle as S
import sgdmp_oracle as M
from guarded_memory import DeviceMemory

pytestmark = pytest.mark.gpu

C = M.C
LR, MU, WD = M.DEFAULT
SIZES = [1, 2, 3, 5, 7, 9, 37, 300, C - 1, C, C + 1, 2 * C + 3]          # twelve parameters; the 37 sits one element off 16 bytes
BF16 = [t % 3 != 2 for t in range(len(SIZES))]                           # every third one is a float32 parameter
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from ccnet_amd import _sgdmp_lib
    return _sgdmp_lib.get_lib()


@pytest.fixture(scope="module")
def expected():
    """The oracle's answer per case, computed once and left unchanged"""
    return {name: M.expected(M.build_case(name)) for name in M.CASES}


def same_or_none(a, b):
    return (a is None and b is None) or np.array_equal(M.bits(a), M.bits(b))


@pytest.mark.parametrize("name", list(M.CASES))
def test_c_abi_matches_the_oracle_bit_exactly_on_guarded_buffers(lib, expected, name):
    case = M.build_case(name)
    code, got, intact = M.run_raw(lib, DeviceMemory(), case)
    assert code == 0, lib.last_error()
    assert intact
    M.assert_matches(case, got, expected[name])
    code, again, intact = M.run_raw(lib, DeviceMemory(), case)               # a second run from the same inputs
    assert code == 0 and intact and again[4] == got[4]
    for mine, theirs in zip(got[:4], again[:4]):
        assert all(same_or_none(a, b) for a, b in zip(mine, theirs))


def test_float32_rows_are_bit_identical_to_libccnet_sgd(lib):
    from ccnet_amd import _sgd_lib
    stock = _sgd_lib.get_lib()
    for name in S.CASES:
        scase = S.build_case(name)
        code, theirs, intact = S.run_raw(stock, DeviceMemory(), scase)
        assert code == 0 and intact, name
        code, mine, intact = M.run_raw(lib, DeviceMemory(), M.from_sgd_case(scase))
        assert code == 0 and intact, (name, lib.last_error())
        assert mine[4] == theirs[3], name
        for key, a_list, b_list in zip("pgb", mine[:3], theirs[:3]):
            assert all(same_or_none(a, b) for a, b in zip(a_list, b_list)), (name, key)


def test_a_refused_call_launches_nothing(lib):
    case = M.build_case("chunk_edges")

    def wrong_chunk(args):
        args["chunks_host"] = args["chunks_host"].copy()
        args["chunks_host"][3, 0] = 1
    code, got, intact = M.run_raw(lib, DeviceMemory(), case, wrong_chunk)
    assert code == -5 and "differs from the plan at entry 3" in lib.last_error()
    assert intact and M.unchanged(case, got)

    def odd_master(args):
        args["tensors_host"] = args["tensors_host"].copy()
        args["tensors_host"][1, 5] += 2
    code, got, intact = M.run_raw(lib, DeviceMemory(), case, odd_master)
    assert code == -8 and "tensor 1 has a master or momentum buffer that is not 4-byte" in lib.last_error()
    assert intact and M.unchanged(case, got)


def bf16_tensor(bits16):
    return torch.from_numpy(np.ascontiguousarray(bits16).view(np.int16)).view(torch.bfloat16)


def bits_of(t):
    """numpy bits of a device tensor: uint16 for bf16, float32 otherwise"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16).copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def off_16(data):
    """the tensor one element past a 16-byte boundary"""
    base = torch.zeros(data.numel() + 1, dtype=data.dtype, device="cuda")
    base[1:].copy_(data)
    assert base[1:].data_ptr() % 16 == data.element_size()
    return base[1:]


def make_params(seed=0, sizes=SIZES, bf16=BF16):
    """Seeded parameters on the device, bf16 where ``bf16`` says so; the one of 37 elements starts one element past a 16-byte
    boundary"""
    params = []
    for t, n in enumerate(sizes):
        values = S.make_data(n, 7000 + seed * 100 + t)
        data = bf16_tensor(M.bf16_of(values)) if bf16[t] else torch.from_numpy(values)
        params.append(torch.nn.Parameter(off_16(data) if n == 37 else data.cuda()))
    return params


def grads_of(step, sizes=SIZES, bf16=BF16):
    """numpy gradients: bf16 bit patterns for the bf16 parameters"""
    out = []
    for t, n in enumerate(sizes):
        g = S.make_data(n, 9000 + step * 100 + t)
        out.append(M.bf16_of(g) if bf16[t] else g)
    return out


def as_tensor(x):
    return (bf16_tensor(x) if x.dtype == np.uint16 else torch.from_numpy(x)).cuda()


def as_float(x):
    return M.float_of(x) if x.dtype == np.uint16 else x


def truth(opt, p):
    """the float32 tensor that holds the parameter's value: its master, or itself"""
    return opt.state[p]["master_param"] if p.dtype == torch.bfloat16 else p


def oracle_step(w, g, b, lr, mu, wd):
    """(w', b', p') on the float32 truth w: p' is bf16(w') for a bf16 gradient, else w' itself"""
    if g.dtype == np.uint16:
        return M.master_step(g, w, b, lr, mu, wd)
    nw, nb = S.sgd_step(w, g, b, lr, mu, wd)
    return nw, nb, nw


@pytest.mark.parametrize("zero_grads", [True, False], ids=["zeroing", "keeping"])
def test_device_mixed_sgd_runs_four_steps_bit_exactly_against_the_oracle(zero_grads):
    from ccnet_amd.optim import DeviceMixedSGD
    params = make_params()
    opt = DeviceMixedSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=zero_grads)
    for p, is16 in zip(params, BF16):
        state = opt.state[p]
        assert state["momentum_buffer"].dtype == torch.float32 and not state["momentum_buffer"].any()
        assert ("master_param" in state) == is16 == (p.dtype == torch.bfloat16)
        assert not is16 or (state["master_param"].dtype == torch.float32 and torch.equal(state["master_param"], p.detach().float()))
    w = [bits_of(truth(opt, p)) for p in params]
    b = [np.zeros(n, np.float32) for n in SIZES]
    shown = [None] * len(SIZES)
    ptrs = None
    for step in range(4):
        g = grads_of(step)
        for q, x in zip(params, g):
            if zero_grads and q.grad is not None:
                q.grad.copy_(as_tensor(x))                              # (zeroing: the .grad tensors stay where they are)
            else:
                q.grad = as_tensor(x)                                   # (keeping: new tensors every step, the tables follow)
            assert q.grad.dtype == q.dtype
        ptrs = [q.grad.data_ptr() for q in params] if ptrs is None else ptrs
        opt.step()
        for t in range(len(SIZES)):
            w[t], b[t], shown[t] = oracle_step(w[t], g[t], b[t], LR, MU, WD)
        if zero_grads:
            assert all(not bits_of(q.grad).view(np.uint8).any() for q in params) and [q.grad.data_ptr() for q in params] == ptrs
        else:
            assert all(M.same_bits(bits_of(q.grad), x) for q, x in zip(params, g))
    for t, q in enumerate(params):
        assert M.same_bits(bits_of(q), shown[t]), f"parameter {t} ({SIZES[t]} elements)"
        assert M.same_bits(bits_of(truth(opt, q)), w[t]), f"master {t} ({SIZES[t]} elements)"
        assert M.same_bits(bits_of(opt.state[q]["momentum_buffer"]), b[t]), f"buffer {t} ({SIZES[t]} elements)"


def bound_ratio(p0, g, b0, p1, b1, q1, c1, lr=LR, mu=MU, wd=WD):
    """The largest |difference| / bound over one tensor for (b, p), DESIGN §22's: per element |db| <= 4 u (|g| + wd |p| + mu |b|)
    and |dp| <= 4 u (|p| + lr |b'|) + lr tol_b, u = 2^-24."""
    p0, g, b0, p1, b1, q1, c1 = (np.asarray(a, np.float64) for a in (p0, g, b0, p1, b1, q1, c1))
    tol_b = 4 * U * (np.abs(g) + wd * np.abs(p0) + mu * np.abs(b0))
    tol_p = 4 * U * (np.abs(p0) + lr * np.abs(b1)) + lr * tol_b
    rb = np.abs(b1 - c1) / np.maximum(tol_b, 1e-300)
    rp = np.abs(p1 - q1) / np.maximum(tol_p, 1e-300)
    return float(rb.max()), float(rp.max())


def stock_twin(opt, params, **kw):
    """torch.optim.SGD over float32 copies of the parameters' truths"""
    twins = [torch.nn.Parameter(truth(opt, p).detach().clone()) for p in params]
    return twins, torch.optim.SGD(twins, lr=LR, momentum=MU, weight_decay=WD, **kw)


def feed(params, twins, g):
    """the same gradients to both: bf16 (or float32) to the parameters, float(g) to the float32 twins"""
    for p, q, x in zip(params, twins, g):
        p.grad, q.grad = as_tensor(x), torch.from_numpy(as_float(x).copy()).cuda()


def worst_ratio(opt, params, stock, twins, w0, b0, g):
    worst = (0.0, 0.0)
    for t, (p, q) in enumerate(zip(params, twins)):
        r = bound_ratio(w0[t], as_float(g[t]), b0[t], bits_of(truth(opt, p)), bits_of(opt.state[p]["momentum_buffer"]),
                        bits_of(q), bits_of(stock.state[q]["momentum_buffer"]))
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    return worst


@pytest.mark.parametrize("foreach", [True, False], ids=["foreach", "single_tensor"])
def test_masters_agree_with_torch_sgd_over_float32_copies_within_the_derived_bound(foreach):
    from ccnet_amd.optim import DeviceMixedSGD
    params = make_params(seed=1)
    opt = DeviceMixedSGD(params, lr=LR, momentum=MU, weight_decay=WD)
    twins, stock = stock_twin(opt, params, foreach=foreach)
    feed(params, twins, grads_of(10))                                         # a first step through both, so that buffers exist
    opt.step()
    stock.step()
    with torch.no_grad():                                                     # and the second one starts from the same state
        for p, q in zip(params, twins):
            truth(opt, p).copy_(q)
            opt.state[p]["momentum_buffer"].copy_(stock.state[q]["momentum_buffer"])
    g = grads_of(11)
    w0, b0 = [bits_of(truth(opt, p)) for p in params], [bits_of(opt.state[p]["momentum_buffer"]) for p in params]
    feed(params, twins, g)
    opt.step()
    stock.step()
    worst = worst_ratio(opt, params, stock, twins, w0, b0, g)
    print(f"DeviceMixedSGD masters against torch.optim.SGD(foreach={foreach}): worst |db| / bound {worst[0]:.3f}, "
          f"worst |dp| / bound {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    for p in params:                                                          # and every bf16 parameter is its master, rounded
        if p.dtype == torch.bfloat16:
            assert M.same_bits(bits_of(p), M.bf16_of(bits_of(truth(opt, p))))


def test_a_master_accumulates_updates_that_a_bf16_parameter_alone_would_lose():
    from ccnet_amd.optim import DeviceMixedSGD
    p = torch.nn.Parameter(torch.ones(9, dtype=torch.bfloat16, device="cuda"))
    opt = DeviceMixedSGD([p], lr=2.0 ** -11, momentum=0.0, weight_decay=0.0)
    lossy = torch.ones(9, dtype=torch.bfloat16, device="cuda")
    for _ in range(32):
        p.grad = torch.ones(9, dtype=torch.bfloat16, device="cuda")
        opt.step()
        lossy = (lossy.float() - 2.0 ** -11).to(torch.bfloat16)                # each update is below half a bf16 ulp at 1.0
    master = opt.state[p]["master_param"]
    assert master.dtype == torch.float32 and bool((master == 1 - 2.0 ** -6).all())
    assert bool((p.detach().float() == 1 - 2.0 ** -6).all())                   # 1 - 2^-6 is a bf16 number
    assert bool((lossy == 1.0).all())


def test_parameters_without_a_gradient_are_left_alone_and_versions_rise_by_one():
    from ccnet_amd.optim import DeviceMixedSGD
    params = make_params(seed=2)
    opt = DeviceMixedSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=True)
    skipped = {1, 6, 9, 11}
    for t, (p, x) in enumerate(zip(params, grads_of(20))):
        p.grad = None if t in skipped else as_tensor(x)
    with torch.no_grad():
        for p in params:
            opt.state[p]["momentum_buffer"].fill_(0.25)
    tensors = [[p, opt.state[p]["momentum_buffer"]] + ([truth(opt, p)] if p.dtype == torch.bfloat16 else []) for p in params]
    before = [[bits_of(x) for x in row] for row in tensors]
    versions = [[x._version for x in row] for row in tensors]
    grad_versions = [None if p.grad is None else p.grad._version for p in params]
    opt.step()
    for t, row in enumerate(tensors):
        if t in skipped:
            assert all(M.same_bits(bits_of(x), old) for x, old in zip(row, before[t])) and params[t].grad is None
            assert [x._version for x in row] == versions[t]
        else:
            assert not any(M.same_bits(bits_of(x), old) for x, old in zip(row, before[t]))
            assert [x._version for x in row] == [v + 1 for v in versions[t]]
            assert params[t].grad._version == grad_versions[t] + 1


def test_state_dict_round_trip_into_torch_sgd_and_back_and_masters_from_params():
    from ccnet_amd.optim import DeviceMixedSGD
    params = make_params(seed=3)
    opt = DeviceMixedSGD(params, lr=LR, momentum=MU, weight_decay=WD)
    for p, x in zip(params, grads_of(30)):
        p.grad = as_tensor(x)
    opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert all(v["momentum_buffer"].dtype == torch.float32 for v in saved["state"].values())
    assert sum("master_param" in v for v in saved["state"].values()) == sum(BF16)
    # into a fresh DeviceMixedSGD over other parameters of the same dtypes: masters and buffers arrive in float32, bit for bit,
    # and every bf16 parameter is rewritten from its master
    fresh = make_params(seed=5)
    again = DeviceMixedSGD(fresh, lr=LR, momentum=MU, weight_decay=WD)
    again.load_state_dict(copy.deepcopy(saved))
    for p, q in zip(params, fresh):
        assert again.state[q]["momentum_buffer"].dtype == torch.float32
        assert M.same_bits(bits_of(again.state[q]["momentum_buffer"]), bits_of(opt.state[p]["momentum_buffer"]))
        if p.dtype == torch.bfloat16:
            assert M.same_bits(bits_of(again.state[q]["master_param"]), bits_of(opt.state[p]["master_param"]))
            assert M.same_bits(bits_of(q), bits_of(p))
        else:
            assert "master_param" not in again.state[q]
    g = grads_of(31)
    for p, q, x in zip(params, fresh, g):
        p.grad, q.grad = as_tensor(x), as_tensor(x)
        if p.dtype == torch.float32:
            with torch.no_grad():
                q.copy_(p)                                                    # (a float32 parameter is the model's to load)
    opt.step()
    again.step()
    for p, q in zip(params, fresh):
        assert M.same_bits(bits_of(q), bits_of(p)) and M.same_bits(bits_of(truth(again, q)), bits_of(truth(opt, p)))
    # into stock over float32 copies, and one further step from each
    twins, stock = stock_twin(opt, params)
    stock.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(torch.equal(stock.state[q]["momentum_buffer"], opt.state[p]["momentum_buffer"]) for p, q in zip(params, twins))
    g = grads_of(32)
    w0, b0 = [bits_of(truth(opt, p)) for p in params], [bits_of(opt.state[p]["momentum_buffer"]) for p in params]
    feed(params, twins, g)
    opt.step()
    stock.step()
    assert max(worst_ratio(opt, params, stock, twins, w0, b0, g)) <= 1.0
    # and back: stock's state into a fresh DeviceMixedSGD, the float32 copies into the masters by hand
    mine = make_params(seed=6)
    back = DeviceMixedSGD(mine, lr=LR, momentum=MU, weight_decay=WD)
    back.load_state_dict(copy.deepcopy(stock.state_dict()))
    with torch.no_grad():
        for m, q in zip(mine, twins):
            truth(back, m).copy_(q)
            m.copy_(q)
    for m, q in zip(mine, twins):
        assert back.state[m]["momentum_buffer"].dtype == torch.float32
        assert torch.equal(back.state[m]["momentum_buffer"], stock.state[q]["momentum_buffer"])
    g = grads_of(33)
    w0, b0 = [bits_of(truth(back, m)) for m in mine], [bits_of(back.state[m]["momentum_buffer"]) for m in mine]
    feed(mine, twins, g)
    back.step()
    stock.step()
    assert max(worst_ratio(back, mine, stock, twins, w0, b0, g)) <= 1.0
    # a state without buffers and masters (a stock optimiser that has not stepped): zeros, and masters from the parameters
    empty = DeviceMixedSGD(make_params(seed=7), lr=LR, momentum=MU, weight_decay=WD)
    held = [p for group in empty.param_groups for p in group["params"]]
    empty.load_state_dict(torch.optim.SGD([torch.nn.Parameter(q.detach().clone()) for q in twins], lr=LR, momentum=MU,
                                          weight_decay=WD).state_dict())
    for p in held:
        assert not empty.state[p]["momentum_buffer"].any()
        assert p.dtype != torch.bfloat16 or torch.equal(empty.state[p]["master_param"], p.detach().float())
    # masters_from_params: the parameters were written from outside
    with torch.no_grad():
        for p in held:
            p.mul_(0.5)
    ptrs = [truth(empty, p).data_ptr() for p in held]
    empty.masters_from_params()
    assert [truth(empty, p).data_ptr() for p in held] == ptrs                 # in place
    assert all(torch.equal(truth(empty, p), p.detach().float()) for p in held)


def test_a_captured_step_replays_with_the_schedule_moving_on_and_a_moved_gradient_raises():
    from ccnet_amd.optim import DeviceMixedSGD, SgdmpError, poly_schedule
    sizes = [1, 5, 37, 300, C + 1, 2 * C + 3]
    kinds = [True, False, True, True, True, False]
    kw = dict(lr=1e-2, momentum=MU, weight_decay=WD, zero_grads=True)
    params, twins = make_params(4, sizes, kinds), make_params(4, sizes, kinds)
    opt = DeviceMixedSGD(params, schedule=poly_schedule(1e-2, 8), **kw)
    twin = DeviceMixedSGD(twins, schedule=poly_schedule(1e-2, 8), **kw)
    source = [torch.zeros(n, device="cuda", dtype=p.dtype) for n, p in zip(sizes, params)]
    for p, q in zip(params, twins):
        p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    keep = [truth(opt, p).detach().clone() for p in params]
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
                truth(opt, p).copy_(k)
                p.copy_(k)
                opt.state[p]["momentum_buffer"].zero_()
            opt.counter.zero_()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()                                                                # copies, the update, the counter: one chain
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == 0 and all(torch.equal(truth(opt, p), k) for p, k in zip(params, keep))      # captured, not run
    for k in range(3):
        g = grads_of(40 + k, sizes, kinds)
        for x, q, data in zip(source, twins, g):
            x.copy_(as_tensor(data))
            q.grad.copy_(as_tensor(data))
        graph.replay()
        twin.step()
        torch.cuda.synchronize()
    assert int(opt.counter.item()) == 3 == int(twin.counter.item())
    for t, (p, q) in enumerate(zip(params, twins)):
        assert M.same_bits(bits_of(p), bits_of(q)), t
        assert M.same_bits(bits_of(truth(opt, p)), bits_of(truth(twin, q))), t
        assert M.same_bits(bits_of(opt.state[p]["momentum_buffer"]), bits_of(twin.state[q]["momentum_buffer"])), t
        assert not bits_of(p.grad).view(np.uint8).any()
    # the three steps are the oracle's at the table's first three entries (tensor 4: a master row of C + 1 elements)
    table = poly_schedule(1e-2, 8).numpy()
    w, b, shown = keep[4].cpu().numpy(), np.zeros(sizes[4], np.float32), None
    for k in range(3):
        w, b, shown = oracle_step(w, grads_of(40 + k, sizes, kinds)[4], b, table[k], MU, WD)
    assert M.same_bits(bits_of(truth(opt, params[4])), w) and M.same_bits(bits_of(params[4]), shown)
    # a .grad that has moved cannot be followed during capture
    old = params[2].grad
    params[2].grad = torch.zeros_like(old)
    assert params[2].grad.data_ptr() != old.data_ptr()
    scratch = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    other = torch.cuda.CUDAGraph()
    with pytest.raises(SgdmpError, match="during stream capture"):
        with torch.cuda.graph(other, stream=s):
            scratch.add_(1.0)
            opt.step()
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == 3


class ToySegmenter(torch.nn.Module):
    """An ABN, two 1/8-resolution heads and the stock CriterionDSN: the shape of the real model's output, nothing of its cost"""

    def __init__(self):
        super().__init__()
        import inplace_abn

        from ccnet_amd.segmodel import CriterionDSN
        self.norm = inplace_abn.InPlaceABNSync(3)
        self.main = torch.nn.Linear(3, 19)
        self.aux = torch.nn.Linear(3, 19)
        self.criterion = CriterionDSN()

    def forward(self, images, labels):
        x = torch.nn.functional.avg_pool2d(self.norm(images), 8).permute(0, 2, 3, 1)       # (B, h, w, 3)
        return self.criterion([self.main(x).permute(0, 3, 1, 2), self.aux(x).permute(0, 3, 1, 2)], labels)


@pytest.mark.parametrize("abn", ["device", "inplace"])
def test_train_driver_with_bf16_params_takes_the_oracles_first_step_and_runs_on(monkeypatch, abn):
    from ccnet_amd import train_synthetic as T
    from ccnet_amd.optim import DeviceMixedSGD, poly_schedule
    argv = ["--bf16-params", "--abn", abn, "--size", "33", "--warmup", "0", "--batch-per-gpu", "2", "--lr", "1e-2",
            "--weight-decay", "5e-4"]
    res = T.run(T.parse_args(argv + ["--steps", "3"]), model_factory=ToySegmenter, quiet=True)
    assert res["steps"] == 3 and math.isfinite(res["final_loss"]) and res["final_loss"] > 0
    assert res["config"]["optimizer"] == "device-mixed-sgd+poly" and res["dtype"] == "bf16-params"
    seen = {}
    real = DeviceMixedSGD.step

    def spy(self, closure=None):
        seen["opt"] = self
        seen["params"] = [p for group in self.param_groups for p in group["params"]]
        seen["start"] = [bits_of(truth(self, p)) for p in seen["params"]]
        seen["grads"] = [bits_of(p.grad) for p in seen["params"]]
        return real(self, closure)
    monkeypatch.setattr(DeviceMixedSGD, "step", spy)
    T.run(T.parse_args(argv + ["--steps", "1"]), model_factory=ToySegmenter, quiet=True)
    lr = poly_schedule(1e-2, 1).numpy()[0]
    dtypes = [p.dtype for p in seen["params"]]
    assert len(seen["params"]) == 6 and dtypes == [torch.float32] * 2 + [torch.bfloat16] * 4        # the ABN's two stay float32
    assert all(g.view(np.uint8).any() for g in seen["grads"])
    for p, start, g in zip(seen["params"], seen["start"], seen["grads"]):
        assert g.dtype == (np.uint16 if p.dtype == torch.bfloat16 else np.float32)
        w, _, shown = oracle_step(start.reshape(-1), g.reshape(-1), np.zeros(g.size, np.float32), lr, 0.9, 5e-4)
        assert M.same_bits(bits_of(truth(seen["opt"], p)).reshape(-1), w)
        assert M.same_bits(bits_of(p).reshape(-1), shown)
        if p.dtype == torch.bfloat16:
            assert M.same_bits(bits_of(p).reshape(-1), M.bf16_of(bits_of(truth(seen["opt"], p)).reshape(-1)))
        assert not bits_of(p.grad).view(np.uint8).any()
