"""The fused CE + Lovász criterion on the MI355X (libccnet_celovasz.so through ccnet_amd.celovasz and through the raw C ABI on
guarded buffers) against the reference fixtures: loss, both terms, the gradient of the low-resolution logits, counts; the
variants and the cases the reference cannot run against the oracle; the recipe fixture of the stock criterion; bitwise
repeatability, two backwards and graph replay; bf16 logits; no host sync; the stock route on the device at the recipe shape;
peak memory; a Seg_Model training step against lovasz.CriterionOhemDSN2."""
import math

import numpy as np
import pytest
import torch

import celovasz_oracle as D
import lovasz_oracle as LO
from guarded_memory import DeviceMemory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = [n for n in D.CASES if n not in D.ORACLE_ONLY]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run_module(logits, target, dtype=torch.float32, backwards=1, **args):
    """forward + backward(s) through celovasz.UpsampledCELovasz; returns the result in the form celovasz_oracle.check_result
    takes, the loss and the gradient(s) as device tensors"""
    from ccnet_amd import celovasz
    x = torch.from_numpy(logits).to(DEV).to(dtype).requires_grad_(True)
    t = torch.from_numpy(target).to(DEV)
    crit = celovasz.UpsampledCELovasz(**args)
    loss = crit(x, t)
    assert type(loss.grad_fn).__name__ == "UpsampledCELovaszFunctionBackward" and loss.dtype == torch.float32
    grads = [torch.autograd.grad(loss, x, retain_graph=k + 1 < backwards)[0] for k in range(backwards)]
    torch.cuda.synchronize()
    r = {"loss": float(loss.detach()), "head_loss": crit.last_head_loss.cpu().numpy(), "valid": int(crit.last_num_valid.item()),
         "out_of_range": int(crit.last_num_out_of_range.item()), "n_kept": int(crit.last_n_kept.item()),
         "grad": grads[0].float().cpu().numpy()}
    return r, loss.detach(), grads


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity_through_the_module(name):
    fx = D.load_fixture(name)
    r, _, _ = run_module(fx["logits"], fx["target"])
    D.check_against_fixture(fx, r)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity_through_the_c_abi_on_guarded_buffers(name):
    """gradients, loss, counts and the workspace sit between guard bands; the gradients start as NaN, so every element is
    written; the second backward from the same workspace gives the same bits"""
    from ccnet_amd import _celovasz_lib
    fx = D.load_fixture(name)
    r = D.run_raw(_celovasz_lib.get_lib(), DeviceMemory(), fx["logits"], fx["target"])
    assert r["intact"] and np.array_equal(r["grad"], r["grad2"])
    D.check_against_fixture(fx, r)


@pytest.mark.parametrize("variant", list(D.VARIANTS))
def test_variants_of_s8_match_the_oracle(variant):
    from ccnet_amd import _celovasz_lib
    logits, target = D.case_inputs("s8")
    args = D.VARIANTS[variant]
    r, _, _ = run_module(logits, target, **args)
    D.check_against_oracle("s8/" + variant, logits, target, r, **args)
    q = D.run_raw(_celovasz_lib.get_lib(), DeviceMemory(), logits, target, **args)
    assert q["intact"] and q["loss"] == r["loss"] and np.array_equal(q["grad"], r["grad"])


@pytest.mark.parametrize("name", D.ORACLE_ONLY)
def test_oracle_only_cases_through_the_c_abi(name):
    from ccnet_amd import _celovasz_lib
    logits, target = D.case_inputs(name)
    r = D.run_raw(_celovasz_lib.get_lib(), DeviceMemory(), logits, target)
    assert r["intact"] and np.array_equal(r["grad"], r["grad2"])
    D.check_against_oracle(name, logits, target, r)
    if name == "ignored":
        assert np.isnan(r["loss"]) and not r["grad"].any()
    else:
        assert r["out_of_range"] > 7


@pytest.fixture(scope="module")
def recipe():
    """the stock criterion's fixture (tests/golden/make_lovasz_golden.py), read and not rewritten, and its inputs"""
    z = np.load(D.RECIPE_FIXTURE)
    main, aux, target = LO.make_criterion_inputs(int(z["seed"]))
    return z, main, aux, target


def test_recipe_fixture_of_the_stock_criterion(recipe):
    """(1, 19, 97, 97) -> 769 x 769 through CriterionOhemDSN2 with the reference's constructor; the DSN logits get no gradient"""
    from ccnet_amd import celovasz
    z, main, aux, target = recipe
    xm = torch.from_numpy(main).to(DEV).requires_grad_(True)
    xa = torch.from_numpy(aux).to(DEV).requires_grad_(True)
    loss = celovasz.CriterionOhemDSN2(ignore_index=255, thresh=0.7, min_kept=100000)([xm, xa], torch.from_numpy(target).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert xa.grad is None
    loss = loss.detach()
    rel = abs(float(loss) - float(z["loss"])) / abs(float(z["loss"]))
    err = np.abs(xm.grad.cpu().numpy().ravel()[z["grad_index"]] - z["grad_sample"]).max() / float(z["grad_absmax"])
    print(f"recipe: loss {float(loss)!r} reference {float(z['loss'])!r} relative error {rel:.3g} (bar {D.LOSS_RTOL:g}); gradient "
          f"max error {err:.3g} of max|grad| (bar {D.GRAD_RTOL:g})")
    assert rel <= D.LOSS_RTOL and err <= D.GRAD_RTOL


def test_two_runs_and_two_backwards_are_bit_identical(recipe):
    _, main, _, target = recipe
    _, l1, g1 = run_module(main, target, backwards=2)
    _, l2, g2 = run_module(main, target, backwards=2)
    assert torch.equal(l1, l2) and torch.equal(g1[0], g1[1]) and torch.equal(g1[0], g2[0]) and torch.equal(g2[0], g2[1])


def test_graph_replay_equals_eager_bitwise():
    """torch's capture recipe as tests/test_gpu_dsn.py follows it: every eager run that touches the captured tensors is on the
    one side stream that also captures, so the graph is a chain without parallel branches"""
    from ccnet_amd import celovasz
    fx = D.load_fixture("s8")
    crit = celovasz.UpsampledCELovasz()
    _, eager_loss, eager_grads = run_module(fx["logits"], fx["target"])
    eager = [eager_loss, eager_grads[0]]
    x = torch.from_numpy(fx["logits"]).to(DEV).requires_grad_(True)
    t = torch.from_numpy(fx["target"]).to(DEV)
    torch.cuda.synchronize()

    def step():
        loss = crit(x, t)
        return [loss.detach()] + list(torch.autograd.grad(loss, [x]))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        warm = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, warm))
    del warm
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = step()
    for out in captured:
        out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    assert int(crit.last_n_kept.item()) == int(fx["n_kept"])


def test_bf16_logits_under_autocast_give_fp32_loss_and_bf16_gradients():
    fx = D.load_fixture("s8")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss, grads = run_module(fx["logits"], fx["target"], dtype=torch.bfloat16)
    rounded = torch.from_numpy(fx["logits"]).to(torch.bfloat16).float().numpy()
    _, loss32, grads32 = run_module(rounded, fx["target"])                  # the fp32 path on the same rounded logits
    assert loss.dtype == torch.float32 and torch.equal(loss, loss32)
    g, g32 = grads[0], grads32[0]
    assert g.dtype == torch.bfloat16 and g.shape == g32.shape
    # one bf16 rounding (8 significand bits, round to nearest: half an ulp is 2^-9 relative) of the fp32 gradient
    assert bool(((g.float() - g32).abs() <= 2.0 ** -8 * g32.abs() + 1e-30).all())


def test_no_host_sync_in_forward_and_backward():
    from ccnet_amd import celovasz
    logits, target = D.case_inputs("s8")
    x = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    t = torch.from_numpy(target).to(DEV)
    for args in (dict(), dict(classes=[1, 2, 2], per_image=True)):
        crit = celovasz.UpsampledCELovasz(**args)
        crit(x, t).backward()                                    # warm: library load, allocator
        torch.cuda.synchronize()
        x.grad = None
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = crit(x, t)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item()) and x.grad is not None


def _growth(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_recipe_agrees_with_the_stock_route_on_the_device_and_stays_below_it_in_memory(recipe):
    """lovasz.CriterionOhemDSN2 (stock up-sample, softmax and cross-entropy around the Lovász kernels) on the same device
    tensors: loss and gradient within the bars; the fused step's peak growth is at most its workspace + three low-resolution
    tensors + 1 MiB, and at least two full-resolution class maps below the stock step's, measured here"""
    from ccnet_amd import _celovasz_lib, celovasz, lovasz
    _, main, aux, target = recipe
    B, C, h, w = main.shape
    H, W = target.shape[1:]
    t = torch.from_numpy(target).to(DEV)
    aux_d = torch.from_numpy(aux).to(DEV)
    res, growth = {}, {}
    for name, crit in (("stock", lovasz.CriterionOhemDSN2()), ("fused", celovasz.CriterionOhemDSN2())):
        x = torch.from_numpy(main).to(DEV).requires_grad_(True)

        def step():
            x.grad = None
            loss = crit([x, aux_d], t)
            loss.backward()
            res[name] = (loss.detach(), x.grad)

        step()                                                   # (a first call: the library is loaded, the allocator warm)
        res.pop(name)
        x.grad = None
        growth[name] = _growth(step)
    (l0, g0), (l1, g1) = res["stock"], res["fused"]
    rel = abs(float(l1) - float(l0)) / abs(float(l0))
    err = float((g1 - g0).abs().max()) / float(g0.abs().max())
    nbytes = _celovasz_lib.get_lib().ccnet_celovasz_workspace_bytes(B, C, h, w, H, W, 0)
    full, low = 4 * B * C * H * W, 4 * B * C * h * w
    print(f"recipe, fused against stock on the device: loss {float(l1)!r} vs {float(l0)!r} relative {rel:.3g}; gradient max error "
          f"{err:.3g} of max|grad|; peak growth fused {growth['fused'] / 2 ** 20:.1f} MiB (workspace {nbytes / 2 ** 20:.1f} MiB), "
          f"stock {growth['stock'] / 2 ** 20:.1f} MiB; one full-resolution class map {full / 2 ** 20:.1f} MiB")
    assert rel <= D.LOSS_RTOL and err <= D.GRAD_RTOL
    assert growth["fused"] <= nbytes + 3 * low + (1 << 20)
    assert growth["fused"] <= growth["stock"] - 2 * full


@pytest.fixture(scope="module")
def seg_model_steps():
    """One training step of Seg_Model(19) on a 65 x 65 crop, on the same weights, input and dropout masks (reseeded), with
    lovasz.CriterionOhemDSN2() (stock ops around the Lovász kernels), with the fused criterion, and with the stock one again;
    deterministic convolutions, as tests/test_gpu_dsn.py explains.  Per run: loss and the first convolution's gradient."""
    from ccnet_amd import celovasz, lovasz
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 65, 65, generator=g).to(DEV)
    labels = torch.randint(0, 19, (2, 65, 65), generator=g)
    labels[torch.rand(2, 65, 65, generator=g) < 0.1] = 255
    labels = labels.to(DEV)
    res = {}
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for name, crit in (("stock", lovasz.CriterionOhemDSN2()), ("fused", celovasz.CriterionOhemDSN2()),
                           ("stock again", lovasz.CriterionOhemDSN2())):
            model.criterion = crit
            model.zero_grad(set_to_none=True)
            torch.manual_seed(7)                              # the same Dropout2d masks in every run
            loss = model(x, labels)
            loss.backward()
            torch.cuda.synchronize()
            res[name] = (float(loss.detach()), model.conv1.weight.grad.double().cpu().numpy().copy())
    finally:
        torch.backends.cudnn.deterministic = keep
    l0, g0 = res["stock"]
    for name in ("fused", "stock again"):
        l, gr = res[name]
        print(f"{name}: loss {l!r} (stock {l0!r}); conv1 gradient max error {np.abs(gr - g0).max():.3g} of max|grad| "
              f"{np.abs(g0).max():.3g}")
    return res


def test_seg_model_training_step_repeats_itself_with_the_stock_criterion(seg_model_steps):
    """the reference of the test below is a reference only if it reproduces itself"""
    a, b = seg_model_steps["stock"], seg_model_steps["stock again"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_seg_model_training_step_matches_the_stock_criterion(seg_model_steps):
    (l0, g0), (l1, g1) = seg_model_steps["stock"], seg_model_steps["fused"]
    assert math.isfinite(l0) and abs(l1 - l0) <= D.LOSS_RTOL * abs(l0)
    assert np.abs(g0).max() > 0 and np.abs(g1 - g0).max() <= D.GRAD_RTOL * np.abs(g0).max()
