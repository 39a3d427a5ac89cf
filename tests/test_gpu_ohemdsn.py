"""The fused OHEM + DSN criterion on the MI355X (libccnet_ohemdsn.so through ccnet_amd.ohemdsn and through the raw C ABI on
guarded buffers) against the reference fixtures: threshold, kept mask, loss, both heads' gradients, counts; the scale-1 case
against the device OhemCrossEntropy2d; tie groups; bitwise repeatability and graph replay; bf16 logits; peak memory; a
Seg_Model training step against ohem.CriterionOhemDSN."""
import math

import numpy as np
import pytest
import torch

import ohem_oracle as O
import ohemdsn_oracle as D
from guarded_memory import DeviceMemory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = [n for n in D.CASES if n not in D.ORACLE_ONLY]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def to_dev(logits, target, dtype=torch.float32):
    xs = [torch.from_numpy(l).to(DEV).to(dtype).requires_grad_(True) for l in logits]
    return xs, torch.from_numpy(target).to(DEV)


def run_module(logits, target, dtype=torch.float32, **args):
    """forward + backward through ohemdsn.CriterionOhemDSN (UpsampledOhemCrossEntropy2d for one head); returns the result in
    the form ohemdsn_oracle.check_result takes -- the kept mask read from the workspace the autograd node saved -- and the
    module"""
    from ccnet_amd import ohemdsn
    xs, t = to_dev(logits, target, dtype)
    if len(xs) == 2:
        crit = ohemdsn.CriterionOhemDSN(**args)
        loss = crit(xs, t)
    else:
        crit = ohemdsn.UpsampledOhemCrossEntropy2d(**args)
        loss = crit(xs[0], t)
    assert type(loss.grad_fn).__name__ == "UpsampledOhemFunctionBackward"
    ws = loss.grad_fn.saved_tensors[0]
    loss.backward()
    torch.cuda.synchronize()
    B, H, W = target.shape
    r = {"loss": float(loss.detach()), "head_loss": crit.last_head_loss.cpu().numpy(), "threshold": crit.last_threshold.item(),
         "kept": int(crit.last_kept.item()), "valid": int(crit.last_num_valid.item()),
         "out_of_range": int(crit.last_num_out_of_range.item()),
         "kept_mask": D.workspace_kept_mask(ws.cpu().numpy(), B, H, W, len(xs)), "grads": [x.grad.float().cpu().numpy() for x in xs]}
    return r, crit, loss.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity_through_the_module(name):
    fx = D.load_fixture(name)
    r, crit, loss, _ = run_module(fx["logits"], fx["target"], **fx["args"])
    r["num_valid_zoomed"] = int(fx["num_valid_zoomed"])                    # (the module does not expose the zoomed count)
    assert loss.dtype == torch.float32 and crit.last_threshold.dtype == torch.float32
    D.check_against_fixture(fx, r)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity_through_the_c_abi_on_guarded_buffers(name):
    """gradients, loss, threshold, counts and the workspace sit between guard bands; the gradients start as NaN, so every
    element is written"""
    from ccnet_amd import _ohemdsn_lib
    fx = D.load_fixture(name)
    r = D.run_raw(_ohemdsn_lib.get_lib(), DeviceMemory(), fx["logits"], fx["target"], **fx["args"])
    assert r["intact"]
    D.check_against_fixture(fx, r)


@pytest.mark.parametrize("name", D.ORACLE_ONLY)
def test_oracle_only_cases_through_the_c_abi(name):
    from ccnet_amd import _ohemdsn_lib
    logits, target, args = D.case_inputs(name)
    r = D.run_raw(_ohemdsn_lib.get_lib(), DeviceMemory(), logits, target, **args)
    assert r["intact"] and r["threshold"] == 1.0 and r["num_valid_zoomed"] == 0
    D.check_against_oracle(name, logits, target, args, r)


def test_identity_case_has_the_device_ohem_criterions_threshold_bits_and_mask():
    """scale 1: the interpolated logits are the logits (l1 = 0 on both axes), so the fused criterion must select exactly what
    libccnet_ohem selects on the same tensor"""
    from ccnet_amd.ohem import OhemCrossEntropy2d
    fx = D.load_fixture("identity")
    r, _, _, _ = run_module(fx["logits"], fx["target"], **fx["args"])
    x = torch.from_numpy(fx["logits"][0]).to(DEV).requires_grad_(True)
    crit = OhemCrossEntropy2d(thresh=fx["args"]["thresh"], min_kept=fx["args"]["min_kept"])
    loss = crit(x, torch.from_numpy(fx["target"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert np.float32(r["threshold"]).tobytes() == np.float32(crit.last_threshold.item()).tobytes()
    mask = (x.grad != 0).any(dim=1).cpu().numpy()
    assert np.array_equal(r["kept_mask"], mask) and r["kept"] == int(crit.last_kept.item())
    assert abs(float(r["head_loss"][0]) - float(loss.detach())) <= D.LOSS_RTOL * abs(float(loss.detach()))


def test_tie_group_at_the_kth_key_is_kept_whole_at_full_resolution():
    """the inputs of tests/test_emu_ohemdsn.py's tie test: low-resolution logits constant over 2 x 2 squares and rounded to
    multiples of 1/8, so that at the exact ratio 8 the full-resolution pixels of a square share one target probability bit
    for bit"""
    from ccnet_amd import _ohemdsn_lib
    B, C, h, w, H, W = 1, 19, 13, 13, 97, 97
    low, _ = O.make_tie_inputs(B, C, h, w, seed=2, block=2)
    low = (np.round(low * 8) / 8).astype(np.float32)
    rng = np.random.default_rng(3)
    logits = [low, (rng.standard_normal(low.shape) * 3).astype(np.float32)]
    up = D.upsample(low, (H, W)).numpy()
    target = up.argmax(1).astype(np.int64)
    rand = rng.integers(0, C, target.shape)
    pick = rng.random(target.shape) < 0.5
    target[pick] = rand[pick]
    target[rng.random(target.shape) < 0.03] = 255
    groups = [g for g in O.tie_groups(up, target, factor=8, thresh=0.0) if g[2] >= 3][:3]
    assert groups
    for value, below, size in groups:
        args = dict(thresh=0.0, min_kept=(below + (size + 1) // 2) * 64)
        r = D.run_raw(_ohemdsn_lib.get_lib(), DeviceMemory(), logits, target, **args)
        sel = D.select(low, target, **args)
        assert sel["threshold"] == value
        D.check_against_oracle("tie", logits, target, args, r)
        group = sel["valid"] & (sel["target_prob"] == value)
        assert group.sum() >= size and r["kept_mask"][group].all(), (value, int(r["kept_mask"][group].sum()), int(group.sum()))


def test_two_runs_are_bit_identical():
    fx = D.load_fixture("recipe")
    a, _, l1, g1 = run_module(fx["logits"], fx["target"], **fx["args"])
    b, _, l2, g2 = run_module(fx["logits"], fx["target"], **fx["args"])
    assert torch.equal(l1, l2) and all(torch.equal(x, y) for x, y in zip(g1, g2))
    assert a["threshold"] == b["threshold"] and np.array_equal(a["kept_mask"], b["kept_mask"])


def test_graph_replay_equals_eager_bitwise():
    """torch's capture recipe as tests/test_gpu_dsn.py follows it: every eager run that touches the captured tensors is on the
    one side stream that also captures, so the graph is a chain without parallel branches"""
    from ccnet_amd import ohemdsn
    fx = D.load_fixture("kth")
    crit = ohemdsn.CriterionOhemDSN(**fx["args"])
    _, _, eager_loss, eager_grads = run_module(fx["logits"], fx["target"], **fx["args"])
    eager = [eager_loss] + eager_grads
    xs, t = to_dev(fx["logits"], fx["target"])
    torch.cuda.synchronize()

    def step():
        loss = crit(xs, t)
        return [loss.detach()] + list(torch.autograd.grad(loss, xs))

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
    assert int(crit.last_kept.item()) == int(fx["kept_mask"].sum())


def test_bf16_logits_under_autocast_give_fp32_loss_and_bf16_gradients():
    fx = D.load_fixture("kth")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, _, loss, grads = run_module(fx["logits"], fx["target"], dtype=torch.bfloat16, **fx["args"])
    rounded = [torch.from_numpy(l).to(torch.bfloat16).float().numpy() for l in fx["logits"]]
    _, _, loss32, grads32 = run_module(rounded, fx["target"], **fx["args"])      # the fp32 path on the same rounded logits
    assert loss.dtype == torch.float32 and torch.equal(loss, loss32)
    for g, g32 in zip(grads, grads32):
        assert g.dtype == torch.bfloat16 and g.shape == g32.shape
        # one bf16 rounding (8 significand bits, round to nearest: half an ulp is 2^-9 relative) of the fp32 gradient
        assert bool(((g.float() - g32).abs() <= 2.0 ** -8 * g32.abs() + 1e-30).all())


def test_peak_memory_at_the_recipe_stays_below_half_a_full_resolution_logits_tensor():
    """the workspace cap is 16 of the 76 bytes a pixel that one (B, 19, H, W) fp32 tensor takes"""
    from ccnet_amd import ohemdsn
    fx = D.load_fixture("recipe")
    B, C, h, w, H, W = (int(v) for v in fx["shape"])
    xs, t = to_dev(fx["logits"], fx["target"])
    crit = ohemdsn.CriterionOhemDSN(**fx["args"])
    loss = crit(xs, t)                                   # (a first call: the library is loaded, the allocator warm)
    loss.backward()
    for x in xs:
        x.grad = None
    del loss
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = crit(xs, t)
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    full = B * C * H * W * 4
    print(f"peak growth during forward + backward: {growth / 2 ** 20:.1f} MiB; one full-resolution logits tensor: "
          f"{full / 2 ** 20:.1f} MiB")
    assert growth < full / 2


@pytest.fixture(scope="module")
def seg_model_steps():
    """One training step of Seg_Model(19) on a 65 x 65 crop, on the same weights, input and dropout masks (reseeded), with
    ohem.CriterionOhemDSN() (stock up-samples), with the fused criterion, and with the stock one again; deterministic
    convolutions, as tests/test_gpu_dsn.py explains.  min_kept 64 * 20 of the 2 x 8 x 8 zoomed keys puts the k-th key to
    work.  Per run: loss, kept count, threshold and the first convolution's gradient."""
    from ccnet_amd import ohem, ohemdsn
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 65, 65, generator=g).to(DEV)
    labels = torch.randint(0, 19, (2, 65, 65), generator=g)
    labels[torch.rand(2, 65, 65, generator=g) < 0.1] = 255
    labels = labels.to(DEV)
    args = dict(thresh=0.05, min_kept=64 * 20)
    res = {}
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for name, crit in (("stock", ohem.CriterionOhemDSN(**args)), ("fused", ohemdsn.CriterionOhemDSN(**args)),
                           ("stock again", ohem.CriterionOhemDSN(**args))):
            model.criterion = crit
            model.zero_grad(set_to_none=True)
            torch.manual_seed(7)                              # the same Dropout2d masks in every run
            loss = model(x, labels)
            loss.backward()
            torch.cuda.synchronize()
            head = crit if name == "fused" else crit.criterion1
            res[name] = (float(loss.detach()), int(head.last_kept.item()), float(head.last_threshold.item()),
                         model.conv1.weight.grad.double().cpu().numpy().copy())
    finally:
        torch.backends.cudnn.deterministic = keep
    l0, k0, t0, g0 = res["stock"]
    for name in ("fused", "stock again"):
        l, k, t, gr = res[name]
        print(f"{name}: loss {l!r} (stock {l0!r}); kept {k} (stock {k0}); threshold {t!r} (stock {t0!r}); conv1 gradient max "
              f"error {np.abs(gr - g0).max():.3g} of max|grad| {np.abs(g0).max():.3g}")
    return res


def test_seg_model_training_step_repeats_itself_with_the_stock_criterion(seg_model_steps):
    """the reference of the test below is a reference only if it reproduces itself"""
    a, b = seg_model_steps["stock"], seg_model_steps["stock again"]
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3])


def test_seg_model_training_step_matches_the_stock_ohem_criterion(seg_model_steps):
    """Same kept count, loss within 1e-5 relative, conv1.weight.grad within 1e-5 of its maximum.  The seed is one at which
    the two criteria keep the same pixels (equal counts are asserted, not arranged: no comparison on equalised masks)."""
    (l0, k0, t0, g0), (l1, k1, t1, g1) = seg_model_steps["stock"], seg_model_steps["fused"]
    assert k1 == k0 and 0 < k0 and abs(t1 - t0) <= D.NEAR
    assert math.isfinite(l0) and abs(l1 - l0) <= D.LOSS_RTOL * abs(l0)
    assert np.abs(g0).max() > 0 and np.abs(g1 - g0).max() <= D.GRAD_RTOL * np.abs(g0).max()
