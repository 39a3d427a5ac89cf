"""OHEM cross-entropy on the MI355X (libccnet_ohem.so through ccnet_amd.ohem) against the reference fixtures and the
numpy oracle: threshold, kept mask, loss, gradient; the DSN criterion; no host sync; bitwise repeatability; bf16 logits;
the --ohem train driver."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ohem_oracle as O
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ohem_*.npz")))
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run_device(logits, target, grad_out=1.0, **args):
    from ccnet_amd.ohem import OhemCrossEntropy2d
    m = OhemCrossEntropy2d(**args)
    x = torch.from_numpy(logits).to(DEV).requires_grad_(True) if isinstance(logits, np.ndarray) else logits
    t = torch.from_numpy(target).to(DEV) if isinstance(target, np.ndarray) else target
    loss = m(x, t)
    loss.backward(torch.tensor(grad_out, device=DEV))
    torch.cuda.synchronize()
    return m, loss.detach(), x.grad


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_parity(path):
    fx = O.load_fixture(path)
    m, loss, grad = run_device(fx["logits"], fx["target"], **fx["args"])
    g = grad.cpu().numpy()
    mask = (g != 0).any(axis=1)
    assert int(m.last_kept.item()) == int(mask.sum())
    assert int(m.last_num_valid.item()) == O.ohem(fx["logits"], fx["target"], **fx["args"])["num_valid"]
    n_diff = O.check_against_fixture(fx, m.last_threshold.item(), mask, float(loss.item()), g)
    print(f"{os.path.basename(path)}: kept-mask pixels differing near the threshold: {n_diff}")


def test_dsn_criterion_against_oracle_composition():
    from ccnet_amd.segmodel import CriterionOhemDSN
    rng = np.random.default_rng(21)
    main = (rng.standard_normal((1, 19, 97, 97)) * 3).astype(np.float32)
    aux = (rng.standard_normal((1, 19, 97, 97)) * 3).astype(np.float32)
    target = rng.integers(0, 19, (1, 769, 769)).astype(np.int64)
    target[rng.random((1, 769, 769)) < 0.05] = 255
    crit = CriterionOhemDSN(thresh=0.6, min_kept=200000)
    xm = torch.from_numpy(main).to(DEV).requires_grad_(True)
    xa = torch.from_numpy(aux).to(DEV).requires_grad_(True)
    loss = crit([xm, xa], torch.from_numpy(target).to(DEV))
    loss.backward()
    torch.cuda.synchronize()

    # oracle composition on the CPU: stock up-sampling, numpy OHEM on the main branch, stock CE on the aux branch
    cm = torch.from_numpy(main).requires_grad_(True)
    ca = torch.from_numpy(aux).requires_grad_(True)
    up = F.interpolate(cm, size=(769, 769), mode="bilinear", align_corners=True)
    o = O.ohem(up.detach().numpy(), target, thresh=0.6, min_kept=200000)
    up.backward(torch.from_numpy(o["grad"]))
    loss2 = F.cross_entropy(F.interpolate(ca, size=(769, 769), mode="bilinear", align_corners=True),
                            torch.from_numpy(target), ignore_index=255)
    (0.4 * loss2).backward()
    ref = o["loss"] + 0.4 * float(loss2.detach())
    assert abs(int(crit.criterion1.last_kept.item()) - o["kept"]) <= 16
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref) * (1 + abs(int(crit.criterion1.last_kept.item()) - o["kept"])), (float(loss), ref)
    for dev_g, ref_g in ((xm.grad, cm.grad), (xa.grad, ca.grad)):
        err = (dev_g.cpu() - ref_g).abs().max().item()
        assert err <= 1e-4 * ref_g.abs().max().item(), err


def test_no_host_sync_in_forward_and_backward():
    logits, target = O.make_case_inputs(2, 19, 97, 97, seed=5)
    from ccnet_amd.ohem import OhemCrossEntropy2d
    m = OhemCrossEntropy2d(thresh=0.7, min_kept=6400)
    x = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    t = torch.from_numpy(target).to(DEV)
    m(x, t).backward()                                   # warm: library load, allocator
    torch.cuda.synchronize()
    x.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = m(x, t)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert math.isfinite(loss.item()) and x.grad is not None


def test_bitwise_repeatable():
    logits, target = O.make_case_inputs(2, 19, 257, 257, seed=9)
    _, l1, g1 = run_device(logits, target, thresh=0.7, min_kept=20000)
    _, l2, g2 = run_device(logits, target, thresh=0.7, min_kept=20000)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_bf16_logits_give_fp32_loss_and_bf16_gradient():
    logits, target = O.make_case_inputs(1, 19, 97, 97, seed=13)
    x = torch.from_numpy(logits).to(DEV).to(torch.bfloat16).requires_grad_(True)
    m, loss, grad = run_device(x, target, thresh=0.7, min_kept=6400)
    assert loss.dtype == torch.float32 and grad.dtype == torch.bfloat16
    o = O.ohem(x.detach().float().cpu().numpy(), target, thresh=0.7, min_kept=6400)
    assert abs(float(loss) - o["loss"]) <= 1e-4 * abs(o["loss"])
    assert (grad.float().cpu().numpy() - o["grad"]).__abs__().max() <= 1e-2 * np.abs(o["grad"]).max()


def _run_checked(logits, target, grad_out=1.0, **args):
    """One device forward + backward checked against the oracle (O.check_result); returns (module, loss, grad, oracle)."""
    m, loss, grad = run_device(logits, target, grad_out=grad_out, **args)
    g = grad.cpu().numpy()
    mask = (g != 0).any(axis=1)
    assert int(m.last_kept.item()) == int(mask.sum())
    o, n_diff = O.check_result(logits, target, args, m.last_threshold.item(), mask, float(loss.item()), g)
    assert int(m.last_num_valid.item()) == o["num_valid"]
    print(f"{tuple(logits.shape)}: threshold {m.last_threshold.item()!r} (oracle {float(o['threshold'])!r}), kept "
          f"{int(mask.sum())}, mask pixels differing near the threshold {n_diff}")
    return m, loss, g, o


@pytest.mark.parametrize("case", O.EDGE_CASES, ids=O.EDGE_IDS)
def test_edge_cases_match_oracle(case):
    logits, target, args = O.edge_case_inputs(case)
    _run_checked(logits, target, **args)


def test_all_ignored_gives_nan_loss_zero_gradient_and_threshold_one():
    logits, target = O.make_case_inputs(2, 19, 40, 56, seed=3, all_ignored=True)
    m, loss, grad = run_device(logits, target, thresh=0.7, min_kept=0, factor=4)
    assert math.isnan(float(loss)) and float(m.last_threshold.item()) == 1.0
    assert int(m.last_kept.item()) == 0 and int(m.last_num_valid.item()) == 0 and not grad.any()


def test_gradient_scales_exactly_with_grad_out():
    logits, target = O.make_case_inputs(2, 19, 97, 129, seed=11)
    _, l1, g1 = run_device(logits, target, thresh=0.7, min_kept=20000)
    _, l2, g2 = run_device(logits, target, grad_out=0.5, thresh=0.7, min_kept=20000)
    assert torch.equal(l1, l2) and torch.equal(g2, 0.5 * g1)


@pytest.mark.parametrize("seed", [1, 2, 4, 6])
def test_tie_group_at_the_kth_key_is_kept_whole(seed):
    """Logits from a few per-pixel vectors: large groups of equal zoomed keys.  The k-th key is the last of its group, so
    one rank more would select the next larger value; the group itself must be kept whole at full resolution."""
    logits, target = O.make_tie_inputs(2, 19, 128, 192, seed=seed)
    groups = [g for g in O.tie_groups(logits, target, factor=4, thresh=0.002) if g[2] >= 4][:6]
    assert groups
    for value, below, size in groups:
        args = dict(thresh=0.002, min_kept=(below + size) * 16, factor=4)
        m, _, g, o = _run_checked(logits, target, **args)
        assert o["threshold"] == value
        group = o["valid"] & (o["target_prob"] == value)
        assert group.sum() >= size and (g != 0).any(axis=1)[group].all(), (float(value), size)


@pytest.mark.parametrize("shape,args", [
    ((8, 19, 769, 769), dict(thresh=0.6, min_kept=200000, factor=8)),       # the training driver's --ohem recipe
    ((2, 150, 257, 385), dict(thresh=0.7, min_kept=50000, factor=8)),       # ADE20K's class count
], ids=["recipe_b8", "c150"])
def test_scale_matches_oracle(shape, args):
    logits, target = O.make_case_inputs(*shape, seed=sum(shape))
    _run_checked(logits, target, **args)


def test_train_synthetic_ohem_child_process():
    cmd = [sys.executable, "-m", "ccnet_amd.train_synthetic", "--ohem", "--steps", "2", "--warmup", "1", "--size", "257"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["criterion"] == "ohem" and math.isfinite(res["final_loss"]), res
