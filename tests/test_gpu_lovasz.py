"""Lovász-softmax on the MI355X (libccnet_lovasz.so through ccnet_amd.lovasz) against the reference fixtures and the numpy
oracle: loss and tie-aware gradient; per_image and the class modes; the CriterionOhemDSN2 composition; no host sync;
bitwise repeatability; bf16 probabilities; the --lovasz train driver."""
import glob
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lovasz_oracle as O
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "lovasz_[0-9]*.npz")))
CRITERION_FIXTURE = os.path.join(GOLDEN, "lovasz_criterion_1x19x97x97_769.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run_device(probas, labels, grad_out=1.0, **args):
    from ccnet_amd.lovasz import LovaszSoftmax
    m = LovaszSoftmax(**args)
    x = torch.from_numpy(probas).to(DEV).requires_grad_(True) if isinstance(probas, np.ndarray) else probas
    t = torch.from_numpy(labels).to(DEV) if isinstance(labels, np.ndarray) else labels
    loss = m(x, t)
    loss.backward(torch.tensor(grad_out, device=DEV))
    torch.cuda.synchronize()
    return m, loss.detach(), x.grad


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_parity(path):
    fx = O.load_fixture(path)
    _, loss, grad = run_device(fx["probas"], fx["labels"], **fx["args"])
    singles, groups = O.check_against_fixture(fx, float(loss.item()), grad.cpu().numpy(), rtol=1e-5, gtol=1e-5)
    print(f"{os.path.basename(path)}: singletons {singles}, equal-error groups {groups}")


@pytest.mark.parametrize("args", [dict(ignore=255), dict(per_image=True, ignore=255), dict(classes="all", ignore=255),
                                  dict(classes=[0, 3, 3, 18], per_image=True, ignore=255), dict(ignore=None)],
                         ids=["present", "per_image", "all", "list_per_image", "ignore_none"])
def test_device_matches_oracle(args):
    probas, labels = O.make_case_inputs(2, 19, 129, 257, seed=31, extra_frac=0.02, absent=18)
    m, loss, grad = run_device(probas, labels, **args)
    o = O.lovasz_softmax(probas, labels, **args)
    assert int(m.last_n_kept.item()) == o["n_kept"]
    assert abs(float(loss) - o["loss"]) <= 1e-6 * abs(o["loss"])
    assert int(O.ulp_distance(grad.cpu().numpy(), o["grad"]).max()) <= 2


def test_no_valid_pixel_gives_zero_loss_and_gradient():
    probas, labels = O.make_case_inputs(2, 19, 65, 65, seed=37)
    labels[:] = 255
    m, loss, grad = run_device(probas, labels, ignore=255)
    assert float(loss) == 0.0 and int(m.last_n_kept.item()) == 0 and not grad.any()


def _check(n_kept, loss, grad, o):
    """The bar of test_device_matches_oracle: n_kept exact, loss within 1e-6 relative, gradient within 2 ulp (+0 and -0
    count as equal).  Returns the largest ulp distance."""
    assert int(n_kept.item()) == o["n_kept"]
    assert abs(float(loss) - o["loss"]) <= 1e-6 * abs(o["loss"]) or float(loss) == o["loss"] == 0, (float(loss), o["loss"])
    g = grad.cpu().numpy() if isinstance(grad, torch.Tensor) else grad
    ulp = O.ulp_distance(g + np.float32(0), o["grad"] + np.float32(0))             # x + 0 turns -0 into +0
    worst = int(ulp.max())
    assert worst <= 2, worst
    return worst


def _run_checked(probas, labels, **args):
    m, loss, grad = run_device(probas, labels, **args)
    o = O.lovasz_softmax(probas, labels, **args)
    worst = _check(m.last_n_kept, loss, grad, o)
    print(f"{tuple(probas.shape)} {args}: loss {float(loss)!r} (oracle {o['loss']!r}), n_kept {o['n_kept']}, "
          f"worst gradient distance {worst} ulp")
    return m, loss, grad.cpu().numpy(), o


def test_all_equal_probabilities_give_the_oracle_gradient_bitwise():
    """One tie group per class: the sorted order is pixel order across 33 tiles and every wave of the scatter."""
    probas = np.full((2, 19, 129, 257), np.float32(1 / 19), np.float32)
    labels = np.random.default_rng(51).integers(0, 19, (2, 129, 257)).astype(np.int64)
    labels[np.random.default_rng(52).random(labels.shape) < 0.05] = 255
    _, _, g, o = _run_checked(probas, labels, ignore=255)
    assert np.array_equal(g.view(np.uint32), o["grad"].view(np.uint32))


def test_one_valid_pixel():
    probas, labels = O.make_case_inputs(2, 19, 65, 97, seed=53)
    labels[:] = 255
    labels[1, 40, 61] = 7
    _, _, g, o = _run_checked(probas, labels, ignore=255)
    assert o["n_kept"] == 1 and np.count_nonzero(g) == 1 and g[1, 7, 40, 61] != 0


def test_per_image_with_a_fully_ignored_image():
    probas, labels = O.make_case_inputs(3, 19, 97, 129, seed=55)
    labels[1] = 255
    _, _, g, o = _run_checked(probas, labels, per_image=True, ignore=255)
    assert not g[1].any() and g[0].any() and g[2].any()


@pytest.mark.parametrize("per_image", [False, True], ids=["plain", "per_image"])
def test_gradient_scales_exactly_with_grad_out(per_image):
    probas, labels = O.make_case_inputs(2, 19, 97, 129, seed=57)
    _, l1, g1 = run_device(probas, labels, per_image=per_image, ignore=255)
    _, l2, g2 = run_device(probas, labels, grad_out=0.5, per_image=per_image, ignore=255)
    assert torch.equal(l1, l2) and torch.equal(g2, 0.5 * g1)


def test_exact_zero_negative_zero_and_one_probabilities():
    """Where e = |fg - p| = 0 the sign of d e / d p is 0, so the gradient is exactly 0."""
    probas, labels = O.make_case_inputs(2, 19, 97, 129, seed=59)
    rng = np.random.default_rng(60)
    pick = rng.random(probas.shape)
    probas[pick < 0.1] = 0.0
    probas[(pick >= 0.1) & (pick < 0.2)] = -0.0
    fg = labels[:, None] == np.arange(19)[None, :, None, None]
    probas[fg & (pick >= 0.2) & (pick < 0.6)] = 1.0
    _, _, g, o = _run_checked(probas, labels, ignore=255)
    zero_e = (np.abs(fg.astype(np.float32) - probas) == 0) & (labels != 255)[:, None]
    assert zero_e.sum() > 10000 and not g[zero_e].any()


@pytest.mark.parametrize("C,ignore", [(2, 255), (256, None)], ids=["c2", "c256_all_labels"])
@pytest.mark.parametrize("per_image", [False, True], ids=["plain", "per_image"])
def test_class_count_limits(C, ignore, per_image):
    """C = 2 and C = 256 (labels 0..255, none ignored; per_image: finalize takes 512 segments on 256 threads)."""
    H, W = (129, 257) if C == 2 else (48, 80)
    probas, labels = O.make_case_inputs(2, C, H, W, seed=61 + C)
    if C == 256:
        assert labels.min() == 0 and labels.max() == 255
    _run_checked(probas, labels, per_image=per_image, ignore=ignore)


_SCALE = {}


def _scale_inputs():
    if not _SCALE:
        _SCALE["x"] = O.make_case_inputs(8, 19, 769, 769, seed=63)
    return _SCALE["x"]


@pytest.mark.parametrize("per_image", [False, True], ids=["plain", "per_image"])
def test_scale_batch8_769(per_image):
    """(8, 19, 769, 769): 2 310 sort tiles per plain segment, whose payload index crosses image boundaries."""
    probas, labels = _scale_inputs()
    _run_checked(probas, labels, per_image=per_image, ignore=255)


@pytest.mark.parametrize("shape", [(1, 2, 4096, 4096), (4, 3, 2048, 2048)], ids=["1x2x4096x4096", "4x3x2048x2048"])
def test_segment_of_exactly_2_24_pixels(shape):
    """The limit: 2^24 pixels in one segment (the 24-bit payload index, fp32-exact counts); the second spans four images."""
    B, C, H, W = shape
    assert B * H * W == 1 << 24
    probas, labels = O.make_case_inputs(B, C, H, W, seed=67 + B)
    _run_checked(probas, labels, ignore=255)


def test_two_calls_summed_before_one_backward():
    """Two losses, each with its own workspace, one backward: every input gets its own oracle gradient."""
    from ccnet_amd.lovasz import lovasz_softmax
    p1, t1 = O.make_case_inputs(2, 19, 97, 129, seed=71)
    p2, t2 = O.make_case_inputs(1, 11, 65, 257, seed=72)
    x1 = torch.from_numpy(p1).to(DEV).requires_grad_(True)
    x2 = torch.from_numpy(p2).to(DEV).requires_grad_(True)
    s1, s2 = {}, {}
    l1 = lovasz_softmax(x1, torch.from_numpy(t1).to(DEV), ignore=255, stats=s1)
    l2 = lovasz_softmax(x2, torch.from_numpy(t2).to(DEV), classes="all", per_image=True, ignore=255, stats=s2)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    for x, stats, loss, p, t, args in ((x1, s1, l1, p1, t1, dict(ignore=255)),
                                       (x2, s2, l2, p2, t2, dict(classes="all", per_image=True, ignore=255))):
        _check(stats["n_kept"], loss.detach(), x.grad, O.lovasz_softmax(p, t, **args))


def test_criterion_against_reference_fixture_and_oracle_composition():
    from ccnet_amd.segmodel import CriterionOhemDSN2
    z = np.load(CRITERION_FIXTURE)
    main, aux, target = O.make_criterion_inputs(int(z["seed"]))
    xm = torch.from_numpy(main).to(DEV).requires_grad_(True)
    xa = torch.from_numpy(aux).to(DEV).requires_grad_(True)
    loss = CriterionOhemDSN2(ignore_index=255)([xm, xa], torch.from_numpy(target).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    assert xa.grad is None
    assert abs(float(loss) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    g = xm.grad.cpu().numpy()
    assert np.abs(g.ravel()[z["grad_index"]] - z["grad_sample"]).max() <= 1e-4 * float(z["grad_absmax"])

    # CPU composition of stock ops with the oracle (the same stable tie order as the device)
    x = torch.from_numpy(main).requires_grad_(True)
    up = F.interpolate(x, size=(769, 769), mode="bilinear", align_corners=True)
    t = torch.from_numpy(target)
    ce = F.cross_entropy(up, t, ignore_index=255)
    prob = F.softmax(up, dim=1)
    o = O.lovasz_softmax(prob.detach().numpy(), target, ignore=255)
    (ce + (prob * torch.from_numpy(o["grad"])).sum()).backward()
    ref = float(ce.detach()) + o["loss"]
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    assert (xm.grad.cpu() - x.grad).abs().max().item() <= 1e-4 * x.grad.abs().max().item()


def test_no_host_sync_in_forward_and_backward():
    from ccnet_amd.lovasz import lovasz_softmax
    probas, labels = O.make_case_inputs(2, 19, 97, 97, seed=41)
    x = torch.from_numpy(probas).to(DEV).requires_grad_(True)
    t = torch.from_numpy(labels).to(DEV)
    for args in (dict(ignore=255), dict(classes=[1, 2, 2], per_image=True, ignore=255)):
        lovasz_softmax(x, t, **args).backward()                  # warm: library load, allocator
        torch.cuda.synchronize()
        x.grad = None
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = lovasz_softmax(x, t, **args)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item()) and x.grad is not None


def test_bitwise_repeatable():
    probas, labels = O.make_case_inputs(2, 19, 257, 257, seed=43)
    probas[..., ::2] = np.round(probas[..., ::2] * 256) / 256             # plenty of equal errors
    _, l1, g1 = run_device(probas, labels, ignore=255)
    _, l2, g2 = run_device(probas, labels, ignore=255)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_bf16_probas_give_fp32_loss_and_bf16_gradient():
    probas, labels = O.make_case_inputs(1, 19, 97, 97, seed=47)
    x = torch.from_numpy(probas).to(DEV).to(torch.bfloat16).requires_grad_(True)
    _, loss, grad = run_device(x, labels, ignore=255)
    assert loss.dtype == torch.float32 and grad.dtype == torch.bfloat16
    o = O.lovasz_softmax(x.detach().float().cpu().numpy(), labels, ignore=255)
    assert abs(float(loss) - o["loss"]) <= 1e-5 * abs(o["loss"])
    assert np.abs(grad.float().cpu().numpy() - o["grad"]).max() <= 1e-2 * np.abs(o["grad"]).max()


@pytest.mark.parametrize("extra", [[], ["--force-ddp"]], ids=["plain", "ddp"])
def test_train_synthetic_lovasz_child_process(extra):
    cmd = [sys.executable, "-m", "ccnet_amd.train_synthetic", "--lovasz", "--steps", "2", "--warmup", "1", "--size", "257"]
    env = dict(os.environ)
    if extra:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["criterion"] == "lovasz" and math.isfinite(res["final_loss"]), res
