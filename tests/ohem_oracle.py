"""numpy restatement of the reference OHEM cross-entropy (loss/loss.py:9-93, ``OhemCrossEntropy2d``).

The probabilities come from torch's softmax, as in the reference; the rest is numpy.  No scipy: ``scipy.ndimage.zoom(order=0 | 1, prefilter=False, grid_mode=False)`` is restated by :func:`zoom_coords`,
:func:`zoom_order0` and :func:`zoom_order1` (tests/test_ohem_host.py checks them against scipy where it is installed), so
the oracle runs where the fixtures are consumed.  Everything here is test infrastructure.
"""
import numpy as np


def zoom_out_size(n, factor):
    """scipy's output length: round(n / factor), ties to even (Python's round)."""
    return int(round(n * (1.0 / factor)))


def zoom_coords(n, factor):
    """Source coordinate of every output sample along one axis, in double: o * (n - 1) / (n_out - 1)."""
    n_out = zoom_out_size(n, factor)
    z = (n - 1) / (n_out - 1) if n_out > 1 else 1.0
    return np.arange(n_out, dtype=np.float64) * z


def zoom_order0(a, factor):
    """Nearest-sample zoom of the last two axes (labels)."""
    cy, cx = zoom_coords(a.shape[-2], factor), zoom_coords(a.shape[-1], factor)
    iy = np.minimum(np.floor(cy + 0.5).astype(np.int64), a.shape[-2] - 1)
    ix = np.minimum(np.floor(cx + 0.5).astype(np.int64), a.shape[-1] - 1)
    return a[..., iy[:, None], ix[None, :]]


def _linear_taps(c, n):
    i0 = np.floor(c).astype(np.int64)
    t = c - i0
    return i0, np.minimum(i0 + 1, n - 1), 1.0 - t, t


def zoom_order1(a, factor):
    """Linear zoom of the last two axes, accumulated in double in scipy's tap order and rounded to a.dtype."""
    H, W = a.shape[-2:]
    y0, y1, wy0, wy1 = _linear_taps(zoom_coords(H, factor), H)
    x0, x1, wx0, wx1 = _linear_taps(zoom_coords(W, factor), W)
    d = a.astype(np.float64)
    acc = np.zeros(a.shape[:-2] + (len(y0), len(x0)), np.float64)
    for yi, wy in ((y0, wy0), (y1, wy1)):
        for xi, wx in ((x0, wx0), (x1, wx1)):
            acc += d[..., yi[:, None], xi[None, :]] * wy[:, None] * wx[None, :]
    return acc.astype(a.dtype)


def softmax_f32(logits):
    """The reference's own softmax (loss.py:90, F.softmax on fp32): the probabilities OHEM zooms and thresholds."""
    import torch
    return torch.softmax(torch.from_numpy(np.ascontiguousarray(logits, np.float32)), 1).numpy()


def find_threshold(prob, target, ignore_label=255, thresh=0.7, min_kept=100000, factor=8):
    """loss.py:20-48 on the zoomed grid.  Returns (fp32 threshold, num_valid on the zoomed grid)."""
    p = zoom_order1(prob, factor)
    t = zoom_order0(target, factor).astype(np.int32)
    kept_min = min_kept // (factor * factor)
    valid = t != ignore_label
    num_valid = int(valid.sum())
    if kept_min >= num_valid:
        return np.float32(1.0), num_valid
    threshold = np.float32(thresh)
    if kept_min > 0:
        lab = t[valid]
        pv = np.moveaxis(p, 1, -1)[valid]                       # (num_valid, C)
        pred = pv[np.arange(len(lab)), lab]
        kth = np.partition(pred, kept_min - 1)[kept_min - 1]
        threshold = max(threshold, np.float32(kth))
    return np.float32(threshold), num_valid


def target_prob(prob, target, ignore_label=255):
    """Softmax probability of every pixel's own label (0 where the label is ignored)."""
    valid = target != ignore_label
    lab = np.where(valid, target, 0)
    return np.take_along_axis(prob, lab[:, None], axis=1)[:, 0], valid


def ohem(logits, target, ignore_label=255, thresh=0.7, min_kept=100000, factor=8, prob=None):
    """The whole reference criterion on numpy arrays: logits (B,C,H,W) fp32, target (B,H,W) int.

    Returns a dict: threshold (fp32), num_valid (zoomed), new_target (int64), kept count, loss (float64; NaN when nothing is
    kept, as F.cross_entropy) and grad (d loss / d logits, fp32, for an upstream gradient of 1)."""
    prob = softmax_f32(logits) if prob is None else prob
    threshold, num_valid = find_threshold(prob, target, ignore_label, thresh, min_kept, factor)
    pt, valid = target_prob(prob, target, ignore_label)
    kept = valid & (pt <= threshold)
    new_target = np.where(kept, target, ignore_label).astype(np.int64)
    n = int(kept.sum())
    x = logits.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    lab = np.where(kept, target, 0)
    xt = np.take_along_axis(x, lab[:, None], axis=1)[:, 0]
    loss = float(((lse - xt) * kept).sum() / n) if n else float("nan")
    sm = np.exp(x - lse[:, None])
    onehot = np.zeros_like(sm)
    np.put_along_axis(onehot, lab[:, None], 1.0, axis=1)
    grad = ((sm - onehot) * kept[:, None] / max(n, 1)).astype(np.float32)
    return {"threshold": threshold, "num_valid": num_valid, "new_target": new_target, "kept": n, "loss": loss,
            "grad": grad, "target_prob": pt, "valid": valid}


def make_case_inputs(B, C, H, W, seed, scale=3.0, ignore_frac=0.05, all_ignored=False):
    """Seeded logits and labels of one fixture case (tests/golden/make_ohem_golden.py regenerates them the same way)."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C, H, W)) * scale).astype(np.float32)
    target = rng.integers(0, C, (B, H, W)).astype(np.int64)
    target[rng.random((B, H, W)) < ignore_frac] = 255
    if all_ignored:
        target[:] = 255
    return logits, target


# small cases at the edges of the select (tests/test_ohem_host.py runs them in the emulator, tests/test_gpu_ohem.py on the
# device): C = 19; ``min_kept`` and ``factor`` pick the branch of find_threshold
EDGE_CASES = [
    dict(B=1, H=24, W=40, thresh=0.7, min_kept=0, factor=4),                 # min_kept' == 0: thresh alone
    dict(B=2, H=17, W=33, thresh=0.002, min_kept=16 * 40, factor=4),         # k-th above a low thresh
    dict(B=1, H=9, W=9, thresh=0.7, min_kept=10 ** 6, factor=8),             # one zoomed pixel: threshold 1.0
    dict(B=1, H=3, W=30, thresh=0.7, min_kept=100, factor=8),                # zoomed height 0: no keys at all
    dict(B=1, H=20, W=20, thresh=0.002, min_kept=16 * 20, factor=4, ignore_label=7),   # another ignore label, k-th above
]
EDGE_IDS = ["minkept0", "kth_above", "one_zoomed_pixel", "zoomed_height0", "ignore7"]


def edge_case_inputs(case):
    """(logits, target, criterion args) of one EDGE_CASES entry."""
    case = dict(case)
    B, H, W = case.pop("B"), case.pop("H"), case.pop("W")
    logits, target = make_case_inputs(B, 19, H, W, seed=H * W + B)
    if case.get("ignore_label") == 7:
        target[target == 255] = 3
    return logits, target, case


def make_tie_inputs(B, C, H, W, seed, n_vectors=12, block=16):
    """Logits made of ``n_vectors`` distinct per-pixel vectors, each with its own label, constant over ``block`` x ``block``
    squares: every zoomed sample whose taps lie inside one square repeats its vector's target probability exactly, so the
    zoomed keys form a few large groups of equal values.  About 3 % of the pixels are ignored."""
    rng = np.random.default_rng(seed)
    vec = (rng.standard_normal((n_vectors, C)) * 3).astype(np.float32)
    lab = rng.integers(0, C, n_vectors)
    which = rng.integers(0, n_vectors, (B, -(-H // block), -(-W // block)))
    which = np.repeat(np.repeat(which, block, axis=1), block, axis=2)[:, :H, :W]
    logits = np.ascontiguousarray(vec[which].transpose(0, 3, 1, 2))
    target = lab[which].astype(np.int64)
    target[rng.random((B, H, W)) < 0.03] = 255
    return logits, target


def tie_groups(logits, target, ignore_label=255, factor=8, thresh=0.0):
    """The groups of equal zoomed keys above ``thresh`` but the largest key, largest group first: a list of (value, keys
    below it, group size)."""
    p = zoom_order1(softmax_f32(logits), factor)
    t = zoom_order0(target, factor).astype(np.int64)
    valid = t != ignore_label
    pred = np.take_along_axis(p, np.where(valid, t, 0)[:, None], axis=1)[:, 0][valid]
    vals, counts = np.unique(pred, return_counts=True)
    below = np.concatenate([[0], np.cumsum(counts)[:-1]])
    keep = (vals > thresh) & (below + counts < len(pred))
    order = np.argsort(-counts[keep], kind="stable")
    return [(np.float32(v), int(b), int(n)) for v, b, n in zip(vals[keep][order], below[keep][order], counts[keep][order])]


def check_result(logits, target, args, threshold, kept_mask, loss, grad, near=1e-6, rtol=1e-5, gtol=1e-5):
    """The numerics bar of a device result against :func:`ohem` on the same inputs: threshold within 2 fp32 ulp; the kept
    mask identical except at pixels whose target probability lies within ``near`` of the threshold (the device's expf is
    not the oracle's exp); loss within ``rtol`` relative and the gradient within ``gtol`` x max|grad| of the oracle on the
    device's own mask.  Returns (oracle result, number of differing pixels)."""
    ignore = args.get("ignore_label", 255)
    o = ohem(logits, target, **args)
    assert ulp_distance(threshold, o["threshold"]) <= 2, (float(threshold), float(o["threshold"]))
    diff = kept_mask != (o["new_target"] != ignore)
    n_diff = int(diff.sum())
    ref = o
    if n_diff:
        assert np.all(np.abs(o["target_prob"][diff] - o["threshold"]) <= near), o["target_prob"][diff]
        masked = np.where(kept_mask, target, ignore)
        ref = ohem(logits, masked, ignore_label=ignore, thresh=1.0, min_kept=0, factor=args.get("factor", 8))
    if np.isnan(ref["loss"]):
        assert np.isnan(loss) and not kept_mask.any() and np.all(grad == 0)
    else:
        assert abs(float(loss) - ref["loss"]) <= rtol * abs(ref["loss"]), (float(loss), ref["loss"])
        err = float(np.abs(grad - ref["grad"]).max())
        assert err <= gtol * float(np.abs(ref["grad"]).max()), err
    return o, n_diff


# ---- fixtures (tests/golden/ohem_*.npz, written by tests/golden/make_ohem_golden.py from the reference) ----
def load_fixture(path):
    """A fixture with its inputs regenerated from the stored seed."""
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    B, C, H, W = (int(v) for v in fx["shape"])
    fx["logits"], fx["target"] = make_case_inputs(B, C, H, W, int(fx["seed"]), all_ignored=bool(fx["all_ignored"]))
    fx["new_target"] = fx["new_target"].astype(np.int64)
    fx["args"] = dict(ignore_label=255, thresh=float(fx["thresh"]), min_kept=int(fx["min_kept"]), factor=8)
    return fx


def ulp_distance(a, b):
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


def check_against_fixture(fx, threshold, kept_mask, loss, grad, max_near=16, near=1e-6, rtol=1e-5, gtol=1e-5):
    """The numerics bar of a device (or emulated) result against a reference fixture.

    threshold within 2 fp32 ulp; the kept mask identical except for at most ``max_near`` pixels whose target probability
    lies within ``near`` of the threshold; loss within ``rtol`` relative and the gradient within ``gtol`` x max|grad|.
    When the masks differ in such pixels, loss and gradient are compared with the oracle evaluated on the device's mask
    (one pixel more or less moves the mean by far more than ``rtol``).  Returns the number of differing pixels."""
    assert ulp_distance(threshold, fx["threshold"]) <= 2, (float(threshold), float(fx["threshold"]))
    ref_mask = fx["new_target"] != 255
    diff = kept_mask != ref_mask
    n_diff = int(diff.sum())
    if n_diff:
        pt, _ = target_prob(softmax_f32(fx["logits"]), fx["target"])
        assert np.all(np.abs(pt[diff] - fx["threshold"]) <= near), pt[diff]
        assert n_diff <= max_near, n_diff
        masked = fx["target"].copy()
        masked[~kept_mask] = 255
        o = ohem(fx["logits"], masked, thresh=1.0, min_kept=0)
        ref_loss, ref_grad = o["loss"], o["grad"]
        ref_g = ref_grad if "grad" in fx else ref_grad.ravel()[fx["grad_index"]]
    else:
        ref_loss = float(fx["loss"])
        ref_g = fx["grad"] if "grad" in fx else fx["grad_sample"]
    got_g = grad if "grad" in fx else grad.ravel()[fx["grad_index"]]
    if np.isnan(ref_loss):
        assert np.isnan(loss) and not kept_mask.any() and np.all(grad == 0)
    else:
        assert abs(float(loss) - ref_loss) <= rtol * abs(ref_loss), (float(loss), ref_loss)
        scale = float(np.abs(ref_g).max())
        assert float(np.abs(got_g - ref_g).max()) <= gtol * scale, (float(np.abs(got_g - ref_g).max()), scale)
    return n_diff
