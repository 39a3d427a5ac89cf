"""What the tests of the fused OHEM + DSN criterion (include/ccnet_ohemdsn.h, ccnet_amd/ohemdsn.py) share: the case table, the
seeded inputs, the fixture loader, a restatement of the criterion from what the suite already has, and the numerics bar.

The fixtures (tests/golden/ohemdsn_*.npz, written by tests/golden/make_ohemdsn_golden.py from the unmodified reference
``CriterionOhemDSN``, loss/criterion.py:37-56) hold the truth: threshold and kept mask from the reference's own fp32 run,
loss and gradients from its run on float64 logits.  :func:`reference` is the same composition restated: the up-sample is
``F.interpolate`` in the requested dtype, threshold and mask are :func:`ohem_oracle.ohem` on its softmax (``prob=``), loss and
gradients are torch autograd in float64 on that mask.  It serves the cases no fixture covers.  Test infrastructure only.
"""
import glob
import os

import numpy as np

import ohem_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_RTOL = 1e-5                 # loss and each head's CE within 1e-5 relative of the float64 reference
GRAD_RTOL = 1e-5                 # every gradient element within 1e-5 of that head's max|grad|
AUX_WEIGHT = 0.4                 # loss/criterion.py:56
MAX_NEAR = 16                    # at most this many pixels of a case may sit inside the window and differ

# The k-th probability -- hence the threshold and the kept mask -- is pinned only up to the fp32 rounding of the up-sample and
# the softmax.  MEASURED_P_GAP is the largest max|p_target(fp32 run) - p_target(float64 run)| of the reference against itself
# over all fixtures, as tests/golden/make_ohemdsn_golden.py printed it; NEAR = 2 x that is the comparison window: the device
# threshold lies within NEAR of the fixture's, and the kept masks may differ only at pixels whose reference p_target lies
# within 2 * NEAR of the reference threshold.
MEASURED_P_GAP = 4.5627585e-06
NEAR = 2 * MEASURED_P_GAP

# name: (B, C, h, w, H, W, seed, heads, logit scale, all_ignored, thresh, min_kept, the branch the case claims)
CASES = {
    "kth": (2, 19, 13, 13, 97, 97, 1, 2, 3.0, False, 0.3, 64 * 150, "kth_above"),       # k-th above thresh, B = 2, ratio 8
    "below": (2, 19, 13, 13, 97, 97, 6, 2, 3.0, False, 0.7, 6400, "kth_below"),         # k-th below thresh
    "hw": (1, 19, 17, 33, 129, 257, 2, 2, 3.0, False, 0.7, 20000, "any"),               # h != w
    "frac": (1, 19, 7, 11, 50, 83, 3, 2, 3.0, False, 0.5, 64 * 30, "any"),              # inexact scale; zoomed grid 6 x 10
    "identity": (1, 19, 24, 40, 24, 40, 4, 2, 3.0, False, 0.7, 64 * 4, "any"),          # scale 1: also ohem.OhemCrossEntropy2d's
    "line": (1, 19, 1, 9, 16, 65, 5, 2, 3.0, False, 0.7, 64, "any"),                    # h = 1
    "keepall": (1, 19, 9, 9, 65, 65, 3, 2, 3.0, False, 0.7, 100000, "one"),             # threshold 1.0
    "minkept0": (1, 19, 9, 13, 65, 97, 4, 2, 3.0, False, 0.7, 63, "thresh"),            # min_kept // 64 == 0
    "zoomed0": (1, 19, 2, 5, 3, 30, 8, 2, 3.0, False, 0.7, 100, "one"),                 # zoomed height 0: no keys at all
    "ignored": (1, 19, 5, 5, 33, 33, 5, 2, 3.0, True, 0.7, 100000, "none_kept"),        # nothing valid: NaN loss, zero gradients
    "c150": (1, 150, 6, 6, 41, 41, 9, 2, 3.0, False, 0.7, 64 * 8, "any"),               # class loop beyond a wave
    # (logits x 30 saturate 70 % of the probabilities at 1.0: with min_kept 6400 the k-th key sits among them, where fp32 and
    # float64 disagree on thousands of pixels at every seed tried; 64 * 20 puts it among the wrong labels, threshold 0.7)
    "hot": (1, 19, 13, 13, 97, 97, 7, 2, 90.0, False, 0.7, 64 * 20, "kth_below"),       # logits x 30: softmax range
    "one_head": (1, 19, 13, 13, 97, 97, 10, 1, 3.0, False, 0.6, 6400, "any"),           # heads == 1
    "recipe": (1, 19, 97, 97, 769, 769, 11, 2, 3.0, False, 0.6, 200000, "recipe"),      # the training shape, once
}
# scipy's zoom refuses an empty output, so the reference cannot run this case: the oracle alone serves it
ORACLE_ONLY = ("zoomed0",)


def fixture_path(name):
    return os.path.join(GOLDEN, "ohemdsn_" + name + ".npz")


def fixture_names():
    return sorted(os.path.basename(p)[len("ohemdsn_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ohemdsn_*.npz")))


def upsample(x, size, dtype=None):
    """F.interpolate(mode="bilinear", align_corners=True) of a numpy (B, C, h, w) array, as a torch tensor of ``dtype``."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype or torch.float32)
    return F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True)


def make_case_inputs(B, C, h, w, H, W, seed, heads=2, scale=3.0, all_ignored=False, agree=0.70, ignored=0.05):
    """Seeded ([fp32 (B, C, h, w) logits per head], int64 (B, H, W) target).  ``agree`` of the labels are the argmax of the
    up-sampled main logits, the rest random (with purely random labels nearly every pixel is hard and the threshold separates
    nothing); about ``ignored`` of them are 255."""
    rng = np.random.default_rng(seed)
    logits = [(rng.standard_normal((B, C, h, w)) * scale).astype(np.float32) for _ in range(heads)]
    target = upsample(logits[0], (H, W)).argmax(1).numpy().astype(np.int64)
    rand = rng.integers(0, C, (B, H, W)).astype(np.int64)
    pick = rng.random((B, H, W)) >= agree
    target[pick] = rand[pick]
    target[rng.random((B, H, W)) < ignored] = 255
    if all_ignored:
        target[:] = 255
    return logits, target


def case_inputs(name, seed=None):
    """(logits, target, criterion args) of one CASES entry."""
    B, C, h, w, H, W, s, heads, scale, all_ignored, thresh, min_kept, _ = CASES[name]
    logits, target = make_case_inputs(B, C, h, w, H, W, s if seed is None else seed, heads, scale, all_ignored)
    return logits, target, dict(thresh=thresh, min_kept=min_kept)


def load_fixture(name):
    """The fixture as a dict, with its inputs regenerated from the stored seed."""
    z = np.load(fixture_path(name))
    fx = {k: z[k] for k in z.files}
    B, C, h, w, H, W = (int(v) for v in fx["shape"])
    fx["heads"] = int(fx["heads"])
    fx["logits"], fx["target"] = make_case_inputs(B, C, h, w, H, W, int(fx["seed"]), fx["heads"], float(fx["scale"]),
                                                  bool(fx["all_ignored"]))
    fx["args"] = dict(thresh=float(fx["thresh"]), min_kept=int(fx["min_kept"]))
    fx["kept_mask"] = fx["new_target"] != 255
    fx["name"] = name
    return fx


def select(logits0, target, thresh, min_kept, ignore_label=255, factor=8, dtype=None):
    """Threshold and kept mask of the OHEM head: ohem_oracle.ohem on the softmax of the up-sampled main logits (``dtype``:
    fp32 unless stated).  Returns ohem_oracle.ohem's dict: threshold, new_target, kept, target_prob, valid, num_valid."""
    import torch
    up = upsample(logits0, target.shape[1:], dtype)
    prob = torch.softmax(up, 1).numpy()
    return O.ohem(up.numpy(), target, ignore_label, thresh, min_kept, factor, prob=prob)


def masked_loss(logits, target, kept_mask, ignore_label=255):
    """Loss, both heads' cross-entropies and the gradients of the low-resolution logits in float64, for a given kept mask:
    CE(up(logits0), target where kept) [+ 0.4 * CE(up(logits1), target)] through torch autograd."""
    import torch
    import torch.nn.functional as F
    xs = [torch.from_numpy(np.asarray(l)).to(torch.float64).requires_grad_(True) for l in logits]
    t = torch.from_numpy(np.asarray(target))
    t0 = torch.from_numpy(np.where(kept_mask, target, ignore_label))
    ce = [F.cross_entropy(F.interpolate(xs[0], size=t.shape[1:], mode="bilinear", align_corners=True), t0,
                          ignore_index=ignore_label)]
    if len(xs) == 2:
        ce.append(F.cross_entropy(F.interpolate(xs[1], size=t.shape[1:], mode="bilinear", align_corners=True), t,
                                  ignore_index=ignore_label))
    loss = ce[0] + ce[1] * AUX_WEIGHT if len(xs) == 2 else ce[0]
    loss.backward()
    return float(loss.detach()), [float(c.detach()) for c in ce], [x.grad.numpy() for x in xs]


def reference(logits, target, thresh, min_kept, ignore_label=255, factor=8, kept_mask=None):
    """The whole criterion restated.  Threshold and mask come from the fp32 up-sample (the reference's own arithmetic) unless
    ``kept_mask`` gives the mask; loss, head losses and gradients are float64 on that mask."""
    sel = select(logits[0], target, thresh, min_kept, ignore_label, factor)
    mask = sel["new_target"] != ignore_label if kept_mask is None else kept_mask
    loss, head_loss, grads = masked_loss(logits, target, mask, ignore_label)
    return {"threshold": sel["threshold"], "kept_mask": mask, "target_prob": sel["target_prob"], "valid": sel["valid"],
            "num_valid_zoomed": sel["num_valid"], "loss": loss, "head_loss": head_loss, "grads": grads}


def _check_numbers(name, r, heads, loss, head_loss, grads, grad_refs, out):
    """loss, head losses, gradients of a result ``r`` against float64 ones; ``grad_refs``: per head (got, want, max|grad|)"""
    if np.isnan(loss):
        out(f"{name}: loss {r['loss']!r} (reference NaN)")
        assert np.isnan(r["loss"])
    else:
        rel = abs(float(r["loss"]) - loss) / abs(loss)
        out(f"{name}: loss {float(r['loss'])!r} reference {loss!r} relative error {rel:.3g} (bar {LOSS_RTOL:g})")
        assert rel <= LOSS_RTOL, (float(r["loss"]), loss, rel)
    for k in range(heads):
        got, want = float(r["head_loss"][k]), float(head_loss[k])
        if np.isnan(want):
            assert np.isnan(got), (k, got)
        else:
            rel = abs(got - want) / abs(want)
            out(f"{name}: head {k} CE {got!r} reference {want!r} relative error {rel:.3g} (bar {LOSS_RTOL:g})")
            assert rel <= LOSS_RTOL, (k, got, want)
    assert len(grads) == heads
    for k, (got, want, top) in enumerate(grad_refs):
        g = np.asarray(grads[k], np.float32)
        assert np.isfinite(g).all(), f"head {k}: gradient elements not written or not finite"
        err = float(np.abs(got.astype(np.float64) - want).max())
        out(f"{name}: head {k} max|grad| {top:.6g} max error {err:.3g} = {err / top if top else 0:.3g} of max|grad| "
            f"(bar {GRAD_RTOL:g})")
        assert err <= GRAD_RTOL * top, (k, err, top)
        if top == 0:
            assert not g.any()


def check_result(name, logits, target, args, r, ref_threshold, ref_mask, ref_prob, ref_numbers=None, out=print):
    """Hold a device (or emulated) result to the bar.  ``r``: threshold, kept_mask (bool (B, H, W)), kept, valid,
    num_valid_zoomed, out_of_range, loss, head_loss, grads.  ``ref_prob`` is the reference's p_target per pixel, or a
    callable that gives it (evaluated only if the masks differ); ``ref_numbers`` is (loss, head losses, per head (index or None,
    gradient values, max|grad|)) for the reference mask; when the device's mask differs inside the window, or none is given,
    loss and gradients come from :func:`masked_loss` on the device's own mask.  Returns the number of differing pixels."""
    heads = len(logits)
    valid = target != 255
    thr_gap = abs(float(r["threshold"]) - float(ref_threshold))
    out(f"{name}: threshold {float(r['threshold'])!r} reference {float(ref_threshold)!r} gap {thr_gap:.3g} (window {NEAR:.3g})")
    assert thr_gap <= NEAR, (float(r["threshold"]), float(ref_threshold))
    mask = np.asarray(r["kept_mask"], bool)
    assert not (mask & ~valid).any()
    diff = mask != ref_mask
    n_diff = int(diff.sum())
    if n_diff:
        gap = np.abs((ref_prob() if callable(ref_prob) else ref_prob)[diff].astype(np.float64) - float(ref_threshold))
        out(f"{name}: kept masks differ at {n_diff} pixels, |p_target - threshold| up to {gap.max():.3g}")
        assert np.all(gap <= 2 * NEAR), gap.max()
        assert n_diff <= MAX_NEAR, n_diff
    # the counts are exact given the mask
    assert int(r["kept"]) == int(mask.sum()) and int(r["valid"]) == int(valid.sum()) and int(r["out_of_range"]) == 0
    if n_diff or ref_numbers is None:
        loss, head_loss, g64 = masked_loss(logits, target, mask)
        refs = [(np.asarray(r["grads"][k]).ravel(), g64[k].ravel(), float(np.abs(g64[k]).max())) for k in range(heads)]
    else:
        loss, head_loss, picks = ref_numbers
        refs = [(np.asarray(r["grads"][k]).ravel() if idx is None else np.asarray(r["grads"][k]).ravel()[idx], want, top)
                for k, (idx, want, top) in enumerate(picks)]
    _check_numbers(name, r, heads, loss, head_loss, r["grads"], refs, out)
    return n_diff


def fixture_numbers(fx):
    picks = []
    for k in range(fx["heads"]):
        if f"grad{k}" in fx:
            picks.append((None, fx[f"grad{k}"].ravel(), float(fx[f"grad{k}_max"])))
        else:
            picks.append((fx[f"grad{k}_index"], fx[f"grad{k}_sample"], float(fx[f"grad{k}_max"])))
    return float(fx["loss"]), [float(v) for v in fx["head_loss"]], picks


def check_against_fixture(fx, r, out=print):
    """:func:`check_result` against a fixture: threshold and mask of the reference's fp32 run, numbers of its float64 run."""
    assert int(r["num_valid_zoomed"]) == int(fx["num_valid_zoomed"])
    prob = lambda: select(fx["logits"][0], fx["target"], **fx["args"])["target_prob"]      # noqa: E731  (only if masks differ)
    return check_result(fx["name"], fx["logits"], fx["target"], fx["args"], r, fx["threshold"], fx["kept_mask"], prob,
                        fixture_numbers(fx), out)


def check_against_oracle(name, logits, target, args, r, out=print):
    """:func:`check_result` against :func:`reference` on the same inputs (the cases without a fixture)."""
    sel = select(logits[0], target, **args)
    assert int(r["num_valid_zoomed"]) == int(sel["num_valid"])
    return check_result(name, logits, target, args, r, sel["threshold"], sel["new_target"] != 255, sel["target_prob"], None, out)


# ---- the C ABI on guarded buffers (guarded_memory.HostMemory for the emulator build, DeviceMemory on the GPU) ----
def align256(n):
    return (n + 255) & ~255


def workspace_kept_mask(ws, B, H, W, heads, factor=8):
    """The kept mask from the saved labels of a workspace (uint8 array): include/ccnet_ohemdsn.h lays the workspace out as the
    uint32 keys, the fp32 log-sum-exps (one plane per head), then the int16 labels (label | 0x100 when kept, -1 when not
    valid), each rounded up to 256 bytes."""
    ws = np.asarray(ws).view(np.uint8)
    N, M = B * H * W, B * O.zoom_out_size(H, factor) * O.zoom_out_size(W, factor)
    at = align256(4 * M) + align256(4 * N * heads)
    lab = ws[at:at + 2 * N].view(np.int16).reshape(B, H, W)
    return (lab >= 0) & ((lab & 0x100) != 0)


def run_raw(lib, mem, logits, target, thresh, min_kept, ignore_label=255, factor=8, grad_out=1.0):
    """forward + backward through the C ABI on guarded buffers of ``mem``.  Gradients, loss and workspace start as NaN;
    returns the results (the form :func:`check_result` takes) and whether every guard band is intact."""
    from guarded_memory import Buf
    heads = len(logits)
    B, C, h, w = logits[0].shape
    H, W = target.shape[1:]
    n = lib.ccnet_ohemdsn_workspace_bytes(B, C, h, w, H, W, heads, factor)
    M = B * O.zoom_out_size(H, factor) * O.zoom_out_size(W, factor)
    assert 0 < n <= 16 * B * H * W + 4 * M + 65536 and n % 4 == 0, n
    nan = np.full(1, np.nan, np.float32)
    x = [Buf(mem, f"logits{k}", "f32", l.size, data=np.ascontiguousarray(l, np.float32)) for k, l in enumerate(logits)]
    g = [Buf(mem, f"grad{k}", "f32", l.size, data=np.full(l.size, np.nan, np.float32)) for k, l in enumerate(logits)]
    t = Buf(mem, "target", "f64", target.size, data=np.ascontiguousarray(target, np.int64))
    loss = Buf(mem, "loss", "f32", 1, data=nan)
    head_loss = Buf(mem, "head_loss", "f32", 2, data=np.repeat(nan, 2))
    thr = Buf(mem, "threshold", "f32", 1, data=nan)
    counts = Buf(mem, "counts", "f32", 4, data=np.full(4, -7, np.int32))
    ws = Buf(mem, "workspace", "f32", n // 4, data=np.full(n // 4, np.nan, np.float32))
    go = Buf(mem, "grad_out", "f32", 1, data=np.full(1, grad_out, np.float32))
    second = (lambda bufs: bufs[1].ptr if heads == 2 else None)
    lib.check(lib.ccnet_ohemdsn_forward_f32(x[0].ptr, second(x), t.ptr, ignore_label, thresh, min_kept, factor, loss.ptr,
                                            head_loss.ptr, thr.ptr, counts.ptr, ws.ptr, n, B, C, h, w, H, W, heads, mem.stream),
              "forward")
    lib.check(lib.ccnet_ohemdsn_backward_f32(go.ptr, x[0].ptr, second(x), g[0].ptr, second(g), ws.ptr, n, B, C, h, w, H, W,
                                             heads, factor, mem.stream), "backward")
    intact, res = True, {}
    for buf, key, dt in [(loss, "loss", np.float32), (head_loss, "head_loss", np.float32), (thr, "threshold", np.float32),
                         (counts, "counts", np.int32), (ws, "workspace", np.uint8)] \
            + [(b, f"grad{k}", np.float32) for k, b in enumerate(g)]:
        res[key], ok = buf.read(dt)
        assert ok, f"guard band of {key} overwritten"
        intact = intact and ok
    for buf in x + [t, go]:
        intact = intact and buf.read(np.uint8)[1]
    c = res["counts"]
    return {"loss": float(res["loss"][0]), "head_loss": res["head_loss"], "threshold": res["threshold"][0], "kept": int(c[0]),
            "valid": int(c[1]), "num_valid_zoomed": int(c[2]), "out_of_range": int(c[3]),
            "kept_mask": workspace_kept_mask(res["workspace"], B, H, W, heads, factor),
            "grads": [res[f"grad{k}"].reshape(logits[k].shape) for k in range(heads)], "intact": intact}
