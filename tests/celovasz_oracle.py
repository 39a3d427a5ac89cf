"""What the tests of the fused CE + Lovász criterion (include/ccnet_celovasz.h, ccnet_amd/celovasz.py) share: the case table,
the seeded inputs, the fixture loader, a restatement of the criterion from what the suite already has, the numerics bars and
the C ABI on guarded buffers.

The fixtures (tests/golden/celovasz_*.npz, written by tests/golden/make_celovasz_golden.py from the unmodified reference
``CriterionOhemDSN2``, loss/criterion.py:59-78, run in fp32 on the CPU) hold the truth: loss, gradient of the low-resolution
logits, and for the two terms a stock-op cross-entropy of the same up-sample and the reference's own ``lovasz_softmax``.
:func:`reference` is the same composition restated: ``F.interpolate`` + ``F.cross_entropy`` + ``F.softmax`` as stock ops on the
CPU and :func:`lovasz_oracle.lovasz_softmax` (stable tie order, the device's rule) for the Lovász term, in fp32 or float64.
It serves the variants the reference's criterion cannot express (``per_image``, ``classes``) and the cases it cannot run
(labels outside [0, C), nothing valid).  Test infrastructure only.
"""
import glob
import os

import numpy as np

import dsn_oracle as DS
import lovasz_oracle as LO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the project's bars for this criterion (tests/test_gpu_lovasz.py, test_criterion_against_reference_fixture_and_oracle_composition)
LOSS_RTOL = 1e-5                 # loss, and each of CE and LS, within 1e-5 relative
GRAD_RTOL = 1e-4                 # every gradient element within 1e-4 of max|grad|
FULL_GRAD_MAX = 1 << 16          # fixtures keep every gradient element up to this size, else GRAD_SAMPLE of them
GRAD_SAMPLE = 16384
IGNORE = 255
RECIPE_FIXTURE = os.path.join(GOLDEN, "lovasz_criterion_1x19x97x97_769.npz")     # tests/golden/make_lovasz_golden.py's, read only

# name: (B, C, h, w, H, W, seed, logit scale, number of classes the labels are drawn from (0: all), all_ignored)
# Every case has at least three sort tiles (2048 positions each) per segment unless noted.
CASES = {
    "frac": (1, 5, 9, 11, 67, 83, 1, 3.0, 0, False),            # non-integer ratios, non-square
    "s8": (2, 19, 13, 13, 97, 97, 2, 3.0, 0, False),            # exact ratio 8, a segment spans both images
    "identity": (1, 19, 72, 72, 72, 72, 3, 3.0, 0, False),      # scale 1: the interpolated logits are the logits
    "one": (2, 19, 1, 1, 17, 19, 4, 3.0, 0, False),             # one low-resolution pixel: every error of a class ties (one tile)
    "one_row": (1, 19, 1, 9, 70, 70, 5, 3.0, 0, False),         # h = 1: every column of 70 pixels ties
    "hot": (2, 19, 13, 13, 97, 97, 6, 30.0, 0, False),          # logits x 10: p saturates, sign(0) = 0
    "absent": (2, 19, 13, 13, 97, 97, 7, 3.0, 5, False),        # labels from 5 of the 19 classes: 'present' drops 14
    "c150": (1, 150, 4, 4, 66, 66, 8, 3.0, 0, False),           # class loops beyond a wave
    "out_of_range": (1, 19, 9, 11, 67, 83, 9, 3.0, 0, False),   # labels outside [0, C) beside 255 (see case_inputs)
    "ignored": (1, 19, 5, 5, 65, 65, 10, 3.0, 0, True),         # nothing valid: NaN loss, gradient exactly 0
}
# the reference's cross-entropy raises on a label outside [0, C) and its Lovász term returns an empty tensor without a valid pixel
ORACLE_ONLY = ("out_of_range", "ignored")
# the criterion's arguments the reference does not pass (it calls lovasz_softmax(..., ignore=255)): run at s8, against reference()
VARIANTS = {"per_image": dict(per_image=True), "all": dict(classes="all"), "list": dict(classes=[1, 3, 3, 18]),
            "list_per_image": dict(classes=[0, 2, 2], per_image=True)}


def fixture_path(name):
    return os.path.join(GOLDEN, "celovasz_" + name + ".npz")


def fixture_names():
    return sorted(os.path.basename(p)[len("celovasz_"):-4] for p in glob.glob(os.path.join(GOLDEN, "celovasz_*.npz")))


def upsample(x, size, dtype=None):
    """F.interpolate(mode="bilinear", align_corners=True) of a numpy (B, C, h, w) array, as a torch tensor of ``dtype``."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype or torch.float32)
    return F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True)


def make_case_inputs(B, C, h, w, H, W, seed, scale=3.0, drawn=0, all_ignored=False, agree=0.5, ignored=0.05):
    """Seeded (fp32 (B, C, h, w) logits, int64 (B, H, W) target).  ``agree`` of the labels are the argmax of the up-sampled
    logits (small errors), the rest uniform (large ones); with ``drawn`` > 0 every label is folded onto the first ``drawn``
    classes; about ``ignored`` of them are 255."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C, h, w)) * scale).astype(np.float32)
    target = upsample(logits, (H, W)).argmax(1).numpy().astype(np.int64)
    rand = rng.integers(0, C, (B, H, W)).astype(np.int64)
    pick = rng.random((B, H, W)) >= agree
    target[pick] = rand[pick]
    if drawn:
        target %= drawn
    target[rng.random((B, H, W)) < ignored] = IGNORE
    if all_ignored:
        target[:] = IGNORE
    return logits, target


def case_inputs(name):
    """(logits, target) of one CASES entry."""
    B, C, h, w, H, W, seed, scale, drawn, all_ignored = CASES[name]
    logits, target = make_case_inputs(B, C, h, w, H, W, seed, scale, drawn, all_ignored)
    if name == "out_of_range":
        rng = np.random.default_rng(seed + 1000)
        pick = rng.random(target.shape) < 0.05
        target[pick] = rng.integers(C, IGNORE, int(pick.sum()))
        target[0, 0, :7] = [-1, -5, C, 254, 256, 2 ** 40, -2 ** 40]
    return logits, target


def load_fixture(name):
    """The fixture as a dict, with its inputs regenerated from the stored seed."""
    z = np.load(fixture_path(name))
    fx = {k: z[k] for k in z.files}
    B, C, h, w, H, W = (int(v) for v in fx["shape"])
    fx["logits"], fx["target"] = make_case_inputs(B, C, h, w, H, W, int(fx["seed"]), float(fx["scale"]), int(fx["drawn"]),
                                                  bool(fx["all_ignored"]))
    fx["name"] = name
    return fx


def clean_labels(target, C, ignore=IGNORE):
    """The labels as the criterion reads them: anything outside [0, C) is ``ignore``.  Returns (labels, out-of-range count)."""
    bad = ((target < 0) | (target >= C)) & (target != ignore)
    return np.where(bad, ignore, target), int(bad.sum())


def stock_cross_entropy(logits, target, ignore=IGNORE, dtype=None):
    """The cross-entropy term alone, as dsn_oracle restates it (F.interpolate + F.cross_entropy on the CPU): (CE, gradient)."""
    labels, _ = clean_labels(target, logits.shape[1], ignore)
    ce, grads = DS.stock_reference([logits], labels, ignore_index=ignore, weights=(1.0,), dtype=dtype)
    return ce, grads[0]


def reference(logits, target, classes="present", per_image=False, ignore=IGNORE, dtype=None, grad_out=1.0):
    """The criterion restated on the CPU: stock up-sample, cross-entropy and softmax in ``dtype`` (fp32 unless stated; float64
    is the measuring stick) and lovasz_oracle.lovasz_softmax on that softmax.  Returns loss, head_loss (CE, LS), grad, valid,
    out_of_range, n_kept.  With no valid pixel: NaN loss, zero gradient."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    C = logits.shape[1]
    labels, oor = clean_labels(target, C, ignore)
    valid = int((labels != ignore).sum())
    if valid == 0:
        return {"loss": float("nan"), "head_loss": [float("nan"), 0.0], "grad": np.zeros(logits.shape, np.float64), "valid": 0,
                "out_of_range": oor, "n_kept": 0}
    x = torch.from_numpy(np.asarray(logits)).to(dtype).requires_grad_(True)
    t = torch.from_numpy(labels)
    up = F.interpolate(x, size=t.shape[1:], mode="bilinear", align_corners=True)
    ce = F.cross_entropy(up, t, ignore_index=ignore)
    prob = F.softmax(up, dim=1)
    o = LO.lovasz_softmax(prob.detach().numpy(), labels, classes=classes, per_image=per_image, ignore=ignore)
    ((ce + (prob * torch.from_numpy(o["grad"]).to(dtype)).sum()) * grad_out).backward()
    return {"loss": float(ce.detach()) + o["loss"], "head_loss": [float(ce.detach()), o["loss"]],
            "grad": x.grad.numpy().astype(np.float64), "valid": valid, "out_of_range": oor, "n_kept": o["n_kept"]}


def _rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want)) if want else abs(float(got))


def check_result(name, r, loss, head_loss, grad_pick, valid, out_of_range, n_kept, out=print):
    """Hold a device (or emulated) result ``r`` (loss, head_loss, grad, valid, out_of_range, n_kept) to the bars.  ``grad_pick``
    is (index or None, reference values, max|grad|).  Every figure is printed before it is asserted.  Returns the figures."""
    assert (int(r["valid"]), int(r["out_of_range"]), int(r["n_kept"])) == (int(valid), int(out_of_range), int(n_kept)), \
        (r["valid"], r["out_of_range"], r["n_kept"], valid, out_of_range, n_kept)
    g = np.asarray(r["grad"], np.float32)
    assert np.isfinite(g).all(), "gradient elements not written or not finite"
    if np.isnan(loss):
        out(f"{name}: loss {r['loss']!r} (reference NaN), head losses {list(map(float, r['head_loss']))}")
        assert np.isnan(r["loss"]) and np.isnan(r["head_loss"][0]) and float(r["head_loss"][1]) == 0.0
        assert not g.any(), "nothing valid: the gradient is exactly zero"
        return {"loss": 0.0, "grad": 0.0}
    rel = _rel(r["loss"], loss)
    out(f"{name}: loss {float(r['loss'])!r} reference {float(loss)!r} relative error {rel:.3g} (bar {LOSS_RTOL:g})")
    rels = [_rel(r["head_loss"][k], head_loss[k]) for k in range(2)]
    for k, what in enumerate(("CE", "LS")):
        out(f"{name}: {what} {float(r['head_loss'][k])!r} reference {float(head_loss[k])!r} relative error {rels[k]:.3g} "
            f"(bar {LOSS_RTOL:g})")
    idx, want, top = grad_pick
    got = g.ravel() if idx is None else g.ravel()[idx]
    err = float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64).ravel()).max())
    out(f"{name}: max|grad| {top:.6g} max error {err:.3g} = {err / top if top else 0:.3g} of max|grad| (bar {GRAD_RTOL:g})")
    assert rel <= LOSS_RTOL, (float(r["loss"]), float(loss), rel)
    assert max(rels) <= LOSS_RTOL, (list(map(float, r["head_loss"])), list(map(float, head_loss)), rels)
    assert top > 0 and err <= GRAD_RTOL * top, (err, top)
    return {"loss": rel, "grad": err / top}


def fixture_grad(fx):
    if "grad" in fx:
        return None, fx["grad"].ravel(), float(fx["grad_absmax"])
    return fx["grad_index"], fx["grad_sample"], float(fx["grad_absmax"])


def check_against_fixture(fx, r, out=print):
    """:func:`check_result` against a fixture: the reference's own fp32 numbers."""
    return check_result(fx["name"], r, float(fx["loss"]), [float(v) for v in fx["head_loss"]], fixture_grad(fx),
                        int(fx["valid"]), 0, int(fx["n_kept"]), out)


def check_against_oracle(name, logits, target, r, out=print, **args):
    """:func:`check_result` against :func:`reference` in float64 on the same inputs (variants and oracle-only cases)."""
    import torch
    ref = reference(logits, target, dtype=torch.float64, **args)
    return check_result(name, r, ref["loss"], ref["head_loss"], (None, ref["grad"], float(np.abs(ref["grad"]).max())),
                        ref["valid"], ref["out_of_range"], ref["n_kept"], out)


# ---- the C ABI on guarded buffers (guarded_memory.HostMemory for the emulator build, DeviceMemory on the GPU) ----
def align256(n):
    return (n + 255) & ~255


def workspace_regions(ws, B, H, W):
    """The two documented regions at the start of a workspace (uint8 array): the fp32 log-sum-exp and the int16 label per pixel
    (-1 when not valid), each rounded up to 256 bytes (include/ccnet_celovasz.h)."""
    ws = np.asarray(ws).view(np.uint8)
    N = B * H * W
    lse = ws[:4 * N].view(np.float32).reshape(B, H, W)
    at = align256(4 * N)
    return lse, ws[at:at + 2 * N].view(np.int16).reshape(B, H, W)


def run_raw(lib, mem, logits, target, classes="present", per_image=False, ignore=IGNORE, grad_out=1.0):
    """forward + two backwards through the C ABI on guarded buffers of ``mem``.  Gradients, loss and workspace start as NaN;
    returns the results (the form :func:`check_result` takes, ``grad2`` from the second backward, ``lse`` and ``labels`` from
    the workspace) and whether every guard band is intact."""
    import ctypes

    from ccnet_amd._lovasz_lib import class_selection
    from guarded_memory import Buf
    B, C, h, w = logits.shape
    H, W = target.shape[1:]
    n = lib.ccnet_celovasz_workspace_bytes(B, C, h, w, H, W, int(per_image))
    assert n > 0 and n % 4 == 0, n
    present_only, weights = class_selection(classes, C)
    wptr = None if weights is None else ctypes.addressof(weights)
    nan = np.full(1, np.nan, np.float32)
    x = Buf(mem, "logits", "f32", logits.size, data=np.ascontiguousarray(logits, np.float32))
    g = [Buf(mem, f"grad{k}", "f32", logits.size, data=np.full(logits.size, np.nan, np.float32)) for k in range(2)]
    t = Buf(mem, "target", "f64", target.size, data=np.ascontiguousarray(target, np.int64))
    loss = Buf(mem, "loss", "f32", 1, data=nan)
    head_loss = Buf(mem, "head_loss", "f32", 2, data=np.repeat(nan, 2))
    counts = Buf(mem, "counts", "f32", 3, data=np.full(3, -7, np.int32))
    ws = Buf(mem, "workspace", "f32", n // 4, data=np.full(n // 4, np.nan, np.float32))
    go = Buf(mem, "grad_out", "f32", 1, data=np.full(1, grad_out, np.float32))
    lib.check(lib.ccnet_celovasz_forward_f32(x.ptr, t.ptr, ignore, int(per_image), int(present_only), wptr, loss.ptr,
                                             head_loss.ptr, counts.ptr, ws.ptr, n, B, C, h, w, H, W, mem.stream), "forward")
    for k in range(2):
        lib.check(lib.ccnet_celovasz_backward_f32(go.ptr, x.ptr, g[k].ptr, ws.ptr, n, B, C, h, w, H, W, int(per_image),
                                                  mem.stream), "backward")
    intact, res = True, {}
    for buf, key, dt in [(loss, "loss", np.float32), (head_loss, "head_loss", np.float32), (counts, "counts", np.int32),
                         (ws, "workspace", np.uint8), (g[0], "grad", np.float32), (g[1], "grad2", np.float32)]:
        res[key], ok = buf.read(dt)
        assert ok, f"guard band of {key} overwritten"
        intact = intact and ok
    for buf in (x, t, go):
        intact = intact and buf.read(np.uint8)[1]
    c = res["counts"]
    lse, labels = workspace_regions(res["workspace"], B, H, W)
    return {"loss": float(res["loss"][0]), "head_loss": res["head_loss"], "valid": int(c[0]), "out_of_range": int(c[1]),
            "n_kept": int(c[2]), "grad": res["grad"].reshape(logits.shape), "grad2": res["grad2"].reshape(logits.shape),
            "lse": lse, "labels": labels, "workspace_bytes": n, "intact": intact}
