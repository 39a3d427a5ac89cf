"""numpy restatement of the reference Lovász-softmax loss (loss/lovasz_losses.py:18-31,153-218, ``lovasz_softmax``) with
the device's tie rule: errors sort in descending order with a STABLE argsort, so equal errors keep ascending flattened pixel
order.  ``lovasz_grad``'s arithmetic is restated as the device pins it (exact integer prefix counts converted to fp32,
correctly rounded fp32 division), so for the same sorted fg the per-position weights g are bit-identical.

The reference's own ``torch.sort`` leaves the order inside a group of equal errors unspecified.  The loss does not depend on
it, the per-pixel gradient does; :func:`check_against_fixture` therefore compares gradients tie-aware: pixels whose error is
unique in their (segment, class) elementwise, every other (segment, class, equal-error) group by the sum of its gradient
times -sign(fg - p) (the sum of its g, which a group's order cannot change).  Everything here is test infrastructure.
"""
import numpy as np

FULL_GRAD_MAX = 1 << 16        # fixtures keep every gradient element up to this size, else GRAD_SAMPLE of them
GRAD_SAMPLE = 16384
GROUP_SAMPLE = 16384
NO_GROUP = np.uint64(0xffffffffffffffff)


def softmax_f32(logits):
    """Softmax over axis 1 in double, rounded to fp32 (portable: no vectorised fp32 exp whose last bit depends on the CPU)."""
    x = logits.astype(np.float64)
    x = np.exp(x - x.max(axis=1, keepdims=True))
    return (x / x.sum(axis=1, keepdims=True)).astype(np.float32)


def make_case_inputs(B, C, H, W, seed, scale=3.0, ignore_frac=0.05, extra_frac=0.0, absent=None):
    """Seeded probabilities and labels of one case (tests/golden/make_lovasz_golden.py regenerates them the same way):
    softmax of N(0, scale^2) logits; labels uniform in [0, C), ``extra_frac`` of them moved to [C, 255), ``ignore_frac``
    set to 255, and class ``absent`` (if any) replaced by its neighbour."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C, H, W)) * scale).astype(np.float32)
    labels = rng.integers(0, C, (B, H, W)).astype(np.int64)
    if extra_frac:
        extra = rng.random((B, H, W)) < extra_frac
        labels[extra] = rng.integers(C, 255, int(extra.sum()))
    labels[rng.random((B, H, W)) < ignore_frac] = 255
    if absent is not None:
        labels[labels == absent] = (absent + 1) % C
    return softmax_f32(logits), labels


def class_weights(classes, C):
    """(multiplicity of every class, present_only) for the reference's ``classes`` argument."""
    if isinstance(classes, str):
        assert classes in ("present", "all"), classes
        return np.ones(C, np.int64), classes == "present"
    return np.bincount(np.asarray(list(classes), np.int64), minlength=C), False


def lovasz_segment(pc, fg, valid):
    """One class over one segment (pixels in flattened order).  Returns (loss_seg in double, gts, d) with d = g * (-sign(fg
    - p)) scattered back to pixel order (fp32, 0 where not valid)."""
    out = np.zeros(len(pc), np.float32)
    idx = np.nonzero(valid)[0]
    if len(idx) == 0:
        return 0.0, 0, out
    f = fg[idx]
    d = f.astype(np.float32) - pc[idx]
    e = np.abs(d)
    order = np.argsort(-e, kind="stable")
    fs = f[order].astype(np.int64)
    gts = int(fs.sum())
    cf = np.cumsum(fs)
    cb = np.arange(1, len(idx) + 1) - cf
    J = np.float32(1) - (gts - cf).astype(np.float32) / (gts + cb).astype(np.float32)
    g = J.copy()
    g[1:] = J[1:] - J[:-1]
    loss = float(np.dot(e[order].astype(np.float64), g.astype(np.float64)))
    sign = np.where(d < 0, 1, np.where(d > 0, -1, 0)).astype(np.float32)
    out[idx[order]] = g * sign[order]
    return loss, gts, out


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None, grad_out=1.0):
    """The whole loss on numpy arrays: probas (B, C, H, W) fp32, labels (B, H, W) int.  Returns a dict: loss (double),
    n_kept (weights included, summed over images) and grad (d loss / d probas, fp32, for the upstream gradient grad_out)."""
    B, C, H, W = probas.shape
    HW = H * W
    weights, present_only = class_weights(classes, C)
    P = np.ascontiguousarray(probas.transpose(1, 0, 2, 3)).reshape(C, B * HW)
    lab = labels.reshape(-1)
    valid = np.ones(lab.shape, bool) if ignore is None else lab != ignore
    grad = np.zeros((C, B * HW), np.float32)
    spans = [slice(b * HW, (b + 1) * HW) for b in range(B)] if per_image else [slice(0, B * HW)]
    total, n_kept = 0.0, 0
    for sp in spans:
        v = valid[sp]
        mult = np.zeros(C, np.int64)
        seg_loss, seg_d = np.zeros(C), {}
        for c in range(C):
            if weights[c] == 0:
                continue
            seg_loss[c], gts, seg_d[c] = lovasz_segment(P[c, sp], lab[sp] == c, v)
            if v.any() and not (present_only and gts == 0):
                mult[c] = weights[c]
        den = int(mult.sum())
        n_kept += den
        if den == 0:
            continue
        total += float((mult * seg_loss).sum()) / den
        t = np.float32(grad_out)
        if per_image:
            t = t / np.float32(B)
        fac = t / np.float32(den)
        for c in range(C):
            if mult[c]:
                grad[c, sp] = np.float32(mult[c]) * (fac * seg_d[c])
    grad = np.ascontiguousarray(grad.reshape(C, B, H, W).transpose(1, 0, 2, 3))
    return {"loss": total / len(spans), "n_kept": n_kept, "grad": grad}


# ---- tie-aware comparison ----
def group_keys(probas, labels, per_image=False, ignore=None):
    """For every element of the (B, C, H, W) gradient: the key of its (segment, class, equal-error) group as uint64
    (segment << 40 | class << 32 | bits(e); NO_GROUP where the pixel is not valid) and sigma = -sign(fg - p)."""
    B, C, H, W = probas.shape
    c = np.arange(C, dtype=np.int64)[None, :, None, None]
    fg = labels[:, None] == c
    d = fg.astype(np.float32) - probas
    ebits = np.abs(d).view(np.uint32).astype(np.uint64)
    seg = (np.arange(B, dtype=np.uint64) if per_image else np.zeros(B, np.uint64))[:, None, None, None]
    keys = (seg << np.uint64(40)) | (c.astype(np.uint64) << np.uint64(32)) | ebits
    valid = np.ones(labels.shape, bool) if ignore is None else labels != ignore
    keys = np.where(np.broadcast_to(valid[:, None], keys.shape), keys, NO_GROUP)
    sigma = np.where(d < 0, 1, np.where(d > 0, -1, 0)).astype(np.float32)
    return keys.ravel(), sigma.ravel()


def group_sums(grad, keys, sigma):
    """(group keys, sum of grad * sigma per group in double, group sizes, size of every element's group; 1 off groups)."""
    on = keys != NO_GROUP
    uniq, inv, counts = np.unique(keys[on], return_inverse=True, return_counts=True)
    sums = np.bincount(inv, weights=(grad.ravel()[on] * sigma[on]).astype(np.float64), minlength=len(uniq))
    size = np.ones(keys.shape, np.int64)
    size[on] = counts[inv]
    return uniq, sums, counts, size


def fixture_record(probas, labels, grad, per_image, ignore, seed):
    """What a fixture stores of a reference gradient: max|grad|, an element sample (all elements when small) and the
    gradient sum of a sample of the groups of two or more equal errors."""
    keys, sigma = group_keys(probas, labels, per_image, ignore)
    uniq, sums, counts, _ = group_sums(grad, keys, sigma)
    rng = np.random.default_rng(seed)
    if grad.size <= FULL_GRAD_MAX:
        idx = np.arange(grad.size, dtype=np.int64)
    else:
        idx = np.sort(rng.choice(grad.size, GRAD_SAMPLE, replace=False)).astype(np.int64)
    multi = np.nonzero(counts > 1)[0]
    if len(multi) > GROUP_SAMPLE:
        multi = np.sort(rng.choice(multi, GROUP_SAMPLE, replace=False))
    return {"grad_absmax": np.array(np.abs(grad).max(), np.float64), "grad_index": idx, "grad_sample": grad.ravel()[idx],
            "group_key": uniq[multi], "group_sum": sums[multi], "group_size": counts[multi].astype(np.int64),
            "n_groups_multi": np.array(int((counts > 1).sum()))}


def check_gradient(fx, grad, gtol):
    """Tie-aware gradient bar against a fixture: sampled pixels with a unique error elementwise, sampled groups of equal
    errors by their sum, both within gtol x max|grad|.  Returns (singletons compared, groups compared)."""
    keys, sigma = group_keys(fx["probas"], fx["labels"], fx["args"]["per_image"], fx["args"]["ignore"])
    uniq, sums, counts, size = group_sums(grad, keys, sigma)
    scale = float(fx["grad_absmax"])
    idx = fx["grad_index"]
    single = size[idx] == 1
    err = np.abs(grad.ravel()[idx][single].astype(np.float64) - fx["grad_sample"][single])
    assert err.max(initial=0.0) <= gtol * scale, (float(err.max()), scale)
    pos = np.searchsorted(uniq, fx["group_key"])
    assert np.all(pos < len(uniq)) and np.array_equal(uniq[np.minimum(pos, len(uniq) - 1)], fx["group_key"])
    assert np.array_equal(counts[pos], fx["group_size"])
    gerr = np.abs(sums[pos] - fx["group_sum"])
    assert gerr.max(initial=0.0) <= gtol * scale, (float(gerr.max()), scale)
    return int(single.sum()), len(pos)


# ---- fixtures (tests/golden/lovasz_*.npz, written by tests/golden/make_lovasz_golden.py from the reference) ----
def _classes_arg(fx):
    mode = str(fx["classes"])
    return [int(c) for c in fx["class_list"]] if mode == "list" else mode


def load_fixture(path):
    """A fixture with its inputs regenerated from the stored seed."""
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    B, C, H, W = (int(v) for v in fx["shape"])
    absent = int(fx["absent"])
    fx["probas"], fx["labels"] = make_case_inputs(B, C, H, W, int(fx["seed"]), ignore_frac=float(fx["ignore_frac"]),
                                                  extra_frac=float(fx["extra_frac"]), absent=None if absent < 0 else absent)
    ignore = int(fx["ignore"])
    fx["args"] = dict(classes=_classes_arg(fx), per_image=bool(fx["per_image"]), ignore=None if ignore < 0 else ignore)
    return fx


def check_against_fixture(fx, loss, grad, rtol=1e-6, gtol=1e-6):
    """Loss within rtol relative (absolute when the reference loss is 0), gradient tie-aware within gtol x max|grad|."""
    ref = float(fx["loss"])
    assert abs(float(loss) - ref) <= rtol * max(abs(ref), 1e-30) or (ref == 0 and float(loss) == 0), (float(loss), ref)
    return check_gradient(fx, grad, gtol)


def make_criterion_inputs(seed):
    """The CriterionOhemDSN2 fixture's inputs: (1, 19, 97, 97) main and DSN logits, (1, 769, 769) labels, 5 % ignored."""
    rng = np.random.default_rng(seed)
    main = (rng.standard_normal((1, 19, 97, 97)) * 3).astype(np.float32)
    aux = (rng.standard_normal((1, 19, 97, 97)) * 3).astype(np.float32)
    target = rng.integers(0, 19, (1, 769, 769)).astype(np.int64)
    target[rng.random((1, 769, 769)) < 0.05] = 255
    return main, aux, target


def ulp_distance(a, b):
    """Elementwise distance in fp32 units in the last place."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
