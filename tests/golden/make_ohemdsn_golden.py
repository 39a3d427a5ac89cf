#!/usr/bin/env python3
"""Generate the fixtures of the fused OHEM + DSN criterion (tests/golden/ohemdsn_*.npz) from the LIVE reference criterion.

Runs only where the upstream tree is checked out (needs /root/reference and scipy, which its loss package imports).  It
imports the unmodified ``loss/criterion.py`` (``CriterionOhemDSN``, criterion.py:37-56) and patches only ``torch.Tensor.cuda``
(loss.py:76 moves the new target to the GPU) so the criterion runs on the CPU.  Every case runs twice: in fp32 -- the
reference's own run, whose threshold and new target the fixture stores -- and on float64 copies of the logits, whose loss,
head cross-entropies and gradients the fixture stores.  Beside them go three gaps of the reference against itself:
|threshold32 - threshold64|, max|p_target32 - p_target64| over the valid pixels, and the fp32 run's loss and gradient
error against the float64 run.  The generator asserts, per case: the branch the case claims, identical kept masks in the
two runs, at most MAX_NEAR valid pixels within 2 * NEAR of the threshold, and the fp32 run's own error at least 4x below
the bars of tests/ohemdsn_oracle.py.  It prints the window NEAR = 2 x the largest p_target gap, which ohemdsn_oracle.py
stores as a constant (run it again after changing that constant).

    python tests/golden/make_ohemdsn_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ohemdsn_oracle as D  # noqa: E402

FULL_GRAD_MAX = 1 << 16          # store the whole gradient up to this many elements, else GRAD_SAMPLE of them
GRAD_SAMPLE = 8192
SEED_TRIES = 8


def load_reference():
    sys.path.insert(0, REF)
    return importlib.import_module("loss.criterion")


def run_reference(ref, logits, target, thresh, min_kept, dtype):
    """(threshold, new target, p_target per pixel, loss, [CE per head], [gradient per head]) of one run of the reference"""
    crit = ref.CriterionOhemDSN(ignore_index=255, thresh=thresh, min_kept=min_kept)
    ohem, seen = crit.criterion1, {}
    find, gen = ohem.find_threshold, ohem.generate_new_target

    def capture_threshold(np_predict, np_target):
        seen["threshold"] = find(np_predict, np_target)
        return seen["threshold"]

    def capture_target(predict, tgt):
        seen["prob"] = predict.detach().numpy()
        seen["new_target"] = gen(predict, tgt)
        return seen["new_target"]

    ohem.find_threshold, ohem.generate_new_target = capture_threshold, capture_target
    heads = {}
    for k, c in enumerate((crit.criterion1, crit.criterion2)):
        c.register_forward_hook(lambda m, a, out, k=k: heads.__setitem__(k, float(out.detach())))
    xs = [torch.from_numpy(l).to(dtype).requires_grad_(True) for l in logits]
    t = torch.from_numpy(target)
    preds = xs if len(xs) == 2 else [xs[0], xs[0].detach()]          # (the reference indexes preds[1]; one head: CE_0 alone)
    loss = crit(preds, t)
    if len(xs) == 1:
        loss = loss - heads[1] * 0.4
    loss.backward()
    pt, _ = D.O.target_prob(seen["prob"], target)
    return (seen["threshold"], seen["new_target"].numpy(), pt, float(loss.detach()), [heads[k] for k in range(len(xs))],
            [x.grad.numpy() for x in xs])


class AnotherSeed(Exception):
    pass


def make_case(ref, name, case):
    """Run one case at one seed and write its fixture; returns its p_target gap.  AnotherSeed: the seed does not meet the
    conditions the window needs (identical masks in both runs, at most MAX_NEAR pixels inside the window)."""
    B, C, h, w, H, W, seed, heads, scale, all_ignored, thresh, min_kept, want = case
    logits, target = D.make_case_inputs(B, C, h, w, H, W, seed, heads, scale, all_ignored)
    thr32, new32, pt32, loss32, ce32, g32 = run_reference(ref, logits, target, thresh, min_kept, torch.float32)
    thr64, new64, pt64, loss64, ce64, g64 = run_reference(ref, logits, target, thresh, min_kept, torch.float64)
    valid = target != 255
    kept = int((new32 != 255).sum())
    check = {"kth_above": thr32 > thresh, "kth_below": thr32 == thresh and min_kept // 64 > 0, "one": thr32 == 1.0,
             "thresh": thr32 == thresh and min_kept // 64 == 0, "none_kept": kept == 0, "recipe": True, "any": True}[want]
    assert check, (name, thr32, kept)
    if not np.array_equal(new32, new64):
        raise AnotherSeed(f"the fp32 and the float64 run keep different pixels ({int((new32 != new64).sum())})")
    p_gap = float(np.abs(pt32.astype(np.float64) - pt64)[valid].max()) if valid.any() else 0.0
    thr_gap = abs(float(np.float32(thr32)) - float(thr64))
    close = int((np.abs(pt32.astype(np.float64) - float(np.float32(thr32))) <= 2 * D.NEAR)[valid].sum()) if thr32 < 1.0 else 0
    if close > D.MAX_NEAR:
        raise AnotherSeed(f"{close} valid pixels inside the window")
    assert thr_gap <= D.NEAR, (name, thr_gap)
    out = {"shape": np.array([B, C, h, w, H, W]), "seed": np.array(seed), "heads": np.array(heads),
           "scale": np.array(scale), "all_ignored": np.array(all_ignored), "thresh": np.array(thresh),
           "min_kept": np.array(min_kept), "threshold": np.array(thr32, np.float32),
           "new_target": new32.astype(np.uint8), "valid": np.array(int(valid.sum())),
           "num_valid_zoomed": np.array(int((D.O.zoom_order0(target, 8) != 255).sum())),
           "loss": np.array(loss64, np.float64), "head_loss": np.array(ce64, np.float64),
           "threshold_gap": np.array(thr_gap), "p_target_gap": np.array(p_gap), "pixels_in_window": np.array(close)}
    if kept == 0:
        assert np.isnan(loss64) and np.isnan(loss32) and not g64[0].any() and not g32[0].any(), name
        loss_err = 0.0
    else:
        loss_err = max([abs(loss32 - loss64) / abs(loss64)] + [abs(a - b) / abs(b) for a, b in zip(ce32, ce64)])
    assert loss_err <= D.LOSS_RTOL / 4, (name, loss_err)
    grad_errs = []
    for k, (a64, a32) in enumerate(zip(g64, g32)):
        top = float(np.abs(a64).max())
        err = float(np.abs(a32.astype(np.float64) - a64).max()) / top if top else 0.0
        assert err <= D.GRAD_RTOL / 4, (name, k, err)
        grad_errs.append(err)
        out[f"grad{k}_max"] = np.array(top, np.float64)
        if a64.size <= FULL_GRAD_MAX:
            out[f"grad{k}"] = a64
        else:
            idx = np.sort(np.random.default_rng(seed + k).choice(a64.size, GRAD_SAMPLE, replace=False))
            out[f"grad{k}_index"] = idx.astype(np.int64)
            out[f"grad{k}_sample"] = a64.ravel()[idx]
    out["fp32_loss_rel_err"] = np.array(loss_err, np.float64)
    out["fp32_grad_rel_err"] = np.array(grad_errs, np.float64)
    np.savez_compressed(D.fixture_path(name), **out)
    print(f"{name}: threshold {thr32:.9g} (gap to float64 {thr_gap:.2e}) kept {kept} of {int(valid.sum())} valid, "
          f"{close} within the window | p_target gap {p_gap:.2e} | loss {loss64:.9g} | fp32 reference: loss rel err "
          f"{loss_err:.2e}, grad err / max|grad| {max(grad_errs):.2e}", flush=True)
    return p_gap


def main():
    ref = load_reference()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # loss.py:76: keep the new target on the CPU
    worst_gap = 0.0
    try:
        for name, case in D.CASES.items():
            if name in D.ORACLE_ONLY:
                continue
            for attempt in range(SEED_TRIES):               # the case's own seed first, then seed + 100, + 200, ...
                try:
                    worst_gap = max(worst_gap, make_case(ref, name, case[:6] + (case[6] + 100 * attempt,) + case[7:]))
                    break
                except AnotherSeed as why:
                    print(f"{name}: seed {case[6] + 100 * attempt} refused: {why}", flush=True)
            else:
                raise SystemExit(f"{name}: no seed of {SEED_TRIES} meets the case's conditions")
    finally:
        torch.Tensor.cuda = orig_cuda
    print(f"largest p_target gap {worst_gap!r}: near = {2 * worst_gap!r} (ohemdsn_oracle.MEASURED_P_GAP is {D.MEASURED_P_GAP!r})")
    assert worst_gap <= D.MEASURED_P_GAP, "raise ohemdsn_oracle.MEASURED_P_GAP to the printed gap and run again"


if __name__ == "__main__":
    main()
