#!/usr/bin/env python3
"""Generate the fixtures of the fused CE + Lovász criterion (tests/golden/celovasz_*.npz) from the LIVE reference criterion.

Runs only where the upstream tree is checked out (its path is the first argument or $CCNET_REFERENCE; its loss package imports
scipy).  It imports the unmodified ``loss/criterion.py`` and runs ``CriterionOhemDSN2`` (criterion.py:59-78) in fp32 on the
CPU: the fixture stores the seed, that run's loss, the gradient of the low-resolution logits (whole up to 2^16 elements, a
seeded sample above that), max|grad|, and for the two terms a stock-op cross-entropy of the same up-sample and the reference's
own ``lovasz_softmax`` of its softmax.

The reference's Lovász term cannot run in float64 (its ``fg`` is ``.float()``), so the generator also runs
``celovasz_oracle.reference`` in float64 -- stock ops in float64, the Lovász term restated with a stable sort -- and records
the fp32 reference's own relative loss error and gradient error / max|grad| against it.  It asserts that both sit at least 4x
below the bars of tests/celovasz_oracle.py, and prints them.

    python tests/golden/make_celovasz_golden.py <path to the reference tree>
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import celovasz_oracle as D  # noqa: E402


def load_reference():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CCNET_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "loss")):
        raise SystemExit(__doc__)
    sys.path.insert(0, ref)
    return importlib.import_module("loss.criterion")


def make_case(ref, name):
    B, C, h, w, H, W, seed, scale, drawn, all_ignored = D.CASES[name]
    logits, target = D.case_inputs(name)
    x = torch.from_numpy(logits).requires_grad_(True)
    t = torch.from_numpy(target)
    loss = ref.CriterionOhemDSN2(ignore_index=D.IGNORE)([x, x.detach()], t)
    loss.backward()
    grad = x.grad.numpy()
    with torch.no_grad():
        up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
        ce = float(F.cross_entropy(up, t, ignore_index=D.IGNORE))
        ls = float(ref.lovasz_softmax(F.softmax(up, dim=1), t, ignore=D.IGNORE))
    r64 = D.reference(logits, target, dtype=torch.float64)
    top = float(np.abs(r64["grad"]).max())
    loss_err = max(D._rel(float(loss.detach()), r64["loss"]), D._rel(ce, r64["head_loss"][0]), D._rel(ls, r64["head_loss"][1]))
    grad_err = float(np.abs(grad.astype(np.float64) - r64["grad"]).max()) / top
    assert loss_err <= D.LOSS_RTOL / 4 and grad_err <= D.GRAD_RTOL / 4, (name, loss_err, grad_err)
    out = {"shape": np.array([B, C, h, w, H, W]), "seed": np.array(seed), "scale": np.array(scale), "drawn": np.array(drawn),
           "all_ignored": np.array(all_ignored), "loss": np.array(float(loss.detach()), np.float64),
           "head_loss": np.array([ce, ls], np.float64), "valid": np.array(r64["valid"]), "n_kept": np.array(r64["n_kept"]),
           "grad_absmax": np.array(float(np.abs(grad).max()), np.float64), "fp32_loss_rel_err": np.array(loss_err),
           "fp32_grad_rel_err": np.array(grad_err)}
    if grad.size <= D.FULL_GRAD_MAX:
        out["grad"] = grad
    else:
        idx = np.sort(np.random.default_rng(seed).choice(grad.size, D.GRAD_SAMPLE, replace=False)).astype(np.int64)
        out["grad_index"], out["grad_sample"] = idx, grad.ravel()[idx]
    np.savez_compressed(D.fixture_path(name), **out)
    print(f"{name}: loss {float(loss.detach()):.9g} = CE {ce:.9g} + LS {ls:.9g}, {r64['valid']} valid, {r64['n_kept']} classes kept | "
          f"fp32 reference against float64: loss rel err {loss_err:.2e}, grad err / max|grad| {grad_err:.2e}", flush=True)
    return loss_err, grad_err


def main():
    ref = load_reference()
    worst = [max(v) for v in zip(*[make_case(ref, name) for name in D.CASES if name not in D.ORACLE_ONLY])]
    print(f"worst fp32 reference error: loss {worst[0]:.2e} (bar {D.LOSS_RTOL:g}), gradient {worst[1]:.2e} of max|grad| "
          f"(bar {D.GRAD_RTOL:g})")


if __name__ == "__main__":
    main()
