#!/usr/bin/env python3
"""Generate the DSN cross-entropy fixtures (tests/golden/dsn_*.npz) from the LIVE reference criterion.

Runs only where the upstream tree is checked out (needs /root/reference and scipy, which its loss package imports).  It
imports the unmodified ``loss/criterion.py`` and runs ``CriterionDSN`` (criterion.py:11-35) on the CPU twice per case: on
float64 copies of the inputs (the truth the fixtures store) and on the fp32 inputs (the reference's own arithmetic error,
stored beside it).  The bar of tests/dsn_oracle.py must leave that error at least 4x headroom, or the generator stops.

Inputs are regenerated from the seed stored in every fixture (tests/dsn_oracle.make_case_inputs); gradients of large cases
are stored as a seeded sample of their elements.

    python tests/golden/make_dsn_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dsn_oracle import CASES, GRAD_RTOL, LOSS_RTOL, fixture_path, make_case_inputs  # noqa: E402

FULL_GRAD_MAX = 1 << 16          # store the whole gradient up to this many elements, else GRAD_SAMPLE of them
GRAD_SAMPLE = 8192


def load_reference():
    sys.path.insert(0, REF)
    return importlib.import_module("loss.criterion")


def run_reference(ref, logits, target, dtype):
    crit = ref.CriterionDSN(ignore_index=255)
    xs = [torch.from_numpy(l).to(dtype).requires_grad_(True) for l in logits]
    loss = crit(xs, torch.from_numpy(target))
    loss.backward()
    return float(loss.detach()), [x.grad.numpy() for x in xs]


def main():
    ref = load_reference()
    for name, (B, C, h, w, H, W, seed, heads, scale, all_ignored) in CASES.items():
        logits, target = make_case_inputs(B, C, h, w, H, W, seed, heads, scale, all_ignored)
        loss64, grads64 = run_reference(ref, logits, target, torch.float64)
        loss32, grads32 = run_reference(ref, logits, target, torch.float32)
        valid = int((target != 255).sum())
        out = {"shape": np.array([B, C, h, w, H, W]), "seed": np.array(seed), "heads": np.array(heads),
               "scale": np.array(scale), "all_ignored": np.array(all_ignored), "valid": np.array(valid),
               "loss": np.array(loss64, np.float64)}
        if valid == 0:
            assert np.isnan(loss64) and np.isnan(loss32) and not any(g.any() for g in grads64 + grads32), name
            loss_err = 0.0
        else:
            loss_err = abs(loss32 - loss64) / abs(loss64)
        assert loss_err <= LOSS_RTOL / 4, (name, loss_err)
        grad_errs = []
        for k, (g64, g32) in enumerate(zip(grads64, grads32)):
            top = float(np.abs(g64).max())
            err = float(np.abs(g32.astype(np.float64) - g64).max()) / top if top else 0.0
            assert err <= GRAD_RTOL / 4, (name, k, err)
            grad_errs.append(err)
            out[f"grad{k}_max"] = np.array(top, np.float64)
            if g64.size <= FULL_GRAD_MAX:
                out[f"grad{k}"] = g64
            else:
                idx = np.sort(np.random.default_rng(seed + k).choice(g64.size, GRAD_SAMPLE, replace=False))
                out[f"grad{k}_index"] = idx.astype(np.int64)
                out[f"grad{k}_sample"] = g64.ravel()[idx]
        out["fp32_loss_rel_err"] = np.array(loss_err, np.float64)
        out["fp32_grad_rel_err"] = np.array(grad_errs, np.float64)
        np.savez_compressed(fixture_path(name), **out)
        print(f"{name}: valid {valid} loss {loss64:.9g} | fp32 reference: loss rel err {loss_err:.2e}, "
              f"grad err / max|grad| {max(grad_errs):.2e}", flush=True)


if __name__ == "__main__":
    main()
