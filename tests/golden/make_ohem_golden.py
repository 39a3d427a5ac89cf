#!/usr/bin/env python3
"""Generate the OHEM cross-entropy fixtures (tests/golden/ohem_*.npz) from the LIVE reference criterion.

Runs only where the upstream tree is checked out (needs /root/reference and scipy).  It imports the unmodified
``loss/loss.py`` (``OhemCrossEntropy2d``, loss.py:9-93) and patches only ``torch.Tensor.cuda`` (loss.py:71 moves the
new target to the GPU) so the criterion runs on the CPU.  The threshold is captured by wrapping the instance's own
``find_threshold``; the loss and the gradient of the logits come from the reference's forward and torch autograd.

Inputs are regenerated from the seed stored in every fixture (tests/ohem_oracle.make_case_inputs); the new target is
stored as uint8 (255 = ignored), and gradients of large cases as a seeded sample of their elements.

    python tests/golden/make_ohem_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ohem_oracle import make_case_inputs  # noqa: E402

FULL_GRAD_MAX = 1 << 16          # store the whole gradient up to this many elements, else GRAD_SAMPLE of them
GRAD_SAMPLE = 8192

# name: (B, C, H, W, seed, thresh, min_kept, all_ignored, expectation)
CASES = {
    "ohem_2x19x97x97_kth": (2, 19, 97, 97, 1, 0.3, 64 * 265, False, "kth_above"),
    "ohem_1x19x129x257_hw": (1, 19, 129, 257, 2, 0.7, 20000, False, "kth_below"),
    "ohem_1x19x65x65_keepall": (1, 19, 65, 65, 3, 0.7, 100000, False, "one"),
    "ohem_1x19x65x97_minkept0": (1, 19, 65, 97, 4, 0.7, 63, False, "thresh"),
    "ohem_1x19x33x33_ignored": (1, 19, 33, 33, 5, 0.7, 100000, True, "none_kept"),
    "ohem_2x19x97x97_below": (2, 19, 97, 97, 6, 0.7, 6400, False, "kth_below"),
    "ohem_1x19x769x769_recipe": (1, 19, 769, 769, 7, 0.6, 200000, False, "recipe"),
}


def load_reference():
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "loss", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, B, C, H, W, seed, thresh, min_kept, all_ignored):
    logits, target = make_case_inputs(B, C, H, W, seed, all_ignored=all_ignored)
    crit = ref.OhemCrossEntropy2d(ignore_label=255, thresh=thresh, min_kept=min_kept)
    seen = {}
    find = crit.find_threshold

    def capture(np_predict, np_target):
        seen["threshold"] = find(np_predict, np_target)
        return seen["threshold"]

    crit.find_threshold = capture
    made = {}
    gen = crit.generate_new_target

    def capture_target(predict, tgt):
        made["new_target"] = gen(predict, tgt)
        return made["new_target"]

    crit.generate_new_target = capture_target
    x = torch.from_numpy(logits).requires_grad_(True)
    loss = crit(x, torch.from_numpy(target))
    loss.backward()
    return logits, target, float(seen["threshold"]), made["new_target"].numpy(), float(loss.detach()), x.grad.numpy()


def main():
    ref = load_reference()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # loss.py:71: keep the new target on the CPU
    try:
        for name, (B, C, H, W, seed, thresh, min_kept, all_ignored, want) in CASES.items():
            logits, target, thr, new_target, loss, grad = run_case(ref, B, C, H, W, seed, thresh, min_kept, all_ignored)
            kept = int((new_target != 255).sum())
            check = {"kth_above": thr > thresh, "kth_below": thr == np.float32(thresh) and min_kept // 64 > 0,
                     "one": thr == 1.0, "thresh": thr == thresh and min_kept // 64 == 0,
                     "none_kept": kept == 0, "recipe": True}[want]
            assert check, (name, thr, kept)
            out = {"shape": np.array([B, C, H, W]), "seed": np.array(seed), "thresh": np.array(thresh),
                   "min_kept": np.array(min_kept), "all_ignored": np.array(all_ignored),
                   "threshold": np.array(thr, np.float32), "new_target": new_target.astype(np.uint8),
                   "loss": np.array(loss, np.float64)}
            if grad.size <= FULL_GRAD_MAX:
                out["grad"] = grad
            else:
                idx = np.sort(np.random.default_rng(seed).choice(grad.size, GRAD_SAMPLE, replace=False))
                out["grad_index"] = idx.astype(np.int64)
                out["grad_sample"] = grad.ravel()[idx]
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(f"{name}: threshold {thr:.6g} kept {kept} loss {loss:.6g}", flush=True)
    finally:
        torch.Tensor.cuda = orig_cuda


if __name__ == "__main__":
    main()
