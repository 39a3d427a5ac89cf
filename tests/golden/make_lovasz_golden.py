#!/usr/bin/env python3
"""Generate the Lovász-softmax fixtures (tests/golden/lovasz_*.npz) from the LIVE reference loss.

Runs only where the upstream tree is checked out.  It imports the unmodified ``loss/lovasz_losses.py`` (``lovasz_softmax``,
lovasz_losses.py:153-218) and, for one case, ``loss/criterion.py`` (``CriterionOhemDSN2``, criterion.py:59-78); both run on
the CPU.  Loss and gradient come from the reference's forward and torch autograd.

Inputs are regenerated from the seed stored in every fixture (tests/lovasz_oracle.make_case_inputs,
make_criterion_inputs).  Because the reference's sort leaves the order of equal errors unspecified, a fixture keeps the
gradient in the form the tie-aware bar reads (tests/lovasz_oracle.fixture_record): max|grad|, a seeded element sample (all
elements when small) and the gradient sums of a seeded sample of equal-error groups.

    python tests/golden/make_lovasz_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lovasz_oracle as O  # noqa: E402

# name: (B, C, H, W, seed, classes, per_image, ignore, ignore_frac, extra_frac, absent)
CASES = {
    "lovasz_2x19x65x97_present": (2, 19, 65, 97, 1, "present", False, 255, 0.05, 0.0, -1),
    "lovasz_2x19x97x97_per_image": (2, 19, 97, 97, 2, "present", True, 255, 0.05, 0.0, -1),
    "lovasz_1x19x64x64_all_absent": (1, 19, 64, 64, 3, "all", False, 255, 0.05, 0.0, 7),
    "lovasz_1x19x60x70_list_dup": (1, 19, 60, 70, 4, [1, 3, 3, 18, 7], False, 255, 0.05, 0.0, 7),
    "lovasz_1x19x48x48_ignore_none": (1, 19, 48, 48, 5, "present", False, -1, 0.05, 0.0, -1),
    "lovasz_1x19x50x80_extra_labels": (1, 19, 50, 80, 6, "present", False, 255, 0.05, 0.1, -1),
    "lovasz_1x150x40x40_c150": (1, 150, 40, 40, 7, "present", False, 255, 0.05, 0.0, -1),
    "lovasz_2x19x33x129_nonsquare": (2, 19, 33, 129, 8, "present", True, 255, 0.05, 0.0, -1),
    "lovasz_1x19x769x769_recipe": (1, 19, 769, 769, 9, "present", False, 255, 0.05, 0.0, -1),
}
CRITERION_SEED = 21


def load_reference():
    sys.path.insert(0, REF)
    return importlib.import_module("loss.lovasz_losses"), importlib.import_module("loss.criterion")


def run_case(lov, B, C, H, W, seed, classes, per_image, ignore, ignore_frac, extra_frac, absent):
    probas, labels = O.make_case_inputs(B, C, H, W, seed, ignore_frac=ignore_frac, extra_frac=extra_frac,
                                        absent=None if absent < 0 else absent)
    x = torch.from_numpy(probas).requires_grad_(True)
    loss = lov.lovasz_softmax(x, torch.from_numpy(labels), classes=classes, per_image=per_image,
                              ignore=None if ignore < 0 else ignore)
    loss.backward()
    return probas, labels, float(loss.detach()), x.grad.numpy()


def main():
    lov, crit = load_reference()
    for name, (B, C, H, W, seed, classes, per_image, ignore, ifrac, efrac, absent) in CASES.items():
        probas, labels, loss, grad = run_case(lov, B, C, H, W, seed, classes, per_image, ignore, ifrac, efrac, absent)
        mode = classes if isinstance(classes, str) else "list"
        out = {"shape": np.array([B, C, H, W]), "seed": np.array(seed), "classes": np.array(mode),
               "class_list": np.array(classes if mode == "list" else [], np.int64), "per_image": np.array(per_image),
               "ignore": np.array(ignore), "ignore_frac": np.array(ifrac), "extra_frac": np.array(efrac),
               "absent": np.array(absent), "loss": np.array(loss, np.float64)}
        out.update(O.fixture_record(probas, labels, grad, per_image, None if ignore < 0 else ignore, seed))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(f"{name}: loss {loss:.8g}, groups of equal errors {int(out['n_groups_multi'])}", flush=True)

    # CriterionOhemDSN2: CE + Lovász-softmax of the up-sampled main logits (the DSN logits are unused)
    main_l, aux_l, target = O.make_criterion_inputs(CRITERION_SEED)
    xm = torch.from_numpy(main_l).requires_grad_(True)
    xa = torch.from_numpy(aux_l).requires_grad_(True)
    loss = crit.CriterionOhemDSN2(ignore_index=255)([xm, xa], torch.from_numpy(target))
    loss.backward()
    grad = xm.grad.numpy()
    idx = np.sort(np.random.default_rng(CRITERION_SEED).choice(grad.size, O.GRAD_SAMPLE, replace=False)).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "lovasz_criterion_1x19x97x97_769.npz"), seed=np.array(CRITERION_SEED),
                        loss=np.array(float(loss.detach()), np.float64), grad_absmax=np.array(np.abs(grad).max(), np.float64),
                        grad_index=idx, grad_sample=grad.ravel()[idx], aux_grad_is_none=np.array(xa.grad is None))
    print(f"criterion: loss {float(loss.detach()):.8g}", flush=True)


if __name__ == "__main__":
    main()
