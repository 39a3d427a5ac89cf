#!/usr/bin/env python3
"""Generate the evaluation fixtures (tests/golden/eval_*.npz) from the LIVE reference evaluate.py.

Runs only where the upstream tree is checked out.  It imports the unmodified ``evaluate.py`` after stubbing the modules it
needs only for ``main()`` or that are not installed here (cv2, torchvision, networks, dataset.datasets, engine,
utils.pyt_utils), and patches only ``torch.Tensor.cuda`` so the reference runs on the CPU.  It then calls the reference's
own ``predict_sliding`` / ``predict_whole`` with a seeded toy net (tests/eval_oracle.make_toy_net: stride 8, returns a
list), main()'s argmax and ignore mask, and ``get_confusion_matrix``.

Inputs are regenerated from the seed stored in every fixture; the prediction is stored in full (uint8), the confusion
matrix in full, and the (N, C, H, W) score map as a seeded sample of its elements.

    python tests/golden/make_eval_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from eval_oracle import make_case_inputs, make_toy_net  # noqa: E402

SAMPLE = 8192

# name: (H, W, tile, C, whole, seed)
CASES = {
    "eval_1024x2048_t769_c19_recipe": (1024, 2048, 769, 19, False, 1),
    "eval_128x256_t97_c19_multi": (128, 256, 97, 19, False, 2),
    "eval_60x80_t97_c19_padded": (60, 80, 97, 19, False, 3),
    "eval_300x160_t97_c19_portrait": (300, 160, 97, 19, False, 4),
    "eval_128x256_c19_whole": (128, 256, 0, 19, True, 5),
    "eval_200x300_t97_c150": (200, 300, 97, 150, False, 6),
}


def load_reference():
    for name in ("cv2", "torchvision", "torchvision.models", "networks", "dataset", "dataset.datasets", "engine", "utils",
                 "utils.pyt_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["dataset.datasets"].CSDataSet = None
    sys.modules["utils.pyt_utils"].load_model = None
    sys.modules["engine"].Engine = None
    spec = importlib.util.spec_from_file_location("ref_evaluate", os.path.join(REF, "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # evaluate.py:130, 149: keep the tiles on the CPU
    try:
        for name, (H, W, tile, C, whole, seed) in CASES.items():
            image, label = make_case_inputs(1, H, W, C, seed)
            net = make_toy_net(C, seed)
            with torch.no_grad():
                if whole:
                    probs = ref.predict_whole(net, image, (H, W), 0)
                else:
                    probs = ref.predict_sliding(net, image, (tile, tile), C, 0)
            seg_pred = np.asarray(np.argmax(probs, axis=3), dtype=np.uint8)          # main(), evaluate.py:250-251
            seg_gt = np.asarray(label, dtype=np.int64)
            keep = seg_gt != 255
            cm = ref.get_confusion_matrix(seg_gt[keep], seg_pred[keep], C)
            assert (label == 255).any() and np.isfinite(probs).all()
            nchw = np.ascontiguousarray(probs.transpose(0, 3, 1, 2))
            idx = np.sort(np.random.default_rng(seed).choice(nchw.size, min(SAMPLE, nchw.size), replace=False))
            np.savez_compressed(os.path.join(HERE, name + ".npz"), H=np.array(H), W=np.array(W), tile=np.array([tile, tile]),
                                C=np.array(C), whole=np.array(whole), seed=np.array(seed), pred=seg_pred,
                                confusion=cm.astype(np.int64), probs_index=idx.astype(np.int64),
                                probs_sample=nchw.ravel()[idx], max_abs_logit=np.array(np.abs(nchw).max()))
            print(f"{name}: pixels counted {int(cm.sum())}, mIoU {np.nanmean(np.diag(cm) / np.maximum(1, cm.sum(0) + cm.sum(1) - np.diag(cm))):.4f}", flush=True)
    finally:
        torch.Tensor.cuda = orig_cuda


if __name__ == "__main__":
    main()
