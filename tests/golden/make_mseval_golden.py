#!/usr/bin/env python3
"""Generate the multi-scale evaluation fixtures (tests/golden/mseval_*.npz) from the LIVE reference evaluate.py and scipy.

Runs only where the upstream tree is checked out and scipy is installed.  It imports the unmodified ``evaluate.py`` the way
make_eval_golden.py does (stubbed side modules, ``torch.Tensor.cuda`` patched so the reference runs on the CPU).  One case calls
the reference's own ``predict_multiscale`` with scales [1.0], the only list it can run.  The others do what it does per scale
(``ndimage.zoom(order=1, prefilter=False)`` of the image, the reference's ``predict_sliding`` / ``predict_whole`` on the scaled
image and on its mirrored copy, 0.5 * (plain + flipped)) with the flipped pass un-flipped along W, then the step the reference
lacks: ``ndimage.zoom`` of the per-scale map by (H / Hs, W / Ws) back to the image, and the mean over the scales.

Inputs are regenerated from the seed stored in every fixture (tests/eval_oracle.make_case_inputs, make_toy_net; N = 1).

    python tests/golden/make_mseval_golden.py
"""
import os
import sys

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from eval_oracle import make_case_inputs, make_toy_net  # noqa: E402
from make_eval_golden import load_reference  # noqa: E402

SAMPLE = 8192

# name: (H, W, tile, C, whole, seed, scales, flip, through the reference's own predict_multiscale)
CASES = {
    "mseval_128x256_t97_c19_seven_flip": (128, 256, 97, 19, False, 11, (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0), True, False),
    "mseval_60x80_t97_c19_small": (60, 80, 97, 19, False, 12, (0.75, 1.0, 1.5), False, False),
    "mseval_300x160_t97_c19_portrait_flip": (300, 160, 97, 19, False, 13, (0.75, 1.25), True, False),
    "mseval_128x256_c19_whole": (128, 256, 0, 19, True, 14, (0.5, 1.0, 1.5), False, False),
    "mseval_128x256_t97_c19_reference_1x": (128, 256, 97, 19, False, 15, (1.0,), False, True),
}


def one_scale(ref, net, image, scale, tile, C, whole, flip):
    """((1, Hs, Ws, C) float64 score of one scale, (Hs, Ws))."""
    scaled = ndimage.zoom(image, (1.0, 1.0, scale, scale), order=1, prefilter=False)          # evaluate.py:166
    Hs, Ws = scaled.shape[2:]
    predict = (lambda im: ref.predict_whole(net, im, (Hs, Ws), 0)) if whole else \
              (lambda im: ref.predict_sliding(net, im, (tile, tile), C, 0))
    probs = np.asarray(predict(scaled), np.float64)
    if flip:
        flipped = np.asarray(predict(scaled[:, :, :, ::-1].copy()), np.float64)
        probs = 0.5 * (probs + flipped[:, :, ::-1, :])                                        # un-flipped along W (NHWC axis 2)
    return probs, (Hs, Ws)


def main():
    ref = load_reference()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for name, (H, W, tile, C, whole, seed, scales, flip, own) in CASES.items():
            image, label = make_case_inputs(1, H, W, C, seed)
            net = make_toy_net(C, seed)
            sizes = []
            with torch.no_grad():
                if own:
                    full = ref.predict_multiscale(net, torch.from_numpy(image), (tile, tile), list(scales), C, False, 0)
                    sizes = [(H, W)]
                else:
                    full = np.zeros((1, H, W, C))
                    for s in scales:
                        probs, (Hs, Ws) = one_scale(ref, net, image, float(s), tile, C, whole, flip)
                        back = ndimage.zoom(probs, (1.0, H / Hs, W / Ws, 1.0), order=1, prefilter=False)
                        assert back.shape == (1, H, W, C), back.shape
                        full += back
                        sizes.append((Hs, Ws))
                    full /= len(scales)
            seg_pred = np.asarray(np.argmax(full, axis=3), dtype=np.uint8)
            seg_gt = np.asarray(label, dtype=np.int64)
            keep = seg_gt != 255
            cm = ref.get_confusion_matrix(seg_gt[keep], seg_pred[keep], C)
            assert (label == 255).any() and np.isfinite(full).all()
            nchw = np.ascontiguousarray(full.transpose(0, 3, 1, 2))
            idx = np.sort(np.random.default_rng(seed).choice(nchw.size, min(SAMPLE, nchw.size), replace=False))
            np.savez_compressed(os.path.join(HERE, name + ".npz"), H=np.array(H), W=np.array(W), tile=np.array([tile, tile]),
                                C=np.array(C), whole=np.array(whole), seed=np.array(seed), scales=np.array(scales, np.float64),
                                flip=np.array(flip), sizes=np.array(sizes, np.int64), pred=seg_pred,
                                confusion=cm.astype(np.int64), probs_index=idx.astype(np.int64),
                                probs_sample=nchw.ravel()[idx], max_abs_logit=np.array(np.abs(nchw).max()))
            print(f"{name}: scaled sizes {sizes}, pixels counted {int(cm.sum())}", flush=True)
    finally:
        torch.Tensor.cuda = orig_cuda


if __name__ == "__main__":
    main()
