#!/usr/bin/env python3
"""Time the evaluation post-processing of one 1024 x 2048 image with 19 classes and the reference's 8 tiles of 769^2, from
synthetic (8, 19, 97, 97) tile logits (the net is out of the picture): the device kernel (ccnet_amd.evaluate,
libccnet_eval.so: score, argmax and confusion counts in one launch) against the reference-style host path (evaluate.py:
up-sample each tile on the device, copy it to the host, float64 NHWC accumulation, division, np.argmax, np.bincount; the
numpy restatement in tests/eval_oracle.host_path).  Prints one JSON line.

    python tools/eval_time.py [--iters 50] [--warmup 5] [--host-iters 3]

Times are host wall clock around work that ends in a device synchronise, after warm-up.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_oracle as O  # noqa: E402

H, W, TILE, C = 1024, 2048, (769, 769), 19


def time_it(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py measures on a HIP device; none found")
    from ccnet_amd.evaluate import sliding_call, tile_grid
    dev = torch.device("cuda:0")
    origins = tile_grid(H, W, TILE)
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.standard_normal((len(origins), C, 97, 97)) * 3).astype(np.float32)).to(dev)
    _, label_np = O.make_case_inputs(1, H, W, C, seed=0)
    label = torch.from_numpy(label_np).to(dev)
    pred = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
    probs = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
    conf = torch.zeros((C, C), dtype=torch.int64, device=dev)

    def device_pred_confusion():
        sliding_call(logits, origins, False, 1, TILE, H, W, labels=label, pred=pred, confusion=conf)

    def device_with_scores():
        sliding_call(logits, origins, False, 1, TILE, H, W, labels=label, probs=probs, pred=pred, confusion=conf)

    def host_path():
        up = lambda t: F.interpolate(logits[t:t + 1], size=TILE, mode="bilinear", align_corners=True).cpu().numpy()  # noqa: E731
        return O.host_path(up, origins, TILE, H, W, C, label.cpu().numpy())

    dev_ms = time_it(device_pred_confusion, args.iters, args.warmup)
    dev_probs_ms = time_it(device_with_scores, args.iters, args.warmup)
    host_ms = time_it(host_path, args.host_iters, 1)

    # the two routes agree on this input (pred ties aside; both count their own prediction)
    conf.zero_()
    device_pred_confusion()
    host_pred, host_cm = host_path()
    same = float((pred.cpu().numpy() == host_pred).mean())
    print(json.dumps({"metric": "evaluation post-processing of one 1024x2048 image, 8 tiles of 769^2, 19 classes "
                                "(score, argmax, confusion)", "unit": "ms per image",
                      "device_ms": round(dev_ms, 4), "device_with_score_map_ms": round(dev_probs_ms, 4),
                      "host_path_ms": round(host_ms, 1), "speedup": round(host_ms / dev_ms, 1),
                      "pred_agreement": same, "confusion_equal": bool(np.array_equal(conf.cpu().numpy(), host_cm)),
                      "tile_logits_MB": round(logits.numel() * 4 / 1e6, 2),
                      "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
