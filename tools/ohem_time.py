#!/usr/bin/env python3
"""Time the OHEM cross-entropy, forward + backward, at (B, 19, 769, 769): the device criterion (ccnet_amd.ohem, libccnet_ohem.so)
against the reference's host path (loss/loss.py:51-93: softmax, D2H copy, zoom + np.partition on the host, new int64 target
H2D, stock cross-entropy).  Prints one JSON line.

    python tools/ohem_time.py [--batches 1 2 8] [--iters 10] [--warmup 3]

The host side zooms with scipy.ndimage.zoom when scipy is installed, else with the numpy restatement in tests/ohem_oracle.py
(bit-identical to scipy; the line says which).  Times are host wall clock around work that ends in a device synchronise.
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

import ohem_oracle as O  # noqa: E402

try:
    import scipy.ndimage as nd
except ImportError:
    nd = None

THRESH, MIN_KEPT, FACTOR, IGNORE = 0.6, 200000, 8, 255


def host_threshold(np_predict, np_target):
    """loss.py:20-48"""
    if nd is not None:
        predict = nd.zoom(np_predict, (1.0, 1.0, 1.0 / FACTOR, 1.0 / FACTOR), order=1)
        target = nd.zoom(np_target, (1.0, 1.0 / FACTOR, 1.0 / FACTOR), order=0)
    else:
        predict, target = O.zoom_order1(np_predict, FACTOR), O.zoom_order0(np_target, FACTOR)
    c = predict.shape[1]
    min_kept = MIN_KEPT // (FACTOR * FACTOR)
    label = target.ravel().astype(np.int32)
    prob = np.rollaxis(predict, 1).reshape((c, -1))
    valid = label != IGNORE
    num_valid = valid.sum()
    if min_kept >= num_valid:
        return 1.0
    pred = prob[:, valid][label[valid], np.arange(num_valid)]
    threshold = THRESH
    if min_kept > 0:
        k = min(len(pred), min_kept) - 1
        kth = np.partition(pred, k)[k]
        threshold = max(threshold, kth)
    return threshold


def host_step(x, t):
    """The reference's forward (loss.py:51-93) + backward."""
    prob = F.softmax(x, 1)
    np_predict, np_target = prob.detach().cpu().numpy(), t.cpu().numpy()
    threshold = host_threshold(np_predict, np_target)
    c = np_predict.shape[1]
    label = np_target.ravel().astype(np.int32)
    p = np.rollaxis(np_predict, 1).reshape((c, -1))
    valid_inds = np.where(label != IGNORE)[0]
    pred = p[label[valid_inds], valid_inds]
    valid_inds = valid_inds[pred <= threshold]
    new = np.full_like(label, IGNORE)
    new[valid_inds] = label[valid_inds]
    new_t = torch.from_numpy(new.reshape(np_target.shape)).long().to(x.device)
    loss = F.cross_entropy(x, new_t, ignore_index=IGNORE)
    loss.backward()
    return loss


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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ohem_time.py measures on a HIP device; none found")
    from ccnet_amd.ohem import OhemCrossEntropy2d
    dev = torch.device("cuda:0")
    crit = OhemCrossEntropy2d(IGNORE, THRESH, MIN_KEPT, FACTOR)
    rows = []
    for B in args.batches:
        logits, target = O.make_case_inputs(B, 19, 769, 769, seed=B)
        x = torch.from_numpy(logits).to(dev).requires_grad_(True)
        t = torch.from_numpy(target).to(dev)

        def device_step():
            x.grad = None
            crit(x, t).backward()

        def reference_step():
            x.grad = None
            host_step(x, t)

        dev_ms = time_it(device_step, args.iters, args.warmup)
        host_ms = time_it(reference_step, max(args.iters // 2, 1), 1)
        rows.append({"B": B, "device_ms": round(dev_ms, 3), "host_path_ms": round(host_ms, 2),
                     "speedup": round(host_ms / dev_ms, 1), "logits_MB": round(logits.nbytes / 1e6, 1)})
        del x, t
    print(json.dumps({"metric": "OHEM cross-entropy forward+backward at (B,19,769,769), thresh 0.6, min_kept 200000",
                      "unit": "ms per call", "host_zoom": "scipy" if nd is not None else "numpy restatement",
                      "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
