#!/usr/bin/env python3
"""Time the Lovász-softmax loss, forward + backward, at (B, 19, 769, 769): the device loss (ccnet_amd.lovasz,
libccnet_lovasz.so) against a stock-op path shaped like the reference's (loss/lovasz_losses.py:153-218: boolean-mask
flattening, per class a host-synchronising fg.sum(), a full torch.sort, a gather, a cumsum and a dot; autograd for the
backward) on the same GPU.  Prints one JSON line.

    python tools/lovasz_time.py [--batches 1 2 8] [--iters 10] [--warmup 3]

The stock path below is a plain torch restatement of that algorithm, not the reference's code.  Times are host wall clock
around work that ends in a device synchronise.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lovasz_oracle as O  # noqa: E402

IGNORE = 255


def stock_flat(p, lab):
    """Lovász-softmax of (P, C) probabilities against (P,) labels, 'present' classes, with stock torch ops."""
    losses = []
    for c in range(p.shape[1]):
        fg = (lab == c).float()
        if fg.sum() == 0:                                   # a host sync per class, as upstream
            continue
        err = (fg - p[:, c]).abs()
        err_sorted, perm = torch.sort(err, 0, descending=True)
        fg_sorted = fg[perm]
        gts = fg_sorted.sum()
        inter = gts - fg_sorted.cumsum(0)
        union = gts + (1 - fg_sorted).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(err_sorted, jac))
    return sum(losses) / len(losses) if losses else p.sum() * 0.0


def stock_step(x, t, per_image):
    """forward + backward of the stock path on (B, C, H, W) probabilities"""
    def flat(p, lab):
        C = p.shape[1]
        pf = p.permute(0, 2, 3, 1).reshape(-1, C)
        lf = lab.reshape(-1)
        valid = lf != IGNORE
        return stock_flat(pf[valid], lf[valid])
    if per_image:
        loss = sum(flat(x[b:b + 1], t[b:b + 1]) for b in range(x.shape[0])) / x.shape[0]
    else:
        loss = flat(x, t)
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
        raise SystemExit("lovasz_time.py measures on a HIP device; none found")
    from ccnet_amd.lovasz import lovasz_softmax
    dev = torch.device("cuda:0")
    rows = []
    for B in args.batches:
        probas, labels = O.make_case_inputs(B, 19, 769, 769, seed=B)
        x = torch.from_numpy(probas).to(dev).requires_grad_(True)
        t = torch.from_numpy(labels).to(dev)
        for per_image in (False, True):
            def device_step():
                x.grad = None
                lovasz_softmax(x, t, per_image=per_image, ignore=IGNORE).backward()

            def reference_step():
                x.grad = None
                stock_step(x, t, per_image)

            dev_ms = time_it(device_step, args.iters, args.warmup)
            d_loss = float(lovasz_softmax(x, t, per_image=per_image, ignore=IGNORE).detach())
            stock_ms = time_it(reference_step, max(args.iters // 2, 1), 1)
            x.grad = None
            s_loss = float(stock_step(x, t, per_image).detach())
            rows.append({"B": B, "per_image": per_image, "device_ms": round(dev_ms, 3), "stock_path_ms": round(stock_ms, 2),
                         "speedup": round(stock_ms / dev_ms, 1), "loss_rel_diff": abs(d_loss - s_loss) / abs(s_loss)})
        del x, t
    print(json.dumps({"metric": "Lovász-softmax forward+backward at (B,19,769,769), classes 'present', ignore 255",
                      "unit": "ms per call", "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
