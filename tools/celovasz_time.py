#!/usr/bin/env python3
"""Time the --lovasz criterion, forward + backward, at (B, 19, 97, 97) -> 769 x 769: the fused criterion
(ccnet_amd.celovasz.CriterionOhemDSN2, libccnet_celovasz.so: up-sample, softmax, cross-entropy and the Lovász errors on kernels
that interpolate as they read) against ccnet_amd.lovasz.CriterionOhemDSN2 (F.interpolate, F.softmax and nn.CrossEntropyLoss as
stock ops around libccnet_lovasz.so).  Prints one JSON line.

    python tools/celovasz_time.py [--batches 1 2 8] [--iters 30] [--rounds 5] [--warmup 5]

The two criteria alternate in one process: per batch size, `rounds` windows of `iters` calls each, one criterion after the
other; the line reports the median window and the spread (min, max) of each, and each criterion's peak-memory growth
(torch.cuda.max_memory_allocated above what was allocated before the call).  Times are host wall clock around work that ends
in a device synchronise.  Half of the labels are the argmax of the up-sampled logits and the rest random, 5 % are 255; the
tool checks that the two routes agree on the loss within 1e-5 and reports how far their gradients are apart (of max|grad|:
both sort fp32 errors, and where two errors differ by an ulp the routes' roundings of p order them differently).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, LOW, FULL = 19, 97, 769


def make_inputs(B, dev):
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, C, LOW, LOW, generator=g) * 3).to(dev).requires_grad_(True)
    with torch.no_grad():
        t = F.interpolate(x, size=(FULL, FULL), mode="bilinear", align_corners=True).argmax(1).cpu()
    rand = torch.randint(0, C, (B, FULL, FULL), generator=g)
    pick = torch.rand(B, FULL, FULL, generator=g) >= 0.5
    t[pick] = rand[pick]
    t[torch.rand(B, FULL, FULL, generator=g) < 0.05] = 255
    return x, t.to(dev)


def window(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak_growth(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("celovasz_time.py measures on a HIP device; none found")
    from ccnet_amd import celovasz, lovasz
    dev = torch.device("cuda:0")
    criteria = {"fused": celovasz.CriterionOhemDSN2(), "stock": lovasz.CriterionOhemDSN2()}
    rows = []
    for B in args.batches:
        x, t = make_inputs(B, dev)
        out, steps = {}, {}
        for name, crit in criteria.items():
            def step(crit=crit, name=name):
                x.grad = None
                loss = crit([x, None], t)
                loss.backward()
                out[name] = (loss.detach(), x.grad)
            steps[name] = step
            for _ in range(args.warmup):
                step()
        (lf, gf), (ls, gs) = out["fused"], out["stock"]
        loss_rel = abs(float(lf) - float(ls)) / abs(float(ls))
        grad_rel = float((gf - gs).abs().max()) / float(gs.abs().max())
        assert loss_rel <= 1e-5, (loss_rel, grad_rel)
        out.clear()
        x.grad = None
        times = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, step in steps.items():
                times[name].append(window(step, args.iters))
        row = {"B": B, "loss": float(lf), "loss_rel_diff": loss_rel, "grad_diff_of_max": grad_rel}
        for name, step in steps.items():
            out.clear()
            x.grad = None
            row[name + "_ms"] = round(statistics.median(times[name]), 4)
            row[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            row[name + "_peak_MiB"] = round(peak_growth(step), 1)
        row["stock_over_fused"] = round(row["stock_ms"] / row["fused_ms"], 2)
        rows.append(row)
        out.clear()
        del x, t, lf, gf, ls, gs
    print(json.dumps({"metric": f"CriterionOhemDSN2 forward+backward at (B,{C},{LOW},{LOW}) -> {FULL}x{FULL}, fp32",
                      "unit": "ms per call (median of %d windows of %d calls, alternated)" % (args.rounds, args.iters),
                      "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
