#!/usr/bin/env python3
"""Time the --ohem criterion, forward + backward, at (B, 19, 97, 97) -> 769 x 769 with thresh 0.6 and min_kept 200000: the fused
criterion (ccnet_amd.ohemdsn.CriterionOhemDSN, libccnet_ohemdsn.so: both heads and the threshold search on kernels that
up-sample as they read) against ccnet_amd.ohem.CriterionOhemDSN(fused_aux=True) (the OHEM head on a stock F.interpolate, the
DSN head on libccnet_dsn.so) and ccnet_amd.ohem.CriterionOhemDSN() (both heads on stock up-samples).  Prints one JSON line.

    python tools/ohemdsn_time.py [--batches 1 2 8] [--iters 50] [--rounds 5] [--warmup 5]

The three criteria alternate in one process: per batch size, `rounds` windows of `iters` calls each, one criterion after the
other; the line reports the median window and the spread (min, max) of each, and each criterion's peak-memory growth
(torch.cuda.max_memory_allocated above what was allocated before the call).  Times are host wall clock around work that ends
in a device synchronise.  70 % of the labels are the argmax of the up-sampled main logits and the rest random, so that the
threshold separates something; the line also carries each criterion's kept count, and the tool checks that the three agree
on the loss wherever they agree on the kept count.
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
THRESH, MIN_KEPT = 0.6, 200000


def make_inputs(B, dev):
    g = torch.Generator().manual_seed(B)
    xs = [(torch.randn(B, C, LOW, LOW, generator=g) * 3).to(dev).requires_grad_(True) for _ in range(2)]
    with torch.no_grad():
        t = F.interpolate(xs[0], size=(FULL, FULL), mode="bilinear", align_corners=True).argmax(1).cpu()
    rand = torch.randint(0, C, (B, FULL, FULL), generator=g)
    pick = torch.rand(B, FULL, FULL, generator=g) >= 0.70
    t[pick] = rand[pick]
    t[torch.rand(B, FULL, FULL, generator=g) < 0.05] = 255
    return xs, t.to(dev)


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ohemdsn_time.py measures on a HIP device; none found")
    from ccnet_amd import ohem, ohemdsn
    dev = torch.device("cuda:0")
    criteria = {"fused": ohemdsn.CriterionOhemDSN(thresh=THRESH, min_kept=MIN_KEPT),
                "fused_aux": ohem.CriterionOhemDSN(thresh=THRESH, min_kept=MIN_KEPT, fused_aux=True),
                "stock_up": ohem.CriterionOhemDSN(thresh=THRESH, min_kept=MIN_KEPT)}
    kept_of = {"fused": lambda c: c.last_kept, "fused_aux": lambda c: c.criterion1.last_kept,
               "stock_up": lambda c: c.criterion1.last_kept}
    rows = []
    for B in args.batches:
        xs, t = make_inputs(B, dev)
        losses, steps = {}, {}
        for name, crit in criteria.items():
            def step(crit=crit, name=name):
                for x in xs:
                    x.grad = None
                loss = crit(xs, t)
                loss.backward()
                losses[name] = loss.detach()
            steps[name] = step
            for _ in range(args.warmup):
                step()
        kept = {name: int(kept_of[name](crit).item()) for name, crit in criteria.items()}
        for name in ("fused_aux", "stock_up"):
            if kept[name] == kept["fused"]:
                assert abs(float(losses["fused"]) - float(losses[name])) <= 1e-5 * abs(float(losses[name])), (losses, kept)
        times = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, step in steps.items():
                times[name].append(window(step, args.iters))
        row = {"B": B, "kept": kept, "loss": {k: float(v) for k, v in losses.items()}}
        for name, step in steps.items():
            row[name + "_ms"] = round(statistics.median(times[name]), 4)
            row[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            row[name + "_peak_MiB"] = round(peak_growth(step), 1)
        row["fused_aux_over_fused"] = round(row["fused_aux_ms"] / row["fused_ms"], 2)
        row["stock_up_over_fused"] = round(row["stock_up_ms"] / row["fused_ms"], 2)
        rows.append(row)
        del xs, t
    print(json.dumps({"metric": f"CriterionOhemDSN forward+backward at (B,{C},{LOW},{LOW}) -> {FULL}x{FULL}, two heads, fp32, "
                                f"thresh {THRESH}, min_kept {MIN_KEPT}",
                      "unit": "ms per call (median of %d windows of %d calls, alternated)" % (args.rounds, args.iters),
                      "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
