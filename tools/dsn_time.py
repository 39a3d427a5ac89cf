#!/usr/bin/env python3
"""Time the DSN criterion, forward + backward, at (B, 19, 97, 97) -> 769 x 769: the device criterion (ccnet_amd.dsn,
libccnet_dsn.so, the up-sample inside the kernels) against the stock one (ccnet_amd.segmodel.CriterionDSN: F.interpolate +
F.cross_entropy per head).  Prints one JSON line.

    python tools/dsn_time.py [--batches 1 2 8] [--iters 50] [--rounds 5] [--warmup 5]

The two criteria alternate in one process: per batch size, `rounds` windows of `iters` calls each, device and stock in turn;
the line reports the median window and the spread (min, max) of each, and each criterion's peak-memory growth
(torch.cuda.max_memory_allocated above what was allocated before the call).  Times are host wall clock around work that ends
in a device synchronise.  It also checks that the two agree on the loss at every size it times.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, LOW, FULL = 19, 97, 769


def make_inputs(B, dev):
    g = torch.Generator().manual_seed(B)
    xs = [(torch.randn(B, C, LOW, LOW, generator=g) * 3).to(dev).requires_grad_(True) for _ in range(2)]
    t = torch.randint(0, C, (B, FULL, FULL), generator=g)
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
        raise SystemExit("dsn_time.py measures on a HIP device; none found")
    from ccnet_amd import dsn, segmodel
    dev = torch.device("cuda:0")
    criteria = {"device": dsn.CriterionDSN(), "stock": segmodel.CriterionDSN()}
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
        assert abs(float(losses["device"]) - float(losses["stock"])) <= 1e-5 * abs(float(losses["stock"])), losses
        times = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, step in steps.items():
                times[name].append(window(step, args.iters))
        row = {"B": B}
        for name, step in steps.items():
            row[name + "_ms"] = round(statistics.median(times[name]), 4)
            row[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            row[name + "_peak_MiB"] = round(peak_growth(step), 1)
        row["stock_over_device"] = round(row["stock_ms"] / row["device_ms"], 2)
        rows.append(row)
        del xs, t
    print(json.dumps({"metric": f"CriterionDSN forward+backward at (B,{C},{LOW},{LOW}) -> {FULL}x{FULL}, two heads, fp32",
                      "unit": "ms per call (median of %d windows of %d calls, alternated)" % (args.rounds, args.iters),
                      "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
