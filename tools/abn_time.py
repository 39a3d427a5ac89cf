#!/usr/bin/env python3
"""Time one ABN layer, forward + backward, at the backbone's shapes: the device layer (ccnet_amd.abn, libccnet_abn.so; out
of place and in place) against the stock inplace_abn restatement (F.batch_norm and autograd) on the same GPU.  Identity
activation, as the backbone's BatchNorm2d.  Prints one table row per shape and one JSON line.

    python tools/abn_time.py [--batches 1 2 8] [--iters 20] [--warmup 3]

GB/s is the same byte count for every column -- the fused algorithm's minimum, 8 tensor passes (forward: x read for the
statistics, x read and y written; backward: x and dy read for the reduction, x and dy read and dx written) -- over that
column's time, so it ranks the columns like the times do.  Times are device events around `iters` back-to-back layers.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import inplace_abn  # noqa: E402

SHAPES = [(64, 385, 385), (256, 193, 193), (256, 97, 97), (1024, 97, 97), (2048, 97, 97)]


def time_layer(m, x, dy, iters, warmup):
    inplace = getattr(m, "inplace", False)

    def once():
        xi = x.detach().requires_grad_(True)
        y = m(xi * 1.0 if inplace else xi)          # in place needs a non-leaf input: one multiply in that column
        y.backward(dy)

    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abn_time.py needs a HIP device")
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import abn
    dev = torch.device("cuda", 0)
    rows = []
    print(f"{'dtype':5} {'shape':>20} {'stock us':>10} {'device us':>10} {'inplace us':>10} {'stock GB/s':>10} "
          f"{'device GB/s':>11} {'inplace GB/s':>12}", flush=True)
    for dt in args.dtypes:
        dtype = torch.float32 if dt == "f32" else torch.bfloat16
        for B in args.batches:
            for C, H, W in SHAPES:
                torch.manual_seed(0)
                x = torch.randn(B, C, H, W, device=dev).to(dtype)
                dy = torch.randn(B, C, H, W, device=dev).to(dtype)
                stock = inplace_abn.InPlaceABNSync(C, activation="identity").to(dev).train()
                device = abn.ABN(C, activation="identity").to(dev).train()
                inplace = abn.InPlaceABN(C, activation="identity").to(dev).train()
                t = {k: time_layer(m, x, dy, args.iters, args.warmup)
                     for k, m in (("stock", stock), ("device", device), ("inplace", inplace))}
                nbytes = 8 * x.numel() * x.element_size()
                row = {"dtype": dt, "shape": [B, C, H, W], **{f"{k}_us": round(v, 1) for k, v in t.items()},
                       **{f"{k}_GBps": round(nbytes / v / 1e3, 1) for k, v in t.items()}}
                rows.append(row)
                print(f"{dt:5} {str((B, C, H, W)):>20} {t['stock']:10.1f} {t['device']:10.1f} {t['inplace']:10.1f} "
                      f"{row['stock_GBps']:10.1f} {row['device_GBps']:11.1f} {row['inplace_GBps']:12.1f}", flush=True)
                del x, dy
                torch.cuda.empty_cache()
    print(json.dumps({"tool": "abn_time", "what": "one ABN layer (identity) forward + backward", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
