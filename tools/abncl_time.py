#!/usr/bin/env python3
"""Time the channels_last device ABN (ccnet_amd.abncl, libccnet_abncl.so) against what it replaces, then the whole training
step with and without it.  Prints tables and one JSON line; ``--out`` also writes the JSON to a file.

    python tools/abncl_time.py [--rounds 9] [--iters 10] [--no-layers] [--no-step] [--out profiles/abncl_time.json]

Layers: one ABN layer (identity), forward + backward, bf16, on a dense channels_last activation at the backbone's shapes,
B = 1 and 2.  Four contenders, warmed, then timed in alternation (one round = every contender once, `iters` back-to-back
layers between two device events), median and spread (max - min) over the rounds:
    cl        the new route: the layer converted with channels_last=True, the activation as it lies
    nchw      libccnet_abn.so on the NCHW permutation of the same values, alone (what the layer cost before, without the copies)
    nchw+2cp  libccnet_abn.so on the channels_last activation as the combination would run today: one copy to NCHW on the
              way in, one back to channels_last for the next convolution (and their two mirror images in backward)
    native    the stock layer through conv3.NativeChannelsLast (torch's own batch norm kernels, the vendor library off)
GB/s is the fused algorithm's minimum -- 8 tensor passes of numel x 2 bytes -- over the contender's time, the same byte
count in every column; '% peak' is that over 8 TB/s.  Launches are the device kernels of one forward + backward, counted
by torch.profiler.
Step: B = 1, 769 x 769, --no-cudnn-benchmark: ``--bf16-params`` against ``--bf16-params --device-conv3`` against
``--bf16-params --device-conv3 --abn device --abn-channels-last``, three alternated runs each, with peak memory.

Every GPU measurement runs in a child process of its own under its own timeout, and the first that fails, is killed or
runs out of time ends the tool: nothing more is started on the device after it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 385, 385), (256, 193, 193), (256, 97, 97), (1024, 97, 97), (2048, 97, 97)]
PEAK_GBPS = 8000.0
CONTENDERS = ("cl", "nchw", "nchw+2cp", "native")
STEP_CONFIGS = {
    "bf16-params": ["--bf16-params", "--abn", "torch"],
    "conv3": ["--bf16-params", "--device-conv3", "--abn", "torch"],
    "conv3+abncl": ["--bf16-params", "--device-conv3", "--abn", "device", "--abn-channels-last"],
}


# ---------------------------------------------------------------------------------------------------------------------
# the child: one shape, every contender
# ---------------------------------------------------------------------------------------------------------------------
def layer_child(B, C, H, W, rounds, iters, warmup):
    import torch

    import inplace_abn
    from ccnet_amd import abn, conv3
    dev = torch.device("cuda", 0)
    cl = torch.channels_last
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device=dev).to(torch.bfloat16)
    dy = torch.randn(B, C, H, W, device=dev).to(torch.bfloat16)
    x_cl, dy_cl = x.contiguous(memory_format=cl), dy.contiguous(memory_format=cl)
    new = abn.ABN(C, activation="identity").to(dev).train()
    new.channels_last = True
    old = abn.ABN(C, activation="identity").to(dev).train()
    stock = torch.nn.Sequential(inplace_abn.ABN(C, activation="identity"))
    assert conv3.native_batch_norm_for_bf16_channels_last(stock) == 1           # (never the plain stock call on this input)
    stock = stock.to(dev).train()

    def run(m, xx, dd, copies=False):
        xi = xx.detach().requires_grad_(True)
        y = m(xi.contiguous()).contiguous(memory_format=cl) if copies else m(xi)
        y.backward(dd)
        return y

    calls = {"cl": lambda: run(new, x_cl, dy_cl), "nchw": lambda: run(old, x, dy),
             "nchw+2cp": lambda: run(old, x_cl, dy_cl, copies=True), "native": lambda: run(stock, x_cl, dy_cl)}
    y = calls["cl"]()
    assert y.is_contiguous(memory_format=cl) and not y.is_contiguous()
    for f in calls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / iters * 1e3)      # us
    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for k, f in calls.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            launches[k] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                        # the figure is then not measured, and says so
        launches = {k: None for k in calls}
        print("launch count not measured:", repr(e), file=sys.stderr, flush=True)
    nbytes = 8 * x.numel() * x.element_size()
    row = {"shape": [B, C, H, W], "bytes": nbytes}
    for k, v in times.items():
        med = statistics.median(v)
        row[k] = {"median_us": round(med, 1), "spread_us": round(max(v) - min(v), 1), "GBps": round(nbytes / med / 1e3, 1),
                  "pct_peak": round(100 * nbytes / med / 1e3 / PEAK_GBPS, 1), "launches": launches[k]}
    print("ROW " + json.dumps(row), flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------------
def child(argv, limit, marker):
    """run one GPU child under `timeout`; its line that starts with `marker`, parsed.  Any failure ends the tool."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable] + argv
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"abncl_time: child {' '.join(argv)} ended with status {p.returncode}; nothing more is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(marker)]
    if not lines:
        raise SystemExit(f"abncl_time: child {' '.join(argv)} printed no result; nothing more is run")
    return json.loads(lines[-1] if marker == "{" else lines[-1][len(marker):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--step-steps", type=int, default=10)
    ap.add_argument("--step-size", type=int, default=769)
    ap.add_argument("--out", default=None)
    ap.add_argument("--layer-child", type=int, nargs=4, metavar=("B", "C", "H", "W"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.layer_child:
        return layer_child(*args.layer_child, args.rounds, args.iters, args.warmup)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("abncl_time.py needs a HIP device")
    import __graft_entry__ as g
    g.build()
    result = {"tool": "abncl_time", "what": "one ABN layer (identity, bf16, channels_last activation) forward + backward; "
              "the B = 1 training step", "peak_GBps": PEAK_GBPS, "layers": [], "step": {}}
    if not args.no_layers:
        print(f"{'shape':>20} " + " ".join(f"{k + ' us':>12} {'+-':>6} {'GB/s':>7} {'%pk':>5} {'n':>3}" for k in CONTENDERS),
              flush=True)
        for B in args.batches:
            for C, H, W in SHAPES:
                row = child([os.path.abspath(__file__), "--layer-child", str(B), str(C), str(H), str(W), "--rounds",
                             str(args.rounds), "--iters", str(args.iters), "--warmup", str(args.warmup)], 180, "ROW ")
                result["layers"].append(row)
                print(f"{str(tuple(row['shape'])):>20} " + " ".join(
                    f"{row[k]['median_us']:12.1f} {row[k]['spread_us']:6.1f} {row[k]['GBps']:7.1f} {row[k]['pct_peak']:5.1f} "
                    f"{str(row[k]['launches']):>3}" for k in CONTENDERS), flush=True)
    if not args.no_step:
        runs = {k: [] for k in STEP_CONFIGS}
        for _ in range(args.step_runs):
            for k, flags in STEP_CONFIGS.items():
                r = child(["-m", "ccnet_amd.train_synthetic", "--no-cudnn-benchmark", "--size", str(args.step_size), "--steps",
                           str(args.step_steps), "--warmup", "3"] + flags, 420, "{")
                runs[k].append({"step_ms": r["ms_per_step"], "images_per_s": r["value"],
                                "max_memory_allocated_mb": r.get("max_memory_allocated_mb"), "final_loss": r["final_loss"],
                                "layout_copies": r.get("layout_copies")})
                print(k, runs[k][-1], flush=True)
        for k, v in runs.items():
            ms = [q["step_ms"] for q in v if q["step_ms"] is not None]
            result["step"][k] = {"flags": STEP_CONFIGS[k], "runs": v,
                                 "median_step_ms": round(statistics.median(ms), 2) if ms else None,
                                 "spread_ms": round(max(ms) - min(ms), 2) if ms else None}
        print({k: (v["median_step_ms"], v["spread_ms"]) for k, v in result["step"].items()}, flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
