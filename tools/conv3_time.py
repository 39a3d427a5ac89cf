#!/usr/bin/env python3
"""Time the 3x3 dilated convolution of the model's six shape families on the 97 x 97 map, in one process, three contenders:

    library        libccnet_conv3.so through ccnet_amd.conv3 (bf16, channels_last)
    stock_cl       F.conv2d, bf16, channels_last, cudnn.benchmark as the process has it (off by default)
    stock_nchw     F.conv2d, bf16, NCHW, warmed with cudnn.benchmark on (--no-benchmark: as the process has it): NCHW MIOpen at its
                   best.  ``train_synthetic --bf16-params`` runs NCHW with the flag OFF unless --cudnn-benchmark is given

    python tools/conv3_time.py [--families layer3 layer4 ...] [--batches 1 2 8] [--map 97 97] [--repeats 7] [--iters 10]
                               [--warmup 2] [--no-benchmark] [--step-runs 0] [--out FILE]

For each family and batch: forward, input gradient, weight gradient (with its finishing launch) and the pack, each alone, and one
forward + backward through autograd.  Method as tools/bf16_module_time.py: the contenders are warmed, then timed ALTERNATELY --
``repeats`` windows each of ``iters`` back-to-back launches between two device events -- and the median and min .. max of the
windows are reported.  Per launch the FLOPs, their share of the 2.5 PFLOP/s bf16 MFMA peak, and the bytes from the shapes against
8 TB/s are printed with the two floors.  Before timing, each shape's forward is checked against the fp64 sum on the rows of the
first 256-row tile, a middle tile and the last tile, at the bar of tests/conv3_cases.py.

``--step-runs N`` (N > 0) then takes the whole step: ``train_synthetic --bf16-params`` with and without ``--device-conv3``, B = 1,
769 x 769, N alternated runs each, cudnn.benchmark off in both as the driver leaves it; both times and the run-to-run spread
are reported.  One JSON line; ``--out`` also keeps it
(rewritten after every family, so a run that is cut short leaves what it measured).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S, MFMA_FLOPS = 8e12, 2.5e15
# name -> (Cin, Cout, dilation, bias): ccnet_amd/segmodel.py
FAMILIES = {"layer3": (256, 256, 2, False), "layer4": (512, 512, 4, False), "conva": (2048, 512, 1, False),
            "convb": (512, 512, 1, False), "bottleneck": (2560, 512, 1, False), "dsn": (1024, 512, 1, True)}


def launch_accounting(M, ci, co, slabs):
    """{launch: (bytes it must move, flops)} from the shapes alone: every operand read once, every result written once"""
    w = 9 * ci * co
    return {
        "forward": (M * ci * 2 + w * 2 + M * co * 2, 2 * M * w),                                   # x, pack -> y
        "dx": (M * co * 2 + w * 2 + M * ci * 2, 2 * M * w),                                        # dy, pack -> dx
        "wgrad": (M * co * 2 + M * ci * 2 + 2 * slabs * w * 4 + w * 2, 2 * M * w),                 # dy, x -> partials -> dW
        "pack": (w * 2 + 2 * w * 2, 0),                                                            # parameter -> two packs
    }


def floors(nbytes, flops):
    tb, tf = nbytes / HBM_BYTES_PER_S * 1e3, flops / MFMA_FLOPS * 1e3
    return {"bytes": nbytes, "flops": flops, "floor_bytes_ms": round(tb, 4), "floor_flops_ms": round(tf, 4),
            "bound": "HBM" if tb > tf else "MFMA"}


def window(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters           # ms per call


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def alternate(fns, repeats, iters, warmup):
    """{name: summary} of contenders warmed, then timed in alternation"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    t = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t[name].append(window(fn, iters))
    return {name: summary(ts) for name, ts in t.items()}


def check_forward(x, wt, bias, y, d):
    """rows of the first tile, a middle tile and the last tile against the fp64 sum: |got - ref| <= 2^-8 |ref| + 2e-6 mag"""
    B, K, H, W = x.shape
    M, N, HW = B * H * W, wt.shape[0], H * W
    x2, y2 = x.permute(0, 2, 3, 1).reshape(M, K), y.permute(0, 2, 3, 1).reshape(M, N)
    tiles = (M + 255) // 256
    rows = sorted({r for t0 in (0, tiles // 2, tiles - 1) for r in range(256 * t0, min(256 * t0 + 256, M), 3)} | {0, M - 1})
    idx = torch.tensor(rows, device=x.device)
    pix = idx % HW
    h, w = pix // W, pix % W
    ref = torch.zeros(len(rows), N, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for t in range(9):
        yy, xx = h + (t // 3 - 1) * d, w + (t % 3 - 1) * d
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        src = (idx - pix + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))
        a = x2[src].double() * ok[:, None]
        wk = wt[:, t * K:(t + 1) * K].double()
        ref += a @ wk.t()
        mag += a.abs() @ wk.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    err = (y2[idx].double() - ref).abs()
    bar = 2.0 ** -8 * ref.abs() + 2e-6 * mag
    worst = float((err / bar.clamp_min(1e-300)).max())
    if not bool((err <= bar).all()):
        raise SystemExit(f"forward check failed on sampled rows: worst err / bar = {worst:.3f}")
    return {"rows": len(rows), "max_abs_err": float(err.max()), "worst_err_over_bar": round(worst, 4)}


def time_family(name, B, H, W, args, dev):
    from ccnet_amd import _conv3_lib
    from ccnet_amd.conv3 import _launch, _pack, _wgrad, conv3x3
    ci, co, d, has_bias = FAMILIES[name]
    M = B * H * W
    g = torch.Generator(device=dev).manual_seed(ci + co + d + B)
    x = torch.randn(B, H, W, ci, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    dy = torch.randn(B, H, W, co, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    w = (torch.randn(co, ci, 3, 3, device=dev, generator=g) / (9 * ci) ** 0.5).to(torch.bfloat16)
    bias = (torch.randn(co, device=dev, generator=g) * 0.1).to(torch.bfloat16) if has_bias else None
    xn, dyn = x.contiguous(), dy.contiguous()
    wcl = w.contiguous(memory_format=torch.channels_last)
    fwd, adj = _pack(w)
    b32 = None if bias is None else bias.float()
    check = check_forward(x, fwd, b32, _launch(x, ci, fwd, b32, d), d)
    slabs = _conv3_lib.get_lib().ccnet_conv3_wgrad_slabs(B, H, W, co, ci)
    conv = dict(stride=1, padding=d, dilation=d)
    geo = ([1, 1], [d, d], [d, d], False, [0, 0], 1)

    def bwd(xx, ww, mask):
        return lambda: torch.ops.aten.convolution_backward(dy if xx is x else dyn, xx, ww, None, *geo, mask)

    def step(fn, xx, ww, grad):
        xr, wr = xx.detach().requires_grad_(True), ww.detach().requires_grad_(True)
        br = None if bias is None else bias.detach().requires_grad_(True)
        return lambda: fn(xr, wr, br).backward(grad)

    bench = torch.backends.cudnn.benchmark
    groups = {}
    try:
        with torch.no_grad():
            torch.backends.cudnn.benchmark = not args.no_benchmark        # (the NCHW contender's setting; MIOpen keeps what it found)
            for fn in (lambda: F.conv2d(xn, w, bias, **conv), bwd(xn, w, [True, False, False]), bwd(xn, w, [False, True, False])):
                fn()
            torch.backends.cudnn.benchmark = bench
            groups["forward"] = {"library": lambda: _launch(x, ci, fwd, b32, d), "stock_cl": lambda: F.conv2d(x, wcl, bias, **conv),
                                 "stock_nchw": lambda: F.conv2d(xn, w, bias, **conv)}
            groups["dx"] = {"library": lambda: _launch(dy, co, adj, None, d), "stock_cl": bwd(x, wcl, [True, False, False]),
                            "stock_nchw": bwd(xn, w, [True, False, False])}
            groups["wgrad"] = {"library": lambda: _wgrad(dy, co, x, ci, d, torch.bfloat16, tuple(w.shape)),
                               "stock_cl": bwd(x, wcl, [False, True, False]), "stock_nchw": bwd(xn, w, [False, True, False])}
            groups["pack"] = {"library": lambda: _pack(w)}
        groups["forward_backward"] = {"library": step(lambda a, b, c: conv3x3(a, b, c, d), x, w, dy),
                                      "stock_cl": step(lambda a, b, c: F.conv2d(a, b, c, **conv), x, wcl, dy),
                                      "stock_nchw": step(lambda a, b, c: F.conv2d(a, b, c, **conv), xn, w, dyn)}
        acct = launch_accounting(M, ci, co, slabs)
        acct["forward_backward"] = tuple(sum(acct[k][i] for k in ("forward", "dx", "wgrad", "pack")) for i in (0, 1))
        row = {"family": name, "shape": [B, ci, H, W], "cout": co, "dilation": d, "bias": has_bias, "M": M, "wgrad_slabs": slabs,
               "forward_check": check, "launches": {}}
        for what, fns in groups.items():
            with torch.set_grad_enabled(what == "forward_backward"):
                times = alternate(fns, args.repeats, args.iters, args.warmup)
            nbytes, flops = acct[what]
            entry = dict(floors(nbytes, flops), contenders=times)
            for t in times.values():
                sec = t["median_ms"] * 1e-3
                t.update({"share_of_mfma_peak": round(flops / sec / MFMA_FLOPS, 4), "share_of_8TBps": round(nbytes / sec / HBM_BYTES_PER_S, 4)})
            if "stock_cl" in times:
                best = min(times["stock_cl"]["median_ms"], times["stock_nchw"]["median_ms"])
                entry["library_over_best_stock"] = round(times["library"]["median_ms"] / best, 3)
            row["launches"][what] = entry
    finally:
        torch.backends.cudnn.benchmark = bench
    return row


def time_steps(runs, dev):
    """``train_synthetic --bf16-params`` with and without ``--device-conv3``, B = 1, 769 x 769, alternated runs"""
    from ccnet_amd import train_synthetic as T
    base = ["--bf16-params", "--steps", "5", "--warmup", "3", "--batch-per-gpu", "1"]
    t = {"stock": [], "device_conv3": []}
    for _ in range(runs):
        for name, extra in (("stock", []), ("device_conv3", ["--device-conv3"])):
            t[name].append(T.run(T.parse_args(base + extra), quiet=True)["ms_per_step"])
            torch.cuda.empty_cache()
    out = {name: dict(summary(ts), runs_ms=ts) for name, ts in t.items()}
    out["spread_ms"] = round(max(v["max_ms"] - v["min_ms"] for v in (out["stock"], out["device_conv3"])), 3)
    out["gain_ms"] = round(out["stock"]["median_ms"] - out["device_conv3"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--families", nargs="+", default=list(FAMILIES), choices=list(FAMILIES))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--map", type=int, nargs=2, default=[97, 97], metavar=("H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-benchmark", action="store_true", help="leave cudnn.benchmark off for the NCHW contender")
    ap.add_argument("--step-runs", type=int, default=0, help="alternated whole-step runs of train_synthetic (0: skip)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv3_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    H, W = args.map
    result = {"tool": "conv3_time", "what": "3x3 dilated convolution, bf16: library vs F.conv2d channels_last vs F.conv2d NCHW "
              "(cudnn.benchmark), alternated", "device": torch.cuda.get_device_name(dev), "map": [H, W], "repeats": args.repeats,
              "iters": args.iters, "cudnn_benchmark_for_nchw": not args.no_benchmark, "rows": []}

    def keep():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result) + "\n")

    for B in args.batches:
        for name in args.families:
            row = time_family(name, B, H, W, args, dev)
            result["rows"].append(row)
            fb = row["launches"]["forward_backward"]["contenders"]
            print(f"[conv3_time] {name} B={B}: fwd+bwd ms " + ", ".join(f"{k} {v['median_ms']}" for k, v in fb.items()), file=sys.stderr, flush=True)
            keep()
            torch.cuda.empty_cache()
    if args.step_runs > 0:
        result["train_step"] = time_steps(args.step_runs, dev)
        keep()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
