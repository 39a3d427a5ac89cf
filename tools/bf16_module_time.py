#!/usr/bin/env python3
"""Time the bf16 module, forward + backward, on its two routes in one process: the stock projections (``bf16-pixel-major``:
F.linear and autograd) against the library's own (``bf16-pixel-major-lib``: libccnet_proj.so, one autograd node), at BASELINE
configs[4]'s shape, bf16 channels_last.  Prints one JSON line.

    python tools/bf16_module_time.py [--shape 16 512 129 129] [--repeats 9] [--iters 20] [--warmup 3] [--out FILE]

Method: both routes are warmed, then timed ALTERNATELY -- ``repeats`` windows each of ``iters`` back-to-back steps between two
device events -- so that whatever else the machine does falls on both; the median and the spread (min .. max) of the windows
are printed for each.  The three GEMMs, the column sums and the pack are timed alone the same way; for each the bytes it must
move and the operations it needs are computed from the shapes (``launch_accounting``) and put over the time, against the
8 TB/s HBM roofline.  Before any timing the forward GEMM at this size is checked against the fp64 product on sampled rows --
rows of the first 256-row tile, of the middle and of the last, partial one -- at the bar of tests/proj_cases.py.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def launch_accounting(B, C, H, W, slabs=0):
    """{launch: (bytes it must move, flops)} from the shapes alone: every operand read once, every result written once"""
    M, cq = B * H * W, C // 8
    N = 2 * cq + C
    return {
        "pack": (2 * (N * C * 2) + N * C * 2 + 2 * N * 4, 0),                              # parameters in, w and wt out, bias in and out
        "gemm_forward": (M * C * 2 + N * C * 2 + N * 4 + M * N * 2, 2 * M * N * C),        # x, w, bias -> qkv
        "gemm_dx": (M * N * 2 + C * N * 2 + M * C * 2 + M * C * 2, 2 * M * N * C),         # dqkv, wt, dy -> dx
        "gemm_dw": (M * N * 2 + M * C * 2 + max(slabs, 1) * N * C * 4, 2 * M * N * C),     # dqkv, x -> the partials
        "colsum": (M * N * 2 + N * 4, M * N),                                              # dqkv -> db
    }


def windows(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
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


def check_forward_gemm(x2, w, b, qkv):
    """sampled rows of the forward GEMM against the fp64 product of the same bf16 operands: |got - ref| <= 2^-8 |ref| + 2e-6 mag"""
    M = x2.shape[0]
    last = (M - 1) // 256 * 256
    rows = sorted(set([0, 1, 63, 64, 127, 255, M // 2, M // 2 + 1] + list(range(last, M)) + [last - 1, M - 1]))
    idx = torch.tensor([r for r in rows if 0 <= r < M], device=x2.device)
    a64, w64 = x2[idx].double(), w.double()
    ref = a64 @ w64.t() + b.double()
    mag = a64.abs() @ w64.abs().t() + b.double().abs()
    err = (qkv[idx].double() - ref).abs()
    bar = 2.0 ** -8 * ref.abs() + 2e-6 * mag
    worst = float((err / bar).max())
    if not bool((err <= bar).all()):
        raise SystemExit(f"forward GEMM check failed on sampled rows: worst err / bar = {worst:.3f}")
    return {"rows": int(idx.numel()), "first_tile_rows": int((idx < 256).sum()), "last_tile_rows": int((idx >= last).sum()),
            "max_abs_err": float(err.max()), "worst_err_over_bar": round(worst, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=4, default=[16, 512, 129, 129], metavar=("B", "C", "H", "W"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_module_time.py needs a HIP device")
    from ccnet_amd import CrissCrossAttention, _lib
    from ccnet_amd.functions import _proj_colsum, _proj_gemm, _proj_pack, _projection_wgrad_gemm
    B, C, H, W = args.shape
    M, cq = B * H * W, C // 8
    N = 2 * cq + C
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = CrissCrossAttention(C).to(dev).to(torch.bfloat16)
    with torch.no_grad():
        m.gamma.fill_(0.5)
    x = torch.randn(B, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn(B, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    params = (m.query_conv.weight, m.query_conv.bias, m.key_conv.weight, m.key_conv.bias, m.value_conv.weight, m.value_conv.bias)

    # the operands of the launches timed alone (dqkv: any bf16 rows do; the kernels' time does not depend on the values)
    x2 = x.detach().permute(0, 2, 3, 1).reshape(M, C)
    dy2 = dy.permute(0, 2, 3, 1).reshape(M, C)
    w, wt, b = _proj_pack(*params)
    qkv = _proj_gemm(x2, w, b)
    check = check_forward_gemm(x2, w, b, qkv)
    print("forward GEMM check:", check, flush=True)
    dqkv = torch.randn(M, N, device=dev).to(torch.bfloat16)
    cca = _lib.get_lib()

    def step(library):
        m.library_bf16_projections = library
        m.zero_grad(set_to_none=True)
        x.grad = None
        m(x).backward(dy)

    routes = {}
    for library in (False, True):
        m.library_bf16_projections = library
        routes[library] = m.route(x)
    assert routes == {False: "bf16-pixel-major", True: "bf16-pixel-major-lib"}, routes
    for library in (False, True):
        windows(lambda: step(library), args.warmup)
    t = {False: [], True: []}
    for _ in range(args.repeats):
        for library in (False, True):                                      # alternated: drift falls on both
            t[library].append(windows(lambda: step(library), args.iters))
    m.library_bf16_projections = False

    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tiles = -(-N // 128) * -(-C // 256)
    slabs = max(1, min(cus // tiles if tiles <= cus else 1, -(-M // 64)))
    alone = {
        "pack": lambda: _proj_pack(*params),
        "gemm_forward": lambda: _proj_gemm(x2, w, b),
        "gemm_dx": lambda: _proj_gemm(dqkv, wt, None, dy2),
        "gemm_dw": lambda: _projection_wgrad_gemm(cca, dqkv, x2),
        "colsum": lambda: _proj_colsum(dqkv),
    }
    stock_alone = {
        "stock_forward_linear": lambda: torch.nn.functional.linear(x2, w, b.to(torch.bfloat16)),
        "stock_dx_mm_plus_add": lambda: torch.mm(dqkv, w).add_(dy2),
        "stock_dw_mm": lambda: torch.mm(dqkv.t(), x2),
        "stock_db_sum": lambda: dqkv.sum(0),
    }
    acct = launch_accounting(B, C, H, W, slabs)
    launches = {}
    for name, fn in list(alone.items()) + list(stock_alone.items()):
        windows(fn, args.warmup)
        ts = [windows(fn, args.iters) for _ in range(args.repeats)]
        row = summary(ts)
        if name in acct:
            nbytes, flops = acct[name]
            sec = row["median_ms"] * 1e-3
            row.update({"bytes": nbytes, "flops": flops, "TBps": round(nbytes / sec / 1e12, 3),
                        "share_of_8TBps_roofline": round(nbytes / sec / HBM_BYTES_PER_S, 3), "TFLOPs": round(flops / sec / 1e12, 1)})
        launches[name] = row

    stock, ours = summary(t[False]), summary(t[True])
    spread = max(stock["max_ms"] - stock["min_ms"], ours["max_ms"] - ours["min_ms"])
    result = {
        "tool": "bf16_module_time", "what": "module forward + backward, bf16 channels_last, stock vs library projections, alternated",
        "device": torch.cuda.get_device_name(dev), "shape": [B, C, H, W], "M": M, "N": N, "repeats": args.repeats, "iters": args.iters,
        "forward_gemm_check": check,
        "stock_route": {"route": routes[False], **stock}, "library_route": {"route": routes[True], **ours},
        "gain_ms": round(stock["median_ms"] - ours["median_ms"], 4), "spread_ms": round(spread, 4),
        "library_wins_by_more_than_the_spread": bool(stock["median_ms"] - ours["median_ms"] > spread),
        "launches_alone": launches,
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
