#!/usr/bin/env python3
"""Time one optimiser step, gradient zeroing included, over the parameter list of Seg_Model(19, recurrence=2) (342 float32
tensors, 71.3 M elements, seeded values and gradients on the device), three ways, and print one JSON line:

    device   ccnet_amd.optim.DeviceSGD(zero_grads=True): one launch of libccnet_sgd.so reads p, g and the momentum buffer and
             writes p, the buffer and a zeroed g: 24 B per element
    foreach  torch.optim.SGD (foreach, its default on a device) + zero_grad(set_to_none=False).  Its passes, per element:
             g + wd p out of place (read 8, write 4), buffer *= mu (4, 4), buffer += g (8, 4), p -= lr buffer (8, 4), g = 0 (0, 4):
             48 B
    fused    torch.optim.SGD(fused=True) + zero_grad(set_to_none=False): one multi-tensor kernel (read p, g, buffer; write p,
             buffer: 20 B) and the zeroing pass (4 B): 24 B

    python tools/sgd_time.py [--rounds 5] [--steps 200] [--warmup 20] [--lib PATH] [--only device]

The three alternate in one process: per round one window of `steps` steps each in turn, every window between two device events
on the current stream (a fraction of a second each); the line reports the median window per contender, its spread (min, max),
the algorithmic bytes, the resulting TB/s and its share of the 6.3 TB/s streaming ceiling of an MI355X.  The bytes bound the
step: nothing here can be faster than bytes / ceiling.  --lib loads another build of the library (the chunk-size candidates of
DESIGN.md §22 are builds with -DCCNET_SGD_CHUNK=...); the line names the chunk size it ran with.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING_TBS = 6.3
BYTES_PER_ELEMENT = {"device": 24, "foreach": 48, "fused": 24}
LR, MU, WD = 1e-2, 0.9, 5e-4


def model_shapes():
    from ccnet_amd.segmodel import Seg_Model
    with torch.device("meta"):                                  # the shapes only: nothing of the model is allocated
        model = Seg_Model(19, recurrence=2)
    return [tuple(p.shape) for p in model.parameters()]


def make_params(shapes, dev, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    return params


def window(step, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="steps per window (0.1 ... 0.4 s)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of libccnet_sgd.so to load (same C ABI)")
    ap.add_argument("--only", choices=sorted(BYTES_PER_ELEMENT), action="append", help="time these contenders only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_time.py measures on a HIP device; none found")
    from ccnet_amd import _sgd_lib
    from ccnet_amd.optim import DeviceSGD
    if args.lib:
        _sgd_lib._lib = _sgd_lib.SgdLibrary(args.lib)
    lib = _sgd_lib.get_lib()
    chunk = 2 ** 20 // lib.plan([2 ** 20]).shape[0]            # (both candidates divide 2^20)
    dev = torch.device("cuda:0")
    shapes = model_shapes()
    names = args.only or ["device", "foreach", "fused"]
    steps = {}
    for k, name in enumerate(names):
        params = make_params(shapes, dev, seed=k)
        if name == "device":
            opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=True)
            steps[name] = opt.step
        else:
            route = {"fused": True} if name == "fused" else {"foreach": True}
            opt = torch.optim.SGD(params, lr=LR, momentum=MU, weight_decay=WD, **route)

            def step(opt=opt):
                opt.step()
                opt.zero_grad(set_to_none=False)
            steps[name] = step
    elements = sum(p.numel() for p in params)
    for name in names:
        for _ in range(args.warmup):
            steps[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            times[name].append(window(steps[name], args.steps))
    rows = {}
    for name in names:
        ms = statistics.median(times[name])
        nbytes = BYTES_PER_ELEMENT[name] * elements
        tbs = nbytes / (ms * 1e-3) / 1e12
        rows[name] = {"ms_per_step": round(ms, 4), "ms_min_max": [round(min(times[name]), 4), round(max(times[name]), 4)],
                      "algorithmic_bytes": nbytes, "tb_per_s": round(tbs, 3), "share_of_ceiling": round(tbs / CEILING_TBS, 3),
                      "floor_ms_at_ceiling": round(nbytes / (CEILING_TBS * 1e12) * 1e3, 4)}
    print(json.dumps({"metric": "optimiser step with gradient zeroing, Seg_Model(19, recurrence=2) parameter list",
                      "tensors": len(shapes), "elements": elements, "chunk": chunk, "library": os.path.relpath(lib.path, ROOT),
                      "unit": "ms per step (median of %d windows of %d steps, contenders alternated, device events)"
                              % (args.rounds, args.steps),
                      "ceiling_tb_per_s": CEILING_TBS, "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
