#!/usr/bin/env python3
"""Time the optimiser's share of a bf16 training step over the parameter list of Seg_Model(19, recurrence=2) (342 tensors,
71.3 M elements, seeded values and gradients on the device), the mixed-precision route against the route it replaces, and print
one JSON line:

    mixed       ccnet_amd.optim.DeviceMixedSGD(zero_grads=True) with every tensor bf16 beside a float32 master: one launch of
                libccnet_sgdmp.so reads g (2 B), the master and the momentum buffer (4 B each) and writes the master, the buffer,
                p and a zeroed g: 22 B per element
    mixed+acc   the same, and per tensor the add of a fresh bf16 gradient into the kept bf16 .grad that autograd does on that
                route (read 2 + 2, write 2): 28 B
    parent      what `--bf16 --device-sgd` does per step around float32 parameters: ccnet_amd.optim.DeviceSGD(zero_grads=True)
                (24 B), per tensor the cast p.to(bfloat16) that autocast launches (read 4, write 2) and per tensor the
                g_bf16.float() (read 2, write 4) that autograd adds into the kept float32 .grad (read 4 + 4, write 4): 48 B, in
                1 + 3 x 342 launches

    python tools/sgdmp_time.py [--rounds 5] [--steps 100] [--warmup 10] [--lib PATH] [--only mixed]

The contenders alternate in one process: per round one window of `steps` steps each in turn, every window between two device
events on the current stream; the line reports the median window per contender, its spread (min, max), the algorithmic bytes,
the resulting TB/s and its share of the 6.3 TB/s streaming ceiling of an MI355X.  The per-tensor launches of `parent` and
`mixed+acc` are issued from Python here, as autocast and autograd issue theirs from C++: their host cost is part of what is
measured, and a window is bounded by whichever of host and device is slower.  --lib loads another build of the library.
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
BYTES_PER_ELEMENT = {"mixed": 22, "mixed+acc": 28, "parent": 48}
LR, MU, WD = 1e-2, 0.9, 5e-4


def model_shapes():
    from ccnet_amd.segmodel import Seg_Model
    with torch.device("meta"):                                  # the shapes only: nothing of the model is allocated
        model = Seg_Model(19, recurrence=2)
    return [tuple(p.shape) for p in model.parameters()]


def make_params(shapes, dev, seed, dtype):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(s, device=dev, generator=gen) * 0.05).to(dtype)) for s in shapes]
    for p in params:
        p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 1e-3).to(dtype)
    fresh = [(torch.randn(p.shape, device=dev, generator=gen) * 1e-3).to(torch.bfloat16) for p in params]
    return params, fresh


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
    ap.add_argument("--steps", type=int, default=100, help="steps per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lib", default=None, help="another build of libccnet_sgdmp.so to load (same C ABI)")
    ap.add_argument("--only", choices=sorted(BYTES_PER_ELEMENT), action="append", help="time these contenders only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgdmp_time.py measures on a HIP device; none found")
    from ccnet_amd import _sgdmp_lib
    from ccnet_amd.optim import DeviceMixedSGD, DeviceSGD
    if args.lib:
        _sgdmp_lib._lib = _sgdmp_lib.SgdmpLibrary(args.lib)
    lib = _sgdmp_lib.get_lib()
    dev = torch.device("cuda:0")
    shapes = model_shapes()
    names = args.only or ["mixed", "mixed+acc", "parent"]
    steps = {}
    for k, name in enumerate(names):
        if name == "parent":
            params, fresh = make_params(shapes, dev, k, torch.float32)
            opt = DeviceSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=True)

            @torch.no_grad()
            def step(opt=opt, params=params, fresh=fresh):
                for p in params:
                    p.to(torch.bfloat16)                        # autocast's per-step cast of the weight
                for p, g in zip(params, fresh):
                    p.grad.add_(g.float())                      # autograd: the bf16 gradient widened, then accumulated
                opt.step()
        else:
            params, fresh = make_params(shapes, dev, k, torch.bfloat16)
            opt = DeviceMixedSGD(params, lr=LR, momentum=MU, weight_decay=WD, zero_grads=True)
            if name == "mixed":
                step = opt.step
            else:
                @torch.no_grad()
                def step(opt=opt, params=params, fresh=fresh):
                    for p, g in zip(params, fresh):
                        p.grad.add_(g)
                    opt.step()
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
    print(json.dumps({"metric": "optimiser share of a bf16 step, Seg_Model(19, recurrence=2) parameter list",
                      "tensors": len(shapes), "elements": elements, "library": os.path.relpath(lib.path, ROOT),
                      "unit": "ms per step (median of %d windows of %d steps, contenders alternated, device events)"
                              % (args.rounds, args.steps),
                      "ceiling_tb_per_s": CEILING_TBS, "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
