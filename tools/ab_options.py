#!/usr/bin/env python3
"""A/B of library options on the headline split-plane step, on ONE set of buffers inside ONE process (boxes of the pool differ
by 3-4 %, so only same-run comparisons count).  Per option set: eager step ms, hipGraph replay ms, fwd / bwd ms and -- with
every launch on one stream -- the per-launch durations.
The "order-*" sets are the A/B of option "cache_order" (which streaming launches walk the images in descending order):
a mask WINS only if its graph-replay step is below order-0's in EVERY round and its mean gain exceeds the largest difference
between two rounds of one set -- the run's own noise; the closing table says so per set.
The "policy-*" sets are the A/B of option "stream_policy" (the cache policy of the step's C-sized streams): "policy-0"
is the step of before the option, "policy-<name>" one live bit (bits 8 and 9 act together: one set), "policy-mNN" the mask NN,
"policy-shipped" the library's default; the same table and the same win rule, against policy-0.
usage: ab_options.py [B C H W] [--sets name,name,... ("order": every order-* set; "order-mNN": mask NN; "policy": policy-0 and
       every live bit; "policy-mNN")] [--rounds N]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ccnet_amd import _lib  # noqa: E402

args = [a for i, a in enumerate(sys.argv[1:]) if not a.startswith("--") and sys.argv[i] not in ("--sets", "--rounds")]
B, C, H, W = (int(a) for a in args[:4]) if len(args) >= 4 else (8, 512, 97, 97)
DEFAULT_SETS = {
    "default": {},
    "v-as-planes": {"_direct": 0},           # the forward splits v into planes first (what maps beyond 100 positions run)
    "no-xcd": {"planes_xcd": 0},
    "no-energy-tail": {"energy_tail": 0},
    "dqdk-2-per-cu": {"dqdk_wpc3": 0},       # ca_backward on the two-slot / two-workgroups-per-CU form
    "dA-3-stages": {"da_stages": 3},         # the persistent dA kernel with three ring stages: it fills the LDS, nothing runs next to it
    "dA-3-stages-1s": {"da_stages": 3, "planes_overlap": 0},    # the energies launch as one workgroup per strip (2.02 rounds -> three)
    "one-stream": {"planes_overlap": 0},
    "overlap-1": {"planes_overlap": 1},
    "dqdk-three-terms": {"dqdk_exact": 0},   # ca_backward with three bf16 terms per product instead of six (round 6 default: six, fp32-equivalent)
    "ring-2-per-cu": {"planes_ring": 1},     # the column ring passes with three slots and TWO workgroups per CU (slow-box A/B)
    # "cache_order": bit 0 forward column pass (L3), 1 forward NCHW row pass (L4), 2 dA (L6), 3 dv column pass (L7), 4 dv row pass (L8)
    # descending; bit 5 = L4 on the image-major XCD decode with ascending images
    "order-0": {"cache_order": 0},                              # the traversal of before the option
    "order-model": {"cache_order": 14},                         # L4, L6, L7 descending: the residency model's pattern
    "order-L3": {"cache_order": 1},
    "order-L4": {"cache_order": 2},
    "order-L6": {"cache_order": 4},
    "order-L7": {"cache_order": 8},
    "order-L8": {"cache_order": 16},
    "order-L4-xcd": {"cache_order": 32},
    "order-model-no-xcd": {"cache_order": 14, "planes_xcd": 0},
    "order-complement": {"cache_order": 17},                    # L3 and L8 descending, L4, L6, L7 ascending
    # "stream_policy": one bit per (launch, operand class), cca_api.hip
    "policy-0": {"stream_policy": 0},                           # every access as before the option
    "policy-shipped": {"stream_policy": -1},
    "policy-L4-loads-nt": {"stream_policy": 1 << 1},            # forward NCHW row pass: v, partial, x loads non-temporal
    "policy-L8-nt": {"stream_policy": 3 << 8},                  # dv row pass: plane and partial loads, dv stores non-temporal
}
if "--sets" in sys.argv:
    keep = sys.argv[sys.argv.index("--sets") + 1].split(",")
    for k in keep:                                      # "order-mNN": any other mask of "cache_order"
        if k.startswith("order-m") and k[7:].isdigit():
            DEFAULT_SETS[k] = {"cache_order": int(k[7:])}
        if k.startswith("policy-m") and k[8:].isdigit():
            DEFAULT_SETS[k] = {"stream_policy": int(k[8:])}
    DEFAULT_SETS = {k: v for k, v in DEFAULT_SETS.items() if k in keep or k == "default" or ("order" in keep and k.startswith("order-"))
                    or ("policy" in keep and k.startswith("policy-"))}
else:
    DEFAULT_SETS = {k: v for k, v in DEFAULT_SETS.items() if not k.startswith("policy-")}      # (the policy A/B runs when asked for)
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 2
DETAIL = ("one-stream", "dqdk-three-terms") + tuple(k for k in DEFAULT_SETS if k.startswith(("order-", "policy-")))
lib = _lib.get_lib()
dev = torch.device("cuda:0")
BASE = {"planes_ring": 2, "planes_stream": 1, "planes_overlap": -1, "planes_xcd": 1, "energy_tail": 1, "da_stages": 2, "dqdk_wpc3": 1,
        "dqdk_exact": 1, "cache_order": -1, "stream_policy": -1}
wl = bench.PlanesWorkload(lib, B, C, H, W, dev, 1234)
ref = None
graph_ms = {}                              # set -> graph-replay ms per round
for rnd in range(ROUNDS):                  # (two rounds by default: the order of the sets must not matter)
    for name, opts in DEFAULT_SETS.items():
        for k, v in {**BASE, **opts}.items():
            if not k.startswith("_"):
                lib.set_option(k, v)
        wl.direct = bool(opts.get("_direct", 1)) and max(H, W) <= 100          # (the plane-free form serves strips <= 100)
        if not wl.direct and wl.vpl is None:
            wl.vpl = torch.empty(B, H, W, 2, C, dtype=torch.int16, device=dev)
        for _ in range(5):
            wl.step()
        torch.cuda.synchronize()
        out = (wl.y.clone(), wl.dqkv.clone(), wl.dgamma.clone())
        if ref is None:
            ref = out
        same = all(torch.equal(a, b) for a, b in zip(out[1:], ref[1:])) and float((out[0] - ref[0]).abs().max()) < 1e-5
        ms = bench.time_region(wl.step, 50)
        fwd, bwd = bench.time_region(wl.forward, 30), bench.time_region(wl.backward, 30)
        g = bench.capture_step_graph(wl.step)
        g.replay()
        gms = bench.time_region(g.replay, 50)
        del g
        graph_ms.setdefault(name, []).append(gms)
        print(f"== round {rnd} {name:16s} {opts}: eager {ms:.4f} ms  graph {gms:.4f} ms  fwd {fwd:.4f}  bwd {bwd:.4f}  bit-identical to first: {same}", flush=True)
        if rnd == 0 and name in DETAIL:
            lib.set_option("planes_overlap", 0)          # per-launch durations: every launch on one stream
            rec = lib.profile_launches(lambda: [wl.step() for _ in range(5)])
            n = len(rec) // 5
            print(f"     launches {n}, event sum {sum(t for _, t in rec) / 5:.4f} ms")
            for i in range(n):
                print(f"     {sum(rec[r * n + i][1] for r in range(5)) / 5 * 1e3:8.1f} us  {rec[i][0][:120]}")
            lib.set_option("planes_overlap", -1)
for k, v in BASE.items():
    lib.set_option(k, v)
for option, zero in (("cache_order", "order-0"), ("stream_policy", "policy-0")):
    if zero not in graph_ms:
        continue
    base = graph_ms[zero]
    print(f"== {option}: graph-replay ms per round; noise = the larger of the set's and {zero}'s spread over the rounds")
    for name, v in graph_ms.items():
        if not name.startswith(zero.split("-")[0] + "-"):
            continue
        gain, noise = sum(base) / len(base) - sum(v) / len(v), max(max(v) - min(v), max(base) - min(base))
        below = all(a < b for a, b in zip(v, base))
        print(f"   {name:20s} " + " ".join(f"{x:.4f}" for x in v) + f"  mean {sum(v) / len(v):.4f}  gain over {zero} {gain * 1e3:+6.1f} us  noise {noise * 1e3:4.1f} us"
              f"  below {zero} in every round: {below}  wins: {name != zero and below and gain > noise}")
