"""Synthetic-data evaluation driver: the reference's ``evaluate.py`` (Cityscapes val mIoU) on seeded random images.

    model      ccnet_amd.segmodel.Seg_Model(num_classes, recurrence=R), random init (seeded) or --restore-from, eval mode;
               --abn device|inplace swaps its inplace_abn layers for the HIP twins (ccnet_amd.abn.convert_abn)
    data       image i: randn(1, 3, H, W), labels randint(0, C) with ~5 % set to 255, from a generator seeded with seed + i
    inference  SegEvaluator: the 8 zero-padded 769^2 tiles of a 1024 x 2048 image (--whole: the image itself), --flip adds
               the mirrored image's tiles; one net call per image, one HIP kernel for the score, argmax and confusion
    scales     --scales 0.75,1.0,1.25 evaluates every image at those scales (MultiScaleEvaluator, include/ccnet_mseval.h):
               per scale a gather kernel zooms, mirrors and cuts the tiles, the net runs over --tile-batch tiles at a time, and
               one kernel resamples the scale's score back and accumulates; the default 1.0 is the single-scale path above
    parallel   under torch.distributed.run rank r takes images r, r + world, ...; result() sums the confusion counts

Launch:   python -m ccnet_amd.eval_synthetic --images 8
          python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
                 -m ccnet_amd.eval_synthetic --images 8
Rank 0 prints one JSON line: images/s over all images (max wall time over ranks), the mean time per image split into the
net (tile cutting + forward) and the post-processing kernel (each side closed by a device synchronise), the mIoU, and the
route the criss-cross attention took.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def synthetic_image(i, H, W, num_classes, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed * 1_000_003 + i)
    image = torch.randn(1, 3, H, W, device=device, generator=g)
    label = torch.randint(0, num_classes, (1, H, W), device=device, generator=g)
    ignore = torch.rand(1, H, W, device=device, generator=g) < 0.05
    return image, label.masked_fill(ignore, 255)


def parse_scales(text):
    """"0.75,1.0,1.25" -> (0.75, 1.0, 1.25)."""
    scales = tuple(float(v) for v in str(text).split(",") if v.strip())
    if not scales or min(scales) <= 0:
        raise SystemExit(f"--scales {text!r}: a comma-separated list of positive numbers")
    return scales


def run(args, quiet=False):
    from .evaluate import MultiScaleEvaluator, SegEvaluator, all_reduce_confusion, mean_iou, shard_indices
    from .segmodel import Seg_Model, load_model

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("eval_synthetic runs on a HIP device; none found")
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("gloo")          # only the confusion counts and two timings travel
    torch.manual_seed(args.seed)                 # the same weights on every rank
    model = Seg_Model(args.num_classes, recurrence=args.recurrence)
    if args.restore_from:
        load_model(model, args.restore_from)
    if args.abn in ("device", "inplace"):
        from .abn import convert_abn
        convert_abn(model, args.abn)
    model = model.to(device).eval()
    if args.abn is not None:
        torch.cuda.reset_peak_memory_stats(device)
    routes = set()
    model.head.cca.register_forward_pre_hook(lambda m, inp: routes.add(m.route(inp[0])))
    scales = parse_scales(args.scales)
    if scales == (1.0,):
        ev = SegEvaluator(args.num_classes, tile_size=(args.tile, args.tile), whole=args.whole, flip=args.flip, device=device)
    else:
        ev = MultiScaleEvaluator(args.num_classes, scales=scales, tile_size=(args.tile, args.tile), whole=args.whole,
                                 flip=args.flip, tile_batch=args.tile_batch, device=device)

    def net(x):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.bf16):
            return model(x)

    mine = list(shard_indices(args.images, rank, world))
    net_s = post_s = 0.0
    with torch.no_grad():
        if args.warmup and mine:                 # first launches: code objects, MIOpen algorithm choice (counts reset below)
            image, label = synthetic_image(mine[0], args.height, args.width, args.num_classes, args.seed, device)
            ev.update(net, image, label)
            ev.reset()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in mine:
            image, label = synthetic_image(i, args.height, args.width, args.num_classes, args.seed, device)
            torch.cuda.synchronize()
            a = time.perf_counter()
            logits = ev.net_logits(net, image)
            torch.cuda.synchronize()
            b = time.perf_counter()
            ev.accumulate(logits, label, args.height, args.width)
            torch.cuda.synchronize()
            net_s += b - a
            post_s += time.perf_counter() - b
        elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed, net_s, post_s], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t[:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
    counts = all_reduce_confusion(ev.confusion).cpu()             # SegEvaluator.result()'s reduction, kept for the total
    res = mean_iou(counts)
    result = None
    if rank == 0:
        elapsed, net_s, post_s = (float(v) for v in t)
        n = max(args.images, 1)
        result = {
            "metric": "CCNet (ResNet-101 + RCCA R=%d) synthetic evaluation, images/s" % args.recurrence,
            "value": round(args.images / elapsed, 3) if elapsed > 0 else None, "unit": "images/s", "n_gpus": world,
            "images": args.images, "ms_per_image": round(elapsed * world / n * 1e3, 2),
            "net_ms_per_image": round(net_s / n * 1e3, 2), "post_ms_per_image": round(post_s / n * 1e3, 3),
            "meanIU": round(res["meanIU"], 6), "route": sorted(routes),
            "dtype": "bf16-autocast" if args.bf16 else "f32", "data": "synthetic",
            "config": {"image": [3, args.height, args.width], "mode": "whole" if args.whole else "sliding",
                       "tile": None if args.whole else args.tile, "tiles": len(ev.geometry(args.height, args.width)[0]),
                       "flip": args.flip, "num_classes": args.num_classes,
                       "weights": "restored" if args.restore_from else "random"},
            "counted_pixels": int(counts.sum()),
        }
        if scales != (1.0,):
            result["config"].update(scales=list(scales), tile_batch=args.tile_batch,
                                    tiles=[len(g[2]) for g in ev.geometry(args.height, args.width)])
        if args.abn is not None:
            result["abn"] = args.abn
            result["max_memory_allocated_mb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
        if args.dump_confusion:
            torch.save(counts, args.dump_confusion)
        if not quiet:
            print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return result


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=769, help="square tile of the sliding window (evaluate.py: 769)")
    ap.add_argument("--whole", action="store_true", help="one tile equal to the image (evaluate.py --whole)")
    ap.add_argument("--flip", action="store_true", help="average with the horizontally mirrored image's prediction")
    ap.add_argument("--scales", type=str, default="1.0", help="comma-separated scales, e.g. 0.75,1.0,1.25 (multi-scale evaluation)")
    ap.add_argument("--tile-batch", type=int, default=8, help="multi-scale: tiles per net call")
    ap.add_argument("--recurrence", type=int, default=2)
    ap.add_argument("--num-classes", type=int, default=19)
    ap.add_argument("--bf16", action="store_true", help="run the net under bf16 autocast (the kernel reads its output as fp32)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--abn", choices=("torch", "device", "inplace"), default=None,
                    help="normalisation layers: torch (the default: the stock inplace_abn restatement), device or inplace "
                         "(the HIP ABN kernels, ccnet_amd.abn.convert_abn); when given, the JSON line also reports abn and "
                         "max_memory_allocated_mb")
    ap.add_argument("--restore-from", type=str, default=None, help="checkpoint for Seg_Model (segmodel.load_model)")
    ap.add_argument("--warmup", type=int, default=1, help="1: one untimed, uncounted image first")
    ap.add_argument("--dump-confusion", type=str, default=None, help="tests: torch.save the reduced confusion matrix here")
    return ap


if __name__ == "__main__":
    run(build_parser().parse_args())
