#!/usr/bin/env python3
"""Time the training input pipeline per batch at the recipe shape (B = 8 uint8 1024 x 2048 frames -> 769 x 769 crops) at the
recipe's smallest, middle and largest scale (0.7, 1.0, 2.1), three ways, and print one JSON line:

    fused   ccnet_amd.augment.DeviceAugment: one HIP gather from the packed frames (libccnet_augment.so)
    stock   the same result from stock device ops, per sample: F.interpolate's bilinear up-sample of the WHOLE frame
            (align_corners=False), round to a grey level, mean, pad, slice, flip; nearest resize and table lookup for the label
    host    a NumPy restatement of the reference's host route (dataset/datasets.py:173-210: 35 whole-image compares for the
            label ids, whole-frame resize, float32, mean, pad, crop, mirror), samples spread over --host-threads threads of the
            calling process.  The reference uses cv2 for the resize; this is context, not a measurement of cv2.

    python tools/augment_time.py [--batch 8] [--rounds 5] [--iters 2000] [--stock-iters 50] [--host-rounds 3] [--host-threads 8]

The frames are on the device before the clock starts for fused and stock alike (both need the same uint8 upload).  fused and
stock alternate in one process: per scale, `rounds` windows each in turn; the line reports the median window and its spread
(min, max).  Times are host wall clock around work that ends in a device synchronise.  The line also says how far the stock
route's float arithmetic is from the kernel's integer definition (share of image elements and labels that differ).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HS, WS, CROP = 1024, 2048, 769
MEAN = (104.00698793, 116.66876762, 122.67891434)
SCALES = ((7, 10), (10, 10), (21, 10))


def window(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def stock_sample(frame, label, p, table, mean):
    """One sample from stock device ops; frame uint8 (H, W, 3) R, G, B and label uint8 (H, W) on the device"""
    x = frame.permute(2, 0, 1)[None].float()
    # (the ATen ops behind F.interpolate, which take the size AND the scale: F.interpolate(scale_factor=f) floors the scaled size
    # where cv2 rounds it, and F.interpolate(size=...) maps coordinates by the size ratio where cv2 uses 1 / fx)
    f = p.num / p.den
    y = torch._C._nn.upsample_bilinear2d(x, (p.hz, p.wz), False, f, f)
    y = torch.floor(y + 0.5).flip(1) - mean                                  # grey levels, B, G, R, minus the mean
    t = torch._C._nn.upsample_nearest2d(label[None, None].float(), (p.hz, p.wz), f, f)
    t = table[t[0, 0].long()]
    hz, wz = y.shape[2:]
    y = F.pad(y, (0, max(CROP - wz, 0), 0, max(CROP - hz, 0)))
    t = F.pad(t, (0, max(CROP - wz, 0), 0, max(CROP - hz, 0)), value=255)
    y = y[0, :, p.h_off:p.h_off + CROP, p.w_off:p.w_off + CROP]
    t = t[p.h_off:p.h_off + CROP, p.w_off:p.w_off + CROP]
    return (y.flip(2), t.flip(1)) if p.mirror else (y, t)


def host_sample(frame, label, p, id_map, mean):
    """dataset/datasets.py:173-210 in NumPy for one decoded sample (frame B, G, R as cv2.imread gives it)"""
    out = label.copy()
    for k, v in id_map:                                                      # id2trainId: one whole-image compare per id
        out[label == k] = v
    hz, wz = p.hz, p.wz
    inv = np.float32(p.den / p.num)

    def taps(n_out, n_in):
        s = np.maximum((np.arange(n_out, dtype=np.float32) + 0.5) * inv - 0.5, 0)
        i0 = np.minimum(s.astype(np.int32), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), (s - i0).astype(np.float32)
    j0, j1, wy = taps(hz, frame.shape[0])
    i0, i1, wx = taps(wz, frame.shape[1])
    rows0, rows1 = frame[j0].astype(np.float32), frame[j1].astype(np.float32)
    rows = rows0 + (rows1 - rows0) * wy[:, None, None]
    left, right = rows[:, i0], rows[:, i1]
    image = np.floor(left + (right - left) * wx[None, :, None] + 0.5).astype(np.uint8)      # the uint8 cv2.resize returns
    sy = np.minimum((np.arange(hz) * p.den) // p.num, label.shape[0] - 1)
    sx = np.minimum((np.arange(wz) * p.den) // p.num, label.shape[1] - 1)
    out = out[sy][:, sx]
    image = image.astype(np.float32) - mean
    pad_h, pad_w = max(CROP - hz, 0), max(CROP - wz, 0)
    if pad_h or pad_w:
        image = np.pad(image, ((0, pad_h), (0, pad_w), (0, 0)))
        out = np.pad(out, ((0, pad_h), (0, pad_w)), constant_values=255)
    image = image[p.h_off:p.h_off + CROP, p.w_off:p.w_off + CROP].transpose(2, 0, 1)
    out = out[p.h_off:p.h_off + CROP, p.w_off:p.w_off + CROP]
    if p.mirror:
        image, out = image[:, :, ::-1], out[:, ::-1]
    return image.copy(), out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000, help="fused calls per window (about 0.1 s)")
    ap.add_argument("--stock-iters", type=int, default=50, help="stock batches per window (0.05 ... 0.2 s)")
    ap.add_argument("--host-rounds", type=int, default=3, help="host batches per scale (0: skip the host route)")
    ap.add_argument("--host-threads", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py measures on a HIP device; none found")
    from ccnet_amd import augment
    dev = torch.device("cuda:0")
    B = args.batch
    data = np.random.RandomState(0)
    frames = [data.randint(0, 256, (HS, WS, 3)).astype(np.uint8) for _ in range(B)]
    labels = [data.randint(0, 34, (HS, WS)).astype(np.uint8) for _ in range(B)]
    rng, np_rng = random.Random(0), np.random.RandomState(1)
    table_np = augment.CITYSCAPES_ID_TO_TRAINID
    table = torch.from_numpy(table_np.astype(np.int64)).to(dev)
    mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    aug = augment.DeviceAugment((CROP, CROP), MEAN, 255, table_np, "rgb")
    id_map = [(k, int(table_np[k])) for k in range(34)] + [(255, 255)]       # the reference's 35 entries, -1 as uint8
    frames_dev, labels_dev = [torch.from_numpy(f).to(dev) for f in frames], [torch.from_numpy(l).to(dev) for l in labels]
    rows = []
    for num, den in SCALES:
        params = [augment.draw_params(HS, WS, (CROP, CROP), scales=(num, 0, den), rng=rng, np_rng=np_rng) for _ in range(B)]
        fbuf, lbuf, desc = augment.pack(frames, labels, params, pin=True)
        fdev, ldev = fbuf.to(dev), lbuf.to(dev)
        keep = {}

        def fused():
            keep["fused"] = aug(fdev, ldev, desc)

        def stock():
            pairs = [stock_sample(f, l, p, table, mean) for f, l, p in zip(frames_dev, labels_dev, params)]
            keep["stock"] = torch.stack([a for a, _ in pairs]), torch.stack([b for _, b in pairs])

        for _ in range(args.warmup):
            fused()
            stock()
        torch.cuda.synchronize()
        img_diff = float((keep["fused"][0] != keep["stock"][0]).float().mean())
        lab_diff = float((keep["fused"][1] != keep["stock"][1]).float().mean())
        worst = float((keep["fused"][0] - keep["stock"][0]).abs().max())
        times = {"fused": [], "stock": []}
        for _ in range(args.rounds):
            times["fused"].append(window(fused, args.iters))
            times["stock"].append(window(stock, args.stock_iters))
        row = {"scale": f"{num}/{den}", "scaled": [params[0].hz, params[0].wz]}
        for name in ("fused", "stock"):
            row[name + "_ms"] = round(statistics.median(times[name]), 4)
            row[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
        row["stock_over_fused"] = round(row["stock_ms"] / row["fused_ms"], 1)
        row["stock_vs_fused"] = {"image_elements_differing": round(img_diff, 6), "max_abs": worst,
                                 "labels_differing": round(lab_diff, 6)}
        if args.host_rounds > 0:
            bgr = [f[:, :, ::-1] for f in frames]
            mean_np = np.array(MEAN, np.float32)
            host = []
            with ThreadPoolExecutor(args.host_threads) as pool:
                for _ in range(args.host_rounds):
                    t0 = time.perf_counter()
                    done = list(pool.map(lambda a: host_sample(*a, id_map, mean_np), zip(bgr, labels, params)))
                    host.append((time.perf_counter() - t0) * 1e3)
            row["host_numpy_ms"] = round(statistics.median(host), 1)
            row["host_vs_fused_image_elements_differing"] = round(
                float((np.stack([d[0] for d in done]) != keep["fused"][0].cpu().numpy()).mean()), 6)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del keep, fdev, ldev
    print(json.dumps({"metric": f"training input pipeline per batch, B={B} uint8 {HS}x{WS} frames -> {CROP}x{CROP} crops",
                      "unit": "ms per batch (median of %d windows, fused and stock alternated; host: %d batch(es) on %d threads)"
                              % (args.rounds, args.host_rounds, args.host_threads),
                      "device": torch.cuda.get_device_name(dev), "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
