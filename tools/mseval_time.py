#!/usr/bin/env python3
"""Time the multi-scale evaluation post-processing of one 1024 x 2048 image with 19 classes, tiles of 769^2, scales
0.75 / 1.0 / 1.25 and the flipped pass, from synthetic (T + T, 19, 97, 97) tile logits per scale (the net is out of the
picture): the device route (ccnet_amd.evaluate, libccnet_mseval.so: one accumulate kernel per scale, which samples the
low-resolution logits, resamples the scale's score back to the image, sums, and on the last scale divides, takes the argmax and
counts) against the reference-style host route (evaluate.py's predict_multiscale: ndimage.zoom of the image per scale on the
host, every tile up-sampled on the device and copied to the host, float64 NHWC accumulation, the flipped pass mirrored back,
the zoom back to the image that the reference lacks, the mean, np.argmax, np.bincount).  Also times the gather kernel that
replaces the host zoom (zoom + flip + cut + pad of every tile of every scale).  Prints one JSON line.

    python tools/mseval_time.py [--scales 0.75,1.0,1.25] [--iters 20] [--warmup 3] [--host-iters 1]

Times are host wall clock around work that ends in a device synchronise, after warm-up.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_oracle as O  # noqa: E402
import mseval_oracle as M  # noqa: E402

H, W, TILE, C = 1024, 2048, (769, 769), 19


def host_zoom(a, zoom):
    """ndimage.zoom(order=1, prefilter=False) where scipy is installed, else its numpy restatement (tests/mseval_oracle)."""
    try:
        from scipy import ndimage
        return ndimage.zoom(a, zoom, order=1, prefilter=False)
    except ImportError:
        out_h, out_w = (int(round(n * z)) for n, z in zip(a.shape[2:], zoom[2:]))
        return M.resample(a, out_h, out_w).astype(a.dtype)


def time_it(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scales", type=str, default="0.75,1.0,1.25")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mseval_time.py measures on a HIP device; none found")
    from ccnet_amd.evaluate import accumulate_call, scale_geometry, scaled_tiles_call
    dev = torch.device("cuda:0")
    scales = [float(s) for s in args.scales.split(",")]
    geo = [scale_geometry(H, W, s, TILE, False) for s in scales]
    rng = np.random.default_rng(0)
    logits = [torch.from_numpy((rng.standard_normal((2 * len(g[2]), C, 97, 97)) * 3).astype(np.float32)).to(dev) for g in geo]
    image_np, label_np = O.make_case_inputs(1, H, W, C, seed=0)
    image, label = torch.from_numpy(image_np).to(dev), torch.from_numpy(label_np).to(dev)
    pred = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
    score = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
    conf = torch.zeros((C, C), dtype=torch.int64, device=dev)

    def device_post():
        for i, (lg, (Hs, Ws, origins, tile)) in enumerate(zip(logits, geo)):
            last = i == len(geo) - 1
            accumulate_call(lg, origins, True, 1, tile, Hs, Ws, H, W, score_in=score if i else None,
                            score_out=None if last else score, divide_by=len(geo) if last else 0,
                            labels=label if last else None, pred=pred if last else None, confusion=conf if last else None)

    def device_gather():
        for Hs, Ws, origins, tile in geo:
            for first in range(0, 2 * len(origins), 8):
                scaled_tiles_call(image, Hs, Ws, origins, tile, True, first, min(8, 2 * len(origins) - first))

    def host_route():
        full = np.zeros((1, H, W, C))
        for s, lg, (Hs, Ws, origins, tile) in zip(scales, logits, geo):
            scaled = host_zoom(image_np, (1.0, 1.0, s, s))                        # evaluate.py:166 (fed to the net there)
            assert scaled.shape[2:] == (Hs, Ws)
            T = len(origins)
            passes = []
            for p in range(2):
                acc = np.zeros((1, Hs, Ws, C))
                count = np.zeros((1, Hs, Ws, C))
                for t, (y1, x1) in enumerate(origins):
                    y2, x2 = min(y1 + tile[0], Hs), min(x1 + tile[1], Ws)
                    up = F.interpolate(lg[p * T + t:p * T + t + 1], size=tile, mode="bilinear", align_corners=True)
                    up = up.cpu().numpy().transpose(0, 2, 3, 1)
                    count[0, y1:y2, x1:x2] += 1
                    acc[:, y1:y2, x1:x2] += up[0, 0:y2 - y1, 0:x2 - x1, :]
                passes.append(acc / count)
            probs = 0.5 * (passes[0] + passes[1][:, :, ::-1, :])
            back = host_zoom(probs.transpose(0, 3, 1, 2), (1.0, 1.0, H / Hs, W / Ws))
            full += back.transpose(0, 2, 3, 1)
        full /= len(scales)
        seg_pred = np.asarray(np.argmax(full, axis=3), dtype=np.uint8)
        gt = label.cpu().numpy()
        keep = gt != 255
        cm = np.bincount((gt[keep] * C + seg_pred[keep]).astype("int32"), minlength=C * C)[:C * C].reshape(C, C)
        return seg_pred, cm, full

    post_ms = time_it(device_post, args.iters, args.warmup)
    gather_ms = time_it(device_gather, args.iters, args.warmup)
    host_ms = time_it(host_route, args.host_iters, 0)

    conf.zero_()
    device_post()
    torch.cuda.synchronize()
    host_pred, host_cm, full = host_route()
    differs = pred.cpu().numpy() != host_pred
    top2 = np.sort(full, axis=3)
    gap = top2[..., -1] - top2[..., -2]
    bound = 1e-5 * max(float(lg.abs().max()) for lg in logits)
    if np.any(gap[differs] >= bound):
        raise SystemExit("the device and the host route disagree on a prediction away from a near tie")
    print(json.dumps({"metric": "multi-scale evaluation post-processing of one 1024x2048 image, tiles of 769^2, 19 classes, "
                                "flip (per-scale score, zoom back, mean, argmax, confusion)", "unit": "ms per image",
                      "scales": scales, "tiles_per_scale": [2 * len(g[2]) for g in geo],
                      "device_ms": round(post_ms, 4), "device_gather_tiles_ms": round(gather_ms, 4),
                      "host_path_ms": round(host_ms, 1), "speedup": round(host_ms / post_ms, 1),
                      "pred_agreement": float(1.0 - differs.mean()), "pred_differs_only_at_near_ties": True,
                      "confusion_equal": bool(np.array_equal(conf.cpu().numpy(), host_cm)),
                      "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
