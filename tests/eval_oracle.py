"""numpy restatement of the reference's sliding-window evaluation (evaluate.py:95-195: pad_image, predict_sliding,
predict_whole, get_confusion_matrix and main's argmax / ignore mask), with the project's divergences (each image its own
tiles, the flipped pass mirrored back along W, at least one tile per axis).  Everything here is test infrastructure.

:func:`sliding_scores` restates the per-pixel semantics of include/ccnet_eval.h: every tile's logits are up-sampled with
PyTorch's bilinear, align_corners=True arithmetic in fp32, and the cropped tiles are accumulated and divided in float64 like
the reference.  :func:`host_path` is the reference-style host route tools/eval_time.py times.
"""
from math import ceil

import numpy as np


def reference_tile_grid(H, W, tile_size):
    """evaluate.py:104-124 as written: the origins (y1, x1), possibly none."""
    stride = ceil(tile_size[0] * (1 - 1 / 3))
    rows = int(ceil((H - tile_size[0]) / stride) + 1)
    cols = int(ceil((W - tile_size[1]) / stride) + 1)
    out = []
    for row in range(rows):
        for col in range(cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2, y2 = min(x1 + tile_size[1], W), min(y1 + tile_size[0], H)
            out.append((max(int(y2 - tile_size[0]), 0), max(int(x2 - tile_size[1]), 0)))
    return out


def _axis(n_in, n_out, idx):
    """upsample_bilinear2d's source index, its neighbour and the two lambdas (fp32), for output positions ``idx``."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    r = np.float32(scale) * idx.astype(np.float32)
    i0 = r.astype(np.int64)
    l1 = (r - i0.astype(np.float32)).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def upsample(logits, out_h, out_w, rows=None, cols=None):
    """F.interpolate(logits, (out_h, out_w), mode="bilinear", align_corners=True) in fp32, on (..., h, w); ``rows`` /
    ``cols`` select output positions (default: all)."""
    h, w = logits.shape[-2:]
    rows = np.arange(out_h) if rows is None else rows
    cols = np.arange(out_w) if cols is None else cols
    y0, y1, ly0, ly1 = _axis(h, out_h, rows)
    x0, x1, lx0, lx1 = _axis(w, out_w, cols)
    a = logits.astype(np.float32)
    r0 = a[..., y0, :]
    r1 = a[..., y1, :]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    return (ly0[:, None] * top + ly1[:, None] * bot).astype(np.float32)


def _pass(tiles, origins, tile_size, H, W):
    """One pass of predict_sliding over (N, T, C, h, w) tile logits -> (N, C, H, W) float64."""
    N, T, C = tiles.shape[:3]
    full = np.zeros((N, C, H, W), np.float64)
    count = np.zeros((H, W), np.float64)
    for t, (y1, x1) in enumerate(origins):
        y2, x2 = min(y1 + tile_size[0], H), min(x1 + tile_size[1], W)
        up = upsample(tiles[:, t], tile_size[0], tile_size[1], np.arange(y2 - y1), np.arange(x2 - x1))
        full[:, :, y1:y2, x1:x2] += up
        count[y1:y2, x1:x2] += 1
    return full / count


def sliding_scores(tile_logits, origins, tile_size, H, W, flip=False):
    """The (N, C, H, W) float64 score map from (N, T + T_flip, C, h, w) tile logits."""
    T = len(origins)
    probs = _pass(tile_logits[:, :T], origins, tile_size, H, W)
    if flip:
        probs = 0.5 * (probs + _pass(tile_logits[:, T:], origins, tile_size, H, W)[..., ::-1])
    return probs


def argmax(probs):
    """np.argmax over C as uint8 (main(): seg_pred)."""
    return np.asarray(np.argmax(probs, axis=1), dtype=np.uint8)


def confusion(label, pred, C, ignore_label=255):
    """get_confusion_matrix after main()'s ignore mask, as int64 [label, pred]; labels outside [0, C) are not counted."""
    gt = np.asarray(label, np.int64).ravel()
    pr = np.asarray(pred, np.int64).ravel()
    keep = (gt != ignore_label) & (gt >= 0) & (gt < C)
    return np.bincount(gt[keep] * C + pr[keep], minlength=C * C).reshape(C, C).astype(np.int64)


def top2_gap(probs):
    """Per pixel, the best score minus the second best (over axis 1)."""
    s = np.sort(probs, axis=1)
    return s[:, -1] - s[:, -2]


def host_path(up_tiles_gpu_to_host, origins, tile_size, H, W, C, label, ignore_label=255):
    """The reference-style host route of one image (evaluate.py:126-143 + main): ``up_tiles_gpu_to_host(t)`` returns tile
    t's (1, C, th, tw) up-sampled logits as host numpy; NHWC float64 accumulation, division, argmax, bincount."""
    full = np.zeros((1, H, W, C))
    count = np.zeros((1, H, W, C))
    for t, (y1, x1) in enumerate(origins):
        y2, x2 = min(y1 + tile_size[0], H), min(x1 + tile_size[1], W)
        pred = up_tiles_gpu_to_host(t).transpose(0, 2, 3, 1)[0, 0:y2 - y1, 0:x2 - x1, :]
        count[0, y1:y2, x1:x2] += 1
        full[:, y1:y2, x1:x2] += pred
    full /= count
    seg_pred = np.asarray(np.argmax(full, axis=3), dtype=np.uint8)
    gt = np.asarray(label, np.int64)
    keep = gt != ignore_label
    index = (gt[keep] * C + seg_pred[keep]).astype("int32")
    counts = np.bincount(index)
    cm = np.zeros((C, C))
    n = min(len(counts), C * C)
    cm.ravel()[:n] = counts[:n]
    return seg_pred, cm


# ---- seeded inputs and the toy net of the fixtures (tests/golden/make_eval_golden.py) ----
def make_case_inputs(N, H, W, C, seed, ignore_frac=0.05, out_of_range_frac=0.01):
    """Seeded fp32 images (N, 3, H, W) and int64 labels (N, H, W): uniform classes, ~5 % 255, ~1 % in [C, 255)."""
    rng = np.random.default_rng(seed)
    image = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    label = rng.integers(0, C, (N, H, W)).astype(np.int64)
    label[rng.random((N, H, W)) < ignore_frac] = 255
    if C < 255:
        odd = rng.random((N, H, W)) < out_of_range_frac
        label[odd] = rng.integers(C, 255, int(odd.sum()))
    return image, label


def make_toy_net(C, seed):
    """A stride-8 net (97 x 97 logits for a 769 x 769 input, ceil(n / 8) in general) that returns a list, as CCNet does."""
    import torch

    class ToyNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.conv = torch.nn.Conv2d(3, C, 3, stride=8, padding=1)
            with torch.no_grad():
                self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.5)
                self.conv.bias.copy_(torch.randn(C, generator=g) * 0.1)

        def forward(self, x):
            y = self.conv(x)
            return [y, y]

    return ToyNet().eval()


def load_fixture(path):
    """A fixture (tests/golden/eval_*.npz) with its image, labels and toy net regenerated from the stored seed."""
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    H, W, C = (int(fx[k]) for k in ("H", "W", "C"))
    fx["image"], fx["label"] = make_case_inputs(1, H, W, C, int(fx["seed"]))
    fx["net"] = make_toy_net(C, int(fx["seed"]))
    fx["whole"] = bool(fx["whole"])
    fx["tile"] = (H, W) if fx["whole"] else tuple(int(v) for v in fx["tile"])
    return fx


def fixture_tiles(fx, origins, flip=False):
    """The toy net's (1, T + T_flip, C, h, w) fp32 outputs over the fixture's zero-padded tiles, on the CPU."""
    import torch
    th, tw = fx["tile"]
    img = fx["image"]
    H, W = img.shape[2:]
    views = [img, img[..., ::-1]] if flip else [img]
    outs = []
    with torch.no_grad():
        for v in views:
            for y1, x1 in origins:
                t = v[:, :, y1:y1 + th, x1:x1 + tw]
                t = np.pad(t, ((0, 0), (0, 0), (0, th - t.shape[2]), (0, tw - t.shape[3])))
                outs.append(fx["net"](torch.from_numpy(np.ascontiguousarray(t)))[0].numpy())
    return np.stack(outs, 1).astype(np.float32)


def check_against_fixture(fx, probs=None, pred=None, conf=None, rel=1e-5):
    """The numerics bar of a device (or emulated, or oracle) result against a reference fixture.

    Score map (N, C, H, W) within ``rel`` x max|logit| of the fixture's sample; pred identical except at pixels whose top-2
    gap (in the fixture's scores, recomputed by the oracle) is below that bound; confusion off by at most one count per such
    pixel in each of the two cells it touches, identical when there is none.  Returns the number of such pixels that differ."""
    tol = rel * float(fx["max_abs_logit"])
    if probs is not None:
        got = np.asarray(probs, np.float64).ravel()[fx["probs_index"]]
        err = float(np.abs(got - fx["probs_sample"]).max())
        assert err <= tol, (err, tol)
    n_diff = 0
    if pred is not None:
        diff = np.asarray(pred) != fx["pred"]
        n_diff = int(diff.sum())
        if n_diff:
            origins = [(0, 0)] if fx["whole"] else reference_tile_grid(fx["H"], fx["W"], fx["tile"])
            ref = sliding_scores(fixture_tiles(fx, origins), origins, fx["tile"], int(fx["H"]), int(fx["W"]))
            gap = top2_gap(ref)
            assert np.all(gap[diff] < tol), gap[diff]
        if conf is not None:
            d = np.abs(np.asarray(conf, np.int64) - fx["confusion"])
            assert int(d.sum()) <= 2 * n_diff and int(d.max(initial=0)) <= n_diff, (int(d.sum()), n_diff)
    elif conf is not None:
        np.testing.assert_array_equal(np.asarray(conf, np.int64), fx["confusion"])
    return n_diff
