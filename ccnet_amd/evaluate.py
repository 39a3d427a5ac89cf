"""Segmentation evaluation on the device: the reference's ``evaluate.py`` (predict_sliding / predict_whole, argmax,
get_confusion_matrix, mIoU; evaluate.py:102-195, 262-274).

The reference up-samples every tile's logits to the tile size, copies them to the host and accumulates a float64 NHWC score
map there before ``np.argmax`` and ``np.bincount``.  Here one HIP kernel (include/ccnet_eval.h, libccnet_eval.so) samples
the tiles' 1/8-resolution logits directly, averages, takes the argmax and counts the confusion matrix on the device, so
nothing is copied to the host per image.  There is no CPU fallback.
"""
from __future__ import annotations

from math import ceil
from typing import List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _eval_lib, _mseval_lib

__all__ = ["tile_grid", "predict_sliding", "predict_whole", "SegEvaluator", "shard_indices", "mean_iou",
           "all_reduce_confusion", "scaled_size", "predict_multiscale", "MultiScaleEvaluator"]


def tile_grid(H: int, W: int, tile_size: Sequence[int]) -> List[Tuple[int, int]]:
    """The reference's tile origins (y1, x1), rows then columns (evaluate.py:104-124): stride ceil(tile_h * (1 - 1/3)) on
    both axes, the last tile of a row / column pulled back inside the image.  Unlike the reference, at least one row and
    one column even where its formula yields none (an image smaller than the tile by a stride or more)."""
    th, tw = int(tile_size[0]), int(tile_size[1])
    overlap = 1 / 3
    stride = ceil(th * (1 - overlap))
    rows = max(int(ceil((H - th) / stride) + 1), 1)
    cols = max(int(ceil((W - tw) / stride) + 1), 1)
    out = []
    for row in range(rows):
        for col in range(cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2, y2 = min(x1 + tw, W), min(y1 + th, H)
            out.append((max(int(y2 - th), 0), max(int(x2 - tw), 0)))
    return out


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ccnet_amd.evaluate: inputs must be HIP device tensors (there is no CPU fallback for the "
                               "evaluation kernel)")


def cut_tiles(image: torch.Tensor, origins, tile_size, flip: bool) -> torch.Tensor:
    """(N, 3, H, W) -> (N * (T + T_flip), 3, th, tw): for each image its T zero-padded tiles (pad_image, evaluate.py:95-100),
    then, with ``flip``, the same tiles of its horizontally flipped copy."""
    th, tw = int(tile_size[0]), int(tile_size[1])
    H, W = image.shape[2:]
    views = [image, image.flip(-1)] if flip else [image]
    per = []
    for v in views:
        for y1, x1 in origins:
            t = v[:, :, y1:min(y1 + th, H), x1:min(x1 + tw, W)]
            per.append(F.pad(t, (0, tw - t.shape[3], 0, th - t.shape[2])))
    return torch.stack(per, 1).reshape(-1, image.shape[1], th, tw)


def run_net(net, tiles: torch.Tensor) -> torch.Tensor:
    """The net over a batch of tiles; ``[0]`` of a list output (evaluate.py:131-132), as contiguous fp32."""
    out = net(tiles)
    if isinstance(out, (list, tuple)):
        out = out[0]
    return out.to(torch.float32).contiguous()


def sliding_call(logits, origins, flip, N, tile_size, H, W, labels=None, ignore_label=255, probs=None, pred=None,
                 confusion=None):
    """One ccnet_eval_sliding_f32 launch on the current stream.  ``logits`` (N * (T + T_flip), C, h, w) fp32, ``labels``
    (N, H, W) int64, ``probs`` (N, C, H, W) fp32, ``pred`` (N, H, W) uint8, ``confusion`` (C, C) int64 (it needs labels), all
    contiguous: anything else raises before the launch, nothing is converted or copied."""
    _require_device(logits, labels, probs, pred, confusion)
    lib = _eval_lib.get_lib()
    T = len(origins)
    if T > _eval_lib.MAX_TILES:
        raise RuntimeError(f"ccnet_amd.evaluate: {T} tiles, the kernel takes at most {_eval_lib.MAX_TILES}")
    if logits.dim() != 4:
        raise RuntimeError(f"ccnet_amd.evaluate: logits must be a 4-d (N * tiles, C, h, w) tensor, got {tuple(logits.shape)}")
    C, h, w = logits.shape[1:]
    want = {"logits": (logits, (N * T * (2 if flip else 1), C, h, w), torch.float32),
            "labels": (labels, (N, H, W), torch.int64), "probs": (probs, (N, C, H, W), torch.float32),
            "pred": (pred, (N, H, W), torch.uint8), "confusion": (confusion, (C, C), torch.int64)}
    for name, (t, shape, dtype) in want.items():                          # the kernel indexes raw pointers by these shapes
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
            raise RuntimeError(f"ccnet_amd.evaluate: {name} must be a contiguous {dtype} tensor of shape {shape}, "
                               f"got {t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else ", not contiguous"))
    if confusion is not None and labels is None:
        raise RuntimeError("ccnet_amd.evaluate: confusion needs labels")
    y1x1 = _eval_lib.origins_array(origins)
    ptr = lambda t: None if t is None else t.data_ptr()                  # noqa: E731
    lib.check(lib.ccnet_eval_sliding_f32(logits.data_ptr(), T, T if flip else 0, y1x1, N, C, h, w, int(tile_size[0]),
                                         int(tile_size[1]), H, W, ptr(labels), int(ignore_label), ptr(probs), ptr(pred),
                                         ptr(confusion), _stream(logits.device)), "ccnet_eval_sliding_f32")


def _predict(net, image, tile_size, origins, flip):
    _require_device(image)
    N, _, H, W = image.shape
    logits = run_net(net, cut_tiles(image, origins, tile_size, flip))
    probs = torch.empty((N, logits.shape[1], H, W), dtype=torch.float32, device=image.device)
    sliding_call(logits, origins, flip, N, tile_size, H, W, probs=probs)
    return probs


@torch.no_grad()
def predict_sliding(net, image, tile_size, classes, flip=False):
    """(N, C, H, W) fp32 device score map: the values of the reference's predict_sliding (which returns (N, H, W, C) float64
    numpy), each image from its own tiles.  ``flip`` averages with the mirrored image's map (mirrored back along W)."""
    origins = tile_grid(image.shape[2], image.shape[3], tile_size)
    probs = _predict(net, image, tile_size, origins, flip)
    if probs.shape[1] != classes:
        raise RuntimeError(f"predict_sliding: the net gives {probs.shape[1]} classes, {classes} expected")
    return probs


@torch.no_grad()
def predict_whole(net, image, flip=False):
    """predict_whole (evaluate.py:145-153): the net on the whole image, up-sampled to it; one tile of the call above."""
    H, W = image.shape[2:]
    return _predict(net, image, (H, W), [(0, 0)], flip)


def mean_iou(confusion) -> dict:
    """evaluate.py:268-274: IU = tp / max(1, pos + res - tp), averaged over all C classes."""
    cm = confusion.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(confusion) else np.asarray(confusion, np.float64)
    pos, res, tp = cm.sum(1), cm.sum(0), np.diag(cm)
    iu = tp / np.maximum(1.0, pos + res - tp)
    return {"meanIU": float(iu.mean()), "IU_array": iu}


def all_reduce_confusion(confusion: torch.Tensor) -> torch.Tensor:
    """The sum of every rank's matrix when a default process group with world > 1 is up (engine.all_reduce_tensor,
    norm=False), else the matrix itself.  Over gloo the sum travels through a CPU copy."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return confusion
    t = confusion.detach().clone()
    if dist.get_backend() == "gloo":
        t = t.cpu()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.to(confusion.device)


def shard_indices(num_images: int, rank: int, world: int) -> range:
    """Images rank, rank + world, ...: every image exactly once over the ranks (no DistributedSampler padding)."""
    return range(rank, num_images, world)


class SegEvaluator:
    """Accumulates the confusion matrix of a segmentation net over batches of (image, label), on the device.

    ``update(net, image, label)`` cuts the batch's tiles (and its flipped copy's), runs the net once over all of them,
    and counts prediction against label in one kernel; it returns the uint8 (N, H, W) prediction.  ``result()`` returns
    ``{"meanIU", "IU_array"}`` over every rank of the default process group."""

    def __init__(self, num_classes, ignore_label=255, tile_size=(769, 769), whole=False, flip=False, device=None):
        if not 1 <= num_classes <= _eval_lib.MAX_CLASSES:
            raise ValueError(f"SegEvaluator: num_classes {num_classes} outside [1, {_eval_lib.MAX_CLASSES}]")
        self.num_classes, self.ignore_label = int(num_classes), int(ignore_label)
        self.tile_size, self.whole, self.flip = (int(tile_size[0]), int(tile_size[1])), bool(whole), bool(flip)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.confusion = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)

    def geometry(self, H, W):
        """(tile origins, tile size) for an H x W image."""
        if self.whole:
            return [(0, 0)], (H, W)
        return tile_grid(H, W, self.tile_size), self.tile_size

    @torch.no_grad()
    def net_logits(self, net, image):
        """The net's fp32 (N * (T + T_flip), C, h, w) outputs over every tile of the batch."""
        _require_device(image)
        origins, tile = self.geometry(image.shape[2], image.shape[3])
        if len(origins) > _eval_lib.MAX_TILES:
            raise RuntimeError(f"SegEvaluator: {len(origins)} tiles, the kernel takes at most {_eval_lib.MAX_TILES}")
        return run_net(net, cut_tiles(image, origins, tile, self.flip))

    @torch.no_grad()
    def accumulate(self, logits, label, H, W):
        """pred and confusion counts from net_logits' output; returns the uint8 (N, H, W) prediction.  ``logits`` must be what
        net_logits returns, contiguous fp32 (N * (T + T_flip), C, h, w): a channels_last or sliced tensor raises, as in
        MultiScaleEvaluator."""
        _require_device(logits, label, self.confusion)
        if logits.shape[1] != self.num_classes:
            raise RuntimeError(f"SegEvaluator: the net gives {logits.shape[1]} classes, {self.num_classes} expected")
        N = label.shape[0]
        origins, tile = self.geometry(H, W)
        pred = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device)
        sliding_call(logits, origins, self.flip, N, tile, H, W, labels=label.to(torch.int64).contiguous(),
                     ignore_label=self.ignore_label, pred=pred, confusion=self.confusion)
        return pred

    def update(self, net, image, label):
        if label.shape != (image.shape[0],) + tuple(image.shape[2:]):
            raise RuntimeError(f"SegEvaluator: image {tuple(image.shape)} and label {tuple(label.shape)} do not match")
        return self.accumulate(self.net_logits(net, image), label, image.shape[2], image.shape[3])

    def reset(self):
        self.confusion.zero_()

    def result(self):
        return mean_iou(all_reduce_confusion(self.confusion))


# ---------------------------------------------------------------------------------------------------------------------
# multi-scale evaluation (the reference's predict_multiscale, evaluate.py:155-175; semantics in include/ccnet_mseval.h)
# ---------------------------------------------------------------------------------------------------------------------
def scaled_size(H: int, W: int, s: float) -> Tuple[int, int]:
    """(Hs, Ws) of ndimage.zoom(image, (1, 1, s, s)): round half to even of H * s and W * s (at least one pixel)."""
    return max(int(round(H * float(s))), 1), max(int(round(W * float(s))), 1)


def scale_geometry(H, W, s, tile_size, whole):
    """(Hs, Ws, tile origins on the scaled image, tile size) of one scale."""
    Hs, Ws = scaled_size(H, W, s)
    if whole:
        return Hs, Ws, [(0, 0)], (Hs, Ws)
    tile = (int(tile_size[0]), int(tile_size[1]))
    return Hs, Ws, tile_grid(Hs, Ws, tile), tile


def _check_tiles(T, who):
    if T > _mseval_lib.MAX_TILES:
        raise RuntimeError(f"{who}: {T} tiles at one scale, the kernels take at most {_mseval_lib.MAX_TILES}")


def scaled_tiles_call(image, Hs, Ws, origins, tile_size, flip, first=0, count=None, out=None):
    """One ccnet_mseval_tiles_f32 launch: entries [first, first + count) of every image's T (+ T with ``flip``) zero-padded
    tiles of the image zoomed to (Hs, Ws), as (N, count, Cin, th, tw) fp32 (written into ``out`` when given); the zoomed image
    is never written."""
    _require_device(image, out)
    lib = _mseval_lib.get_lib()
    image = image.to(torch.float32).contiguous()
    N, Cin, H, W = image.shape
    T = len(origins)
    _check_tiles(T, "ccnet_amd.evaluate")
    count = T * (2 if flip else 1) - first if count is None else count
    shape = (N, count, Cin, int(tile_size[0]), int(tile_size[1]))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError(f"ccnet_amd.evaluate: out must be a contiguous fp32 tensor of shape {shape}")
    y1x1 = _mseval_lib.origins_array(origins)
    lib.check(lib.ccnet_mseval_tiles_f32(image.data_ptr(), N, Cin, H, W, Hs, Ws, T, T if flip else 0, y1x1, int(tile_size[0]),
                                         int(tile_size[1]), first, count, out.data_ptr(), _stream(image.device)),
              "ccnet_mseval_tiles_f32")
    return out


def accumulate_call(logits, origins, flip, N, tile_size, Hs, Ws, H, W, score_in=None, score_out=None, divide_by=0, labels=None,
                    ignore_label=255, pred=None, confusion=None):
    """One ccnet_mseval_accumulate_f32 launch on the current stream: this scale's score resampled to (H, W), added to
    ``score_in``, divided by ``divide_by`` when > 0; ``logits`` (N * (T + T_flip), C, h, w) fp32."""
    _require_device(logits, score_in, score_out, labels, pred, confusion)
    lib = _mseval_lib.get_lib()
    T = len(origins)
    _check_tiles(T, "ccnet_amd.evaluate")
    C, h, w = logits.shape[1:]
    want = {"logits": (logits, (N * T * (2 if flip else 1), C, h, w), torch.float32),
            "score_in": (score_in, (N, C, H, W), torch.float32), "score_out": (score_out, (N, C, H, W), torch.float32),
            "labels": (labels, (N, H, W), torch.int64), "pred": (pred, (N, H, W), torch.uint8),
            "confusion": (confusion, (C, C), torch.int64)}
    for name, (t, shape, dtype) in want.items():                          # the kernel indexes raw pointers by these shapes
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
            raise RuntimeError(f"ccnet_amd.evaluate: {name} must be a contiguous {dtype} tensor of shape {shape}, "
                               f"got {t.dtype} {tuple(t.shape)}")
    y1x1 = _mseval_lib.origins_array(origins)
    ptr = lambda t: None if t is None else t.data_ptr()                  # noqa: E731
    lib.check(lib.ccnet_mseval_accumulate_f32(logits.data_ptr(), T, T if flip else 0, y1x1, N, C, h, w, int(tile_size[0]),
                                              int(tile_size[1]), Hs, Ws, H, W, ptr(score_in), ptr(score_out), int(divide_by),
                                              ptr(labels), int(ignore_label), ptr(pred), ptr(confusion),
                                              _stream(logits.device)), "ccnet_mseval_accumulate_f32")


def scale_logits(net, image, Hs, Ws, origins, tile_size, flip, tile_batch=8):
    """The net's fp32 (N * (T + T_flip), C, h, w) outputs over every tile of the image zoomed to (Hs, Ws), the net run over
    about ``tile_batch`` tiles at a time (only the small logits are kept)."""
    N = image.shape[0]
    total = len(origins) * (2 if flip else 1)
    step = max(int(tile_batch) // N, 1)
    logits = None
    for first in range(0, total, step):
        count = min(step, total - first)
        out = run_net(net, scaled_tiles_call(image, Hs, Ws, origins, tile_size, flip, first, count).flatten(0, 1))
        if logits is None:
            logits = torch.empty((N, total) + tuple(out.shape[1:]), dtype=torch.float32, device=out.device)
        logits[:, first:first + count] = out.unflatten(0, (N, count))
    return logits.flatten(0, 1)


@torch.no_grad()
def predict_multiscale(net, image, tile_size, scales, classes, flip_evaluation=False, whole=False, tile_batch=8):
    """(N, C, H, W) fp32 device score map of the reference's predict_multiscale, with the zoom back to (H, W) that it lacks
    (include/ccnet_mseval.h step 5): the mean over ``scales`` of the per-scale sliding-window (``whole``: whole-image) scores."""
    _require_device(image)
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError("predict_multiscale: no scales")
    N, _, H, W = image.shape
    score = None
    for i, s in enumerate(scales):
        Hs, Ws, origins, tile = scale_geometry(H, W, s, tile_size, whole)
        logits = scale_logits(net, image, Hs, Ws, origins, tile, flip_evaluation, tile_batch)
        if logits.shape[1] != classes:
            raise RuntimeError(f"predict_multiscale: the net gives {logits.shape[1]} classes, {classes} expected")
        if score is None:
            score = torch.empty((N, classes, H, W), dtype=torch.float32, device=image.device)
        accumulate_call(logits, origins, flip_evaluation, N, tile, Hs, Ws, H, W, score_in=score if i else None,
                        score_out=score, divide_by=len(scales) if i == len(scales) - 1 else 0)
    return score


class MultiScaleEvaluator:
    """SegEvaluator over several scales (and the flipped image): ``update(net, image, label)`` zooms, cuts and feeds the net
    ``tile_batch`` tiles at a time per scale, keeps only the small logits, and fuses the zoom back, the mean over the scales,
    the argmax and the confusion counts into one kernel per scale; it returns the uint8 (N, H, W) prediction."""

    def __init__(self, num_classes, scales=(1.0,), ignore_label=255, tile_size=(769, 769), whole=False, flip=False,
                 tile_batch=8, device=None):
        if not 1 <= num_classes <= _mseval_lib.MAX_CLASSES:
            raise ValueError(f"MultiScaleEvaluator: num_classes {num_classes} outside [1, {_mseval_lib.MAX_CLASSES}]")
        self.scales = tuple(float(s) for s in scales)
        if not self.scales or min(self.scales) <= 0:
            raise ValueError(f"MultiScaleEvaluator: scales {scales!r} must be a non-empty sequence of positive numbers")
        self.num_classes, self.ignore_label = int(num_classes), int(ignore_label)
        self.tile_size, self.whole, self.flip = (int(tile_size[0]), int(tile_size[1])), bool(whole), bool(flip)
        self.tile_batch = int(tile_batch)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.confusion = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)

    def geometry(self, H, W):
        """[(Hs, Ws, tile origins, tile size)] per scale for an H x W image."""
        return [scale_geometry(H, W, s, self.tile_size, self.whole) for s in self.scales]

    @torch.no_grad()
    def net_logits(self, net, image):
        """Per scale, the net's fp32 (N * (T + T_flip), C, h, w) outputs over every tile of the zoomed batch."""
        _require_device(image)
        geo = self.geometry(image.shape[2], image.shape[3])
        for _, _, origins, _ in geo:
            _check_tiles(len(origins), "MultiScaleEvaluator")
        return [scale_logits(net, image, Hs, Ws, origins, tile, self.flip, self.tile_batch) for Hs, Ws, origins, tile in geo]

    @torch.no_grad()
    def accumulate(self, logits, label, H, W):
        """pred and confusion counts from net_logits' output; returns the uint8 (N, H, W) prediction."""
        _require_device(label, self.confusion, *logits)
        N, S = label.shape[0], len(self.scales)
        labels = label.to(torch.int64).contiguous()
        pred = torch.empty((N, H, W), dtype=torch.uint8, device=labels.device)
        score = torch.empty((N, self.num_classes, H, W), dtype=torch.float32, device=labels.device) if S > 1 else None
        for i, ((Hs, Ws, origins, tile), lg) in enumerate(zip(self.geometry(H, W), logits)):
            if lg.shape[1] != self.num_classes:
                raise RuntimeError(f"MultiScaleEvaluator: the net gives {lg.shape[1]} classes, {self.num_classes} expected")
            last = i == S - 1
            accumulate_call(lg, origins, self.flip, N, tile, Hs, Ws, H, W, score_in=score if i else None,
                            score_out=None if last else score, divide_by=S if last else 0, labels=labels if last else None,
                            ignore_label=self.ignore_label, pred=pred if last else None,
                            confusion=self.confusion if last else None)
        return pred

    def update(self, net, image, label):
        if label.shape != (image.shape[0],) + tuple(image.shape[2:]):
            raise RuntimeError(f"MultiScaleEvaluator: image {tuple(image.shape)} and label {tuple(label.shape)} do not match")
        return self.accumulate(self.net_logits(net, image), label, image.shape[2], image.shape[3])

    def reset(self):
        self.confusion.zero_()

    def result(self):
        return mean_iou(all_reduce_confusion(self.confusion))
