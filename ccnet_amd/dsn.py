"""The deep-supervision cross-entropy on the device (the reference's default criterion, loss/criterion.py:11-35), with the
bilinear up-sample done inside the kernels.

The stock form (``segmodel.CriterionDSN``) up-samples each head's (B, C, h, w) logits to the label's (H, W) with
``F.interpolate(align_corners=True)`` and hands that to ``F.cross_entropy``: per head one full-resolution tensor forward and
one backward.  Here both heads go through one autograd node on the HIP kernels behind include/ccnet_dsn.h
(libccnet_dsn.so): they interpolate from the low-resolution logits as they go, and what the node saves is the
low-resolution logits and a workspace of at most 16 bytes per label.  Opt-in: ``segmodel.CriterionDSN`` is unchanged.
There is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _dsn_lib


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class UpsampledCrossEntropyFunction(torch.autograd.Function):
    """loss = weight0 * CE(up(logits0), target) [+ weight1 * CE(up(logits1), target)] for one or two fp32 (B, C, h, w)
    logits tensors and an int64 (B, H, W) target; ``up`` is bilinear with align_corners=True and CE the mean over the labels
    in [0, C) other than ``ignore_index``.  ``stats`` (a dict) receives the device tensors ``num_valid``,
    ``num_out_of_range`` (int32) and ``head_loss`` (fp32[2]) of this call.  Saved for backward: the logits and the workspace."""

    @staticmethod
    def forward(ctx, target, weight0, weight1, ignore_index, stats, *logits):
        lib = _dsn_lib.get_lib()
        heads = len(logits)
        B, C, h, w = logits[0].shape
        H, W = target.shape[1:]
        dev = logits[0].device
        nbytes = lib.ccnet_dsn_workspace_bytes(B, C, h, w, H, W, heads) if heads in (1, 2) else 0
        if nbytes == 0:
            raise RuntimeError(f"UpsampledCrossEntropy: unsupported shape: logits {tuple(logits[0].shape)} x {heads}, target "
                               f"{tuple(target.shape)} (1 <= C <= {_dsn_lib.MAX_CLASSES}, h <= H, w <= W, one or two heads)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        head_loss = torch.empty(2, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        second = logits[1].data_ptr() if heads == 2 else None
        lib.check(lib.ccnet_dsn_forward_f32(logits[0].data_ptr(), second, target.data_ptr(), float(weight0), float(weight1),
                                            loss.data_ptr(), head_loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                            B, C, h, w, H, W, heads, int(ignore_index), _stream(dev)),
                  "ccnet_dsn_forward_f32")
        stats.update(num_valid=counts[0], num_out_of_range=counts[1], head_loss=head_loss)
        ctx.save_for_backward(ws, *logits)
        ctx.geometry = (B, C, h, w, H, W, heads, float(weight0), float(weight1))
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ws, *logits = ctx.saved_tensors
        lib = _dsn_lib.get_lib()
        B, C, h, w, H, W, heads, weight0, weight1 = ctx.geometry
        g = grad_out.detach().to(torch.float32).contiguous()
        grads = [torch.empty_like(x) for x in logits]
        second = (lambda ts: ts[1].data_ptr() if heads == 2 else None)
        lib.check(lib.ccnet_dsn_backward_f32(g.data_ptr(), logits[0].data_ptr(), second(logits), grads[0].data_ptr(),
                                             second(grads), weight0, weight1, ws.data_ptr(), ws.numel(), B, C, h, w, H, W,
                                             heads, _stream(logits[0].device)),
                  "ccnet_dsn_backward_f32")
        return (None, None, None, None, None, *grads)


def _upsampled_cross_entropy(who, preds, target, weights, ignore_index):
    """Checks and casts shared by the two modules; returns (loss, stats)."""
    assert not target.requires_grad
    if not (target.is_cuda and all(p.is_cuda for p in preds)):
        raise RuntimeError(f"{who}: logits and target must be HIP device tensors (ccnet_amd has no CPU fallback for the DSN "
                           "cross-entropy kernels)")
    shape = tuple(preds[0].shape)
    if len(shape) != 4 or target.dim() != 3 or target.shape[0] != shape[0] or any(tuple(p.shape) != shape for p in preds):
        raise RuntimeError(f"{who}: expected logits (B, C, h, w), the same for every head, and target (B, H, W); got "
                           f"{[tuple(p.shape) for p in preds]} and {tuple(target.shape)}")
    with torch.autocast(device_type="cuda", enabled=False):
        logits = [p.to(torch.float32).contiguous() for p in preds]      # (a differentiable cast: the gradient returns in p's dtype)
        stats = {}
        loss = UpsampledCrossEntropyFunction.apply(target.to(torch.int64).contiguous(), weights[0], weights[1], ignore_index,
                                                   stats, *logits)
    return loss, stats


class UpsampledCrossEntropy2d(nn.Module):
    """``F.cross_entropy(F.interpolate(logits, target's (H, W), mode="bilinear", align_corners=True), target,
    ignore_index=ignore_index)`` for one head, without the full-resolution tensor.  Non-fp32 logits (e.g. under bf16 autocast)
    are cast to fp32 with autocast off; their gradient comes back in their own dtype.  After a call ``last_num_valid`` and
    ``last_num_out_of_range`` (labels outside [0, C) other than ``ignore_index``: ignored, where the stock op asserts) hold
    that call's counts as device tensors; reading them is the caller's synchronisation."""

    def __init__(self, ignore_index=255):
        super().__init__()
        self.ignore_index = ignore_index
        self.last_num_valid = self.last_num_out_of_range = None

    def forward(self, logits, target):
        loss, stats = _upsampled_cross_entropy("UpsampledCrossEntropy2d", [logits], target, (1.0, 0.0), self.ignore_index)
        self.last_num_valid, self.last_num_out_of_range = stats["num_valid"], stats["num_out_of_range"]
        return loss


class CriterionDSN(nn.Module):
    """The reference's ``CriterionDSN(ignore_index=255, use_weight=True, reduction='mean')`` (loss/criterion.py:11-35) on the
    device: cross-entropy of the up-sampled main logits + 0.4 x cross-entropy of the up-sampled DSN logits, both heads in
    one autograd node; one head when ``len(preds) < 2``.  ``use_weight`` is accepted and unused, as in the reference; only
    ``reduction='mean'`` is supported.  ``last_num_valid``, ``last_num_out_of_range`` and ``last_head_loss`` (fp32[2]: the two
    heads' cross-entropies) are device tensors of the last call."""

    AUX_WEIGHT = 0.4

    def __init__(self, ignore_index=255, use_weight=True, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"CriterionDSN: only reduction='mean' runs on the device kernels, got {reduction!r}")
        self.ignore_index = ignore_index
        self.last_num_valid = self.last_num_out_of_range = self.last_head_loss = None

    def forward(self, preds, target):
        heads = list(preds[:2]) if len(preds) >= 2 else [preds[0]]
        weights = (1.0, self.AUX_WEIGHT) if len(heads) == 2 else (1.0, 0.0)
        loss, stats = _upsampled_cross_entropy("CriterionDSN", heads, target, weights, self.ignore_index)
        self.last_num_valid, self.last_num_out_of_range = stats["num_valid"], stats["num_out_of_range"]
        self.last_head_loss = stats["head_loss"]
        return loss
