"""The ``--ohem`` training criterion on the device with the bilinear up-sample done inside its kernels (the reference's
``CriterionOhemDSN``, loss/criterion.py:37-56).

The stock form (``ohem.CriterionOhemDSN``) up-samples the main head's (B, C, h, w) logits to the label's (H, W) with
``F.interpolate(align_corners=True)`` and hands that to the OHEM kernels: one full-resolution tensor forward and one
backward.  Here the OHEM head and the plain cross-entropy head go through one autograd node on the HIP kernels behind
include/ccnet_ohemdsn.h (libccnet_ohemdsn.so): the threshold search, the keep decision and both gradients interpolate from
the low-resolution logits as they go, and what the node saves is the low-resolution logits and a workspace of at most 16
bytes per label.  Opt-in: ``ohem.CriterionOhemDSN`` is unchanged.  There is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _ohemdsn_lib


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class UpsampledOhemFunction(torch.autograd.Function):
    """loss = OHEM-CE(up(logits0), target) [+ 0.4 * CE(up(logits1), target)] for one or two fp32 (B, C, h, w) logits tensors
    and an int64 (B, H, W) target; ``up`` is bilinear with align_corners=True.  ``stats`` (a dict) receives the device
    tensors ``threshold`` (fp32), ``kept``, ``num_valid``, ``num_valid_zoomed``, ``num_out_of_range`` (int32) and
    ``head_loss`` (fp32[2]) of this call.  Saved for backward: the logits and the workspace."""

    @staticmethod
    def forward(ctx, target, ignore_label, thresh, min_kept, factor, stats, *logits):
        lib = _ohemdsn_lib.get_lib()
        heads = len(logits)
        B, C, h, w = logits[0].shape
        H, W = target.shape[1:]
        dev = logits[0].device
        nbytes = lib.ccnet_ohemdsn_workspace_bytes(B, C, h, w, H, W, heads, int(factor)) if heads in (1, 2) else 0
        if nbytes == 0:
            raise RuntimeError(f"UpsampledOhemCrossEntropy: unsupported shape: logits {tuple(logits[0].shape)} x {heads}, target "
                               f"{tuple(target.shape)}, factor {factor} (1 <= C <= {_ohemdsn_lib.MAX_CLASSES}, h <= H, w <= W, "
                               "one or two heads, factor >= 1)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        head_loss = torch.empty(2, dtype=torch.float32, device=dev)
        threshold = torch.empty(1, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        second = logits[1].data_ptr() if heads == 2 else None
        lib.check(lib.ccnet_ohemdsn_forward_f32(logits[0].data_ptr(), second, target.data_ptr(), int(ignore_label),
                                                float(thresh), int(min_kept), int(factor), loss.data_ptr(),
                                                head_loss.data_ptr(), threshold.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                nbytes, B, C, h, w, H, W, heads, _stream(dev)),
                  "ccnet_ohemdsn_forward_f32")
        stats.update(threshold=threshold[0], kept=counts[0], num_valid=counts[1], num_valid_zoomed=counts[2],
                     num_out_of_range=counts[3], head_loss=head_loss)
        ctx.save_for_backward(ws, *logits)
        ctx.geometry = (B, C, h, w, H, W, heads, int(factor))
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ws, *logits = ctx.saved_tensors
        lib = _ohemdsn_lib.get_lib()
        B, C, h, w, H, W, heads, factor = ctx.geometry
        g = grad_out.detach().to(torch.float32).contiguous()
        grads = [torch.empty_like(x) for x in logits]
        second = (lambda ts: ts[1].data_ptr() if heads == 2 else None)
        lib.check(lib.ccnet_ohemdsn_backward_f32(g.data_ptr(), logits[0].data_ptr(), second(logits), grads[0].data_ptr(),
                                                 second(grads), ws.data_ptr(), ws.numel(), B, C, h, w, H, W, heads, factor,
                                                 _stream(logits[0].device)),
                  "ccnet_ohemdsn_backward_f32")
        return (None, None, None, None, None, None, *grads)


def _upsampled_ohem(who, preds, target, ignore_label, thresh, min_kept, factor):
    """Checks and casts shared by the two modules; returns (loss, stats)."""
    assert not target.requires_grad
    shape = tuple(preds[0].shape)
    if len(shape) != 4 or target.dim() != 3 or target.shape[0] != shape[0] or any(tuple(p.shape) != shape for p in preds):
        raise RuntimeError(f"{who}: expected logits (B, C, h, w), the same for every head, and target (B, H, W); got "
                           f"{[tuple(p.shape) for p in preds]} and {tuple(target.shape)}")
    if not (target.is_cuda and all(p.is_cuda for p in preds)):
        raise RuntimeError(f"{who}: logits and target must be HIP device tensors (ccnet_amd has no CPU fallback for the OHEM + "
                           "DSN criterion kernels)")
    with torch.autocast(device_type="cuda", enabled=False):
        logits = [p.to(torch.float32).contiguous() for p in preds]      # (a differentiable cast: the gradient returns in p's dtype)
        stats = {}
        loss = UpsampledOhemFunction.apply(target.to(torch.int64).contiguous(), ignore_label, thresh, min_kept, factor, stats,
                                           *logits)
    return loss, stats


class _Stats:
    """The device tensors of the last call; reading them is the caller's synchronisation."""

    def _clear(self):
        self.last_threshold = self.last_kept = self.last_num_valid = self.last_num_out_of_range = self.last_head_loss = None

    def _take(self, stats):
        self.last_threshold, self.last_kept, self.last_num_valid = stats["threshold"], stats["kept"], stats["num_valid"]
        self.last_num_out_of_range, self.last_head_loss = stats["num_out_of_range"], stats["head_loss"]


class UpsampledOhemCrossEntropy2d(nn.Module, _Stats):
    """``ohem.OhemCrossEntropy2d(ignore_label, thresh, min_kept, factor)(F.interpolate(logits, target's (H, W),
    mode="bilinear", align_corners=True), target)`` for one head, without the full-resolution tensor.  Non-fp32 logits (e.g.
    under bf16 autocast) are cast to fp32 with autocast off; their gradient comes back in their own dtype.  After a call
    ``last_threshold`` (fp32), ``last_kept``, ``last_num_valid`` (valid full-resolution pixels), ``last_num_out_of_range``
    (int32) and ``last_head_loss`` (fp32[2]) hold that call's results as device tensors."""

    def __init__(self, ignore_label=255, thresh=0.7, min_kept=100000, factor=8):
        super().__init__()
        self.ignore_label = ignore_label
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.factor = factor
        self._clear()

    def forward(self, logits, target, weight=None):
        loss, stats = _upsampled_ohem("UpsampledOhemCrossEntropy2d", [logits], target, self.ignore_label, self.thresh,
                                      self.min_kept, self.factor)
        self._take(stats)
        return loss


class CriterionOhemDSN(nn.Module, _Stats):
    """The reference's ``CriterionOhemDSN(ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction='mean')``
    (loss/criterion.py:37-56) on the device: OHEM cross-entropy of the up-sampled main logits + 0.4 x cross-entropy of the
    up-sampled DSN logits, both heads in one autograd node and neither up-sampled tensor ever in memory.  ``use_weight`` is
    accepted and unused, as in the reference; only ``reduction='mean'`` is supported.  ``last_threshold``, ``last_kept``,
    ``last_num_valid``, ``last_num_out_of_range`` and ``last_head_loss`` (fp32[2]: the two heads' cross-entropies) are device
    tensors of the last call."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"CriterionOhemDSN: only reduction='mean' runs on the device kernels, got {reduction!r}")
        self.ignore_index = ignore_index
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.factor = 8                                      # OhemCrossEntropy2d's default; the reference passes none
        self._clear()

    def forward(self, preds, target):
        loss, stats = _upsampled_ohem("CriterionOhemDSN", list(preds[:2]), target, self.ignore_index, self.thresh,
                                      self.min_kept, self.factor)
        self._take(stats)
        return loss
