"""OHEM cross-entropy on the device (the reference's loss/loss.py:9-93) and the ``--ohem`` training criterion
(loss/criterion.py:37-56).

The reference moves the full-resolution softmax to the host every step (scipy zoom, ``np.partition``, a new int64 target
back to the device).  Here the threshold search, the masked cross-entropy and its gradient are HIP kernels behind
include/ccnet_ohem.h (libccnet_ohem.so): the step stays on the device and never waits for it.  There is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ohem_lib


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class OhemCrossEntropyFunction(torch.autograd.Function):
    """loss = OHEM cross-entropy of fp32 (B, C, H, W) logits against int64 (B, H, W) labels.  ``stats`` (a dict) receives
    the device tensors ``threshold`` (fp32), ``kept`` and ``num_valid`` (int32) of this call."""

    @staticmethod
    def forward(ctx, logits, target, ignore_label, thresh, min_kept, factor, stats):
        lib = _ohem_lib.get_lib()
        B, C, H, W = logits.shape
        dev = logits.device
        nbytes = lib.ccnet_ohem_workspace_bytes(B, C, H, W, factor)
        if nbytes == 0:
            raise RuntimeError(f"OhemCrossEntropy2d: unsupported shape {tuple(logits.shape)} / factor {factor}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        threshold = torch.empty(1, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        lib.check(lib.ccnet_ohem_forward_f32(logits.data_ptr(), target.data_ptr(), loss.data_ptr(), threshold.data_ptr(),
                                             counts.data_ptr(), counts.data_ptr() + 4, ws.data_ptr(), nbytes, B, C, H, W,
                                             int(ignore_label), float(thresh), int(min_kept), int(factor), _stream(dev)),
                  "ccnet_ohem_forward_f32")
        stats.update(threshold=threshold[0], kept=counts[0], num_valid=counts[1])
        ctx.save_for_backward(logits, ws)
        ctx.factor = factor
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, ws = ctx.saved_tensors
        lib = _ohem_lib.get_lib()
        B, C, H, W = logits.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(logits)
        lib.check(lib.ccnet_ohem_backward_f32(g.data_ptr(), logits.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(),
                                              B, C, H, W, ctx.factor, _stream(logits.device)),
                  "ccnet_ohem_backward_f32")
        return grad, None, None, None, None, None, None


class OhemCrossEntropy2d(nn.Module):
    """The reference's ``OhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=100000, factor=8)`` on the device.

    ``forward(predict, target, weight=None)``: ``weight`` is accepted and ignored, as in the reference.  Non-fp32 logits
    (e.g. under bf16 autocast) are cast to fp32 with autocast off; their gradient comes back in their own dtype.  After a
    call, ``last_threshold``, ``last_kept`` and ``last_num_valid`` hold that call's statistics as device tensors (the
    reference prints them; reading them is the caller's synchronisation)."""

    def __init__(self, ignore_label=255, thresh=0.7, min_kept=100000, factor=8):
        super().__init__()
        self.ignore_label = ignore_label
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.factor = factor
        self.last_threshold = self.last_kept = self.last_num_valid = None

    def forward(self, predict, target, weight=None):
        assert not target.requires_grad
        if not (predict.is_cuda and target.is_cuda):
            raise RuntimeError("OhemCrossEntropy2d: predict and target must be HIP device tensors (ccnet_amd has no CPU "
                               "fallback for the OHEM kernels)")
        if predict.dim() != 4 or target.shape != (predict.shape[0],) + tuple(predict.shape[2:]):
            raise RuntimeError(f"OhemCrossEntropy2d: expected predict (B, C, H, W) and target (B, H, W); got "
                               f"{tuple(predict.shape)} and {tuple(target.shape)}")
        with torch.autocast(device_type="cuda", enabled=False):
            logits = predict.to(torch.float32).contiguous()
        stats = {}
        loss = OhemCrossEntropyFunction.apply(logits, target.to(torch.int64).contiguous(), self.ignore_label, self.thresh,
                                              self.min_kept, self.factor, stats)
        self.last_threshold, self.last_kept, self.last_num_valid = stats["threshold"], stats["kept"], stats["num_valid"]
        return loss


class CriterionOhemDSN(nn.Module):
    """OHEM cross-entropy on the up-sampled main logits + 0.4 x cross-entropy on the up-sampled DSN logits
    (loss/criterion.py:37-56).  The bilinear up-sampling stays a stock op, as in the reference; with ``fused_aux=True`` the
    second, plain cross-entropy head runs on :class:`ccnet_amd.dsn.UpsampledCrossEntropy2d` instead, which up-samples
    inside its kernels (the OHEM head keeps the stock op here).  :class:`ccnet_amd.ohemdsn.CriterionOhemDSN` is the fully fused
    form: both heads, the threshold search included, on kernels that up-sample as they read."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction="mean", fused_aux=False):
        super().__init__()
        self.ignore_index = ignore_index
        self.fused_aux = bool(fused_aux)
        self.criterion1 = OhemCrossEntropy2d(ignore_index, thresh, min_kept)
        if self.fused_aux:
            if reduction != "mean":
                raise ValueError(f"CriterionOhemDSN(fused_aux=True): only reduction='mean' runs on the device kernels, got {reduction!r}")
            from .dsn import UpsampledCrossEntropy2d
            self.criterion2 = UpsampledCrossEntropy2d(ignore_index)
        else:
            self.criterion2 = nn.CrossEntropyLoss(ignore_index=ignore_index, reduction=reduction)

    def forward(self, preds, target):
        h, w = target.size(1), target.size(2)
        loss1 = self.criterion1(F.interpolate(preds[0], size=(h, w), mode="bilinear", align_corners=True), target)
        if self.fused_aux:
            loss2 = self.criterion2(preds[1], target)
        else:
            loss2 = self.criterion2(F.interpolate(preds[1], size=(h, w), mode="bilinear", align_corners=True), target)
        return loss1 + loss2 * 0.4
