"""The ``--lovasz`` training criterion on the device with the bilinear up-sample and the softmax done inside its kernels (the
reference's ``CriterionOhemDSN2``, loss/criterion.py:59-78).

The stock form (``lovasz.CriterionOhemDSN2``) up-samples the main head's (B, C, h, w) logits to the label's (H, W) with
``F.interpolate(align_corners=True)``, takes ``F.softmax`` and ``nn.CrossEntropyLoss`` of that as stock ops and hands the
probabilities to the Lovász kernels: three full-resolution class maps forward and as many gradients backward.  Here the whole
criterion is one autograd node on the HIP kernels behind include/ccnet_celovasz.h (libccnet_celovasz.so): the errors that the
Lovász sort takes, the cross-entropy and the gradient interpolate from the low-resolution logits as they go, and what the node
saves is the low-resolution logits and a workspace: the Lovász sort workspace plus at most 12 bytes per label.  Opt-in:
``lovasz.CriterionOhemDSN2`` is unchanged.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _celovasz_lib
from ._lovasz_lib import class_selection


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class UpsampledCELovaszFunction(torch.autograd.Function):
    """loss = CE(up(logits), target) + lovasz_softmax(softmax(up(logits)), target) for fp32 (B, C, h, w) logits and an int64
    (B, H, W) target; ``up`` is bilinear with align_corners=True.  ``stats`` (a dict) receives the device tensors
    ``head_loss`` (fp32[2]: CE, Lovász), ``num_valid``, ``num_out_of_range`` and ``n_kept`` (int32) of this call.  Saved for
    backward: the workspace and the logits."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, classes, per_image, stats):
        lib = _celovasz_lib.get_lib()
        B, C, h, w = logits.shape
        H, W = target.shape[1:]
        dev = logits.device
        nbytes = lib.ccnet_celovasz_workspace_bytes(B, C, h, w, H, W, int(per_image))
        if nbytes == 0:
            raise RuntimeError(f"UpsampledCELovasz: unsupported shape: logits {tuple(logits.shape)}, target {tuple(target.shape)}, "
                               f"per_image={per_image} ({_celovasz_lib.MIN_CLASSES} <= C <= {_celovasz_lib.MAX_CLASSES}, h <= H, "
                               "w <= W, at most 2^24 pixels per segment)")
        present_only, weights = class_selection(classes, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        head_loss = torch.empty(2, dtype=torch.float32, device=dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        lib.check(lib.ccnet_celovasz_forward_f32(logits.data_ptr(), target.data_ptr(), int(ignore_index), int(per_image),
                                                 int(present_only), None if weights is None else ctypes.addressof(weights),
                                                 loss.data_ptr(), head_loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                                 B, C, h, w, H, W, _stream(dev)),
                  "ccnet_celovasz_forward_f32")
        stats.update(head_loss=head_loss, num_valid=counts[0], num_out_of_range=counts[1], n_kept=counts[2])
        ctx.save_for_backward(ws, logits)
        ctx.geometry = (B, C, h, w, H, W, int(per_image))
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ws, logits = ctx.saved_tensors
        lib = _celovasz_lib.get_lib()
        B, C, h, w, H, W, per_image = ctx.geometry
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(logits)
        lib.check(lib.ccnet_celovasz_backward_f32(g.data_ptr(), logits.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  B, C, h, w, H, W, per_image, _stream(logits.device)),
                  "ccnet_celovasz_backward_f32")
        return grad, None, None, None, None, None


class UpsampledCELovasz(nn.Module):
    """``F.cross_entropy(up, target, ignore_index=ignore_index) + lovasz_softmax(F.softmax(up, 1), target, classes, per_image,
    ignore=ignore_index)`` with ``up = F.interpolate(logits, target's (H, W), mode="bilinear", align_corners=True)``, without
    any full-resolution class map beside the Lovász sort workspace.  ``classes`` is 'present', 'all' or a list of ids (a
    duplicate counts twice).  Non-fp32 logits (e.g. under bf16 autocast) are cast to fp32 with autocast off; their gradient
    comes back in their own dtype.  After a call ``last_head_loss`` (fp32[2]: the cross-entropy and the Lovász term),
    ``last_num_valid``, ``last_num_out_of_range`` and ``last_n_kept`` (int32) hold that call's results as device tensors;
    reading them is the caller's synchronisation.  A label outside [0, C) other than ``ignore_index`` is ignored by both
    terms and counted (include/ccnet_celovasz.h)."""

    def __init__(self, ignore_index=255, classes="present", per_image=False):
        super().__init__()
        self.ignore_index, self.classes, self.per_image = ignore_index, classes, bool(per_image)
        self.last_head_loss = self.last_num_valid = self.last_num_out_of_range = self.last_n_kept = None

    def forward(self, logits, target):
        assert not target.requires_grad
        if logits.dim() != 4 or target.dim() != 3 or target.shape[0] != logits.shape[0]:
            raise RuntimeError(f"UpsampledCELovasz: expected logits (B, C, h, w) and target (B, H, W); got {tuple(logits.shape)} "
                               f"and {tuple(target.shape)}")
        if not (logits.is_cuda and target.is_cuda):
            raise RuntimeError("UpsampledCELovasz: logits and target must be HIP device tensors (ccnet_amd has no CPU fallback "
                               "for the CE + Lovász criterion kernels)")
        classes = self.classes if isinstance(self.classes, str) else [int(c) for c in self.classes]
        with torch.autocast(device_type="cuda", enabled=False):
            x = logits.to(torch.float32).contiguous()          # (a differentiable cast: the gradient returns in logits' dtype)
            stats = {}
            loss = UpsampledCELovaszFunction.apply(x, target.to(torch.int64).contiguous(), self.ignore_index, classes,
                                                   self.per_image, stats)
        self.last_head_loss, self.last_num_valid = stats["head_loss"], stats["num_valid"]
        self.last_num_out_of_range, self.last_n_kept = stats["num_out_of_range"], stats["n_kept"]
        return loss


class CriterionOhemDSN2(nn.Module):
    """The reference's ``CriterionOhemDSN2(ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction='mean')``
    (loss/criterion.py:59-78) on the device: cross-entropy + Lovász-softmax of the up-sampled main logits in one autograd node,
    the up-sampled tensor and its softmax never in memory.  Despite its name it does no OHEM and leaves the DSN logits
    (``preds[1]``) unused, as in the reference: they get no gradient.  ``thresh``, ``min_kept`` and ``use_weight`` are accepted
    and ignored; only ``reduction='mean'`` is supported.  ``criterion`` is the :class:`UpsampledCELovasz` that holds the last
    call's device tensors."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"CriterionOhemDSN2: only reduction='mean' runs on the device kernels, got {reduction!r}")
        self.ignore_index = ignore_index
        self.criterion = UpsampledCELovasz(ignore_index=ignore_index)

    def forward(self, preds, target):
        return self.criterion(preds[0], target)
