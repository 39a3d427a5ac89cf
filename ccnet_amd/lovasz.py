"""Lovász-softmax loss on the device (the reference's loss/lovasz_losses.py:18-31,153-218) and the CE + Lovász training
criterion ``CriterionOhemDSN2`` (loss/criterion.py:59-78).

The reference runs one host-synchronising ``fg.sum()``, a full ``torch.sort``, a gather, a cumsum and a dot per class.
Here the per-class errors, one segmented radix sort over every class at once, the scan that turns the sorted fg flags into
the Lovász gradient, and the means are HIP kernels behind include/ccnet_lovasz.h (libccnet_lovasz.so): the step stays on
the device and never waits for it.  Equal errors sort stably (ascending flattened pixel order).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lovasz_lib


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class LovaszSoftmaxFunction(torch.autograd.Function):
    """loss = Lovász-softmax of fp32 (B, C, H, W) probabilities against int64 (B, H, W) labels.  ``stats`` (a dict)
    receives the device tensor ``n_kept`` (int32: kept classes, multiplicities included, summed over images)."""

    @staticmethod
    def forward(ctx, probas, labels, classes, per_image, ignore, stats):
        lib = _lovasz_lib.get_lib()
        B, C, H, W = probas.shape
        dev = probas.device
        nbytes = lib.ccnet_lovasz_workspace_bytes(B, C, H, W, int(per_image))
        if nbytes == 0:
            raise RuntimeError(f"lovasz_softmax: unsupported shape {tuple(probas.shape)} (per_image={per_image}): "
                               "2 <= C <= 256 and at most 2^24 pixels per segment")
        present_only, weights = _lovasz_lib.class_selection(classes, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        n_kept = torch.empty(1, dtype=torch.int32, device=dev)
        lib.check(lib.ccnet_lovasz_forward_f32(probas.data_ptr(), labels.data_ptr(), loss.data_ptr(), n_kept.data_ptr(),
                                               ws.data_ptr(), nbytes, B, C, H, W, 0 if ignore is None else int(ignore),
                                               int(ignore is None), int(per_image), int(present_only),
                                               None if weights is None else ctypes.addressof(weights), _stream(dev)),
                  "ccnet_lovasz_forward_f32")
        stats["n_kept"] = n_kept[0]
        ctx.save_for_backward(ws)
        ctx.shape, ctx.per_image = (B, C, H, W), per_image
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (ws,) = ctx.saved_tensors
        lib = _lovasz_lib.get_lib()
        B, C, H, W = ctx.shape
        g = grad_out.detach().to(torch.float32).contiguous()
        grad = torch.empty((B, C, H, W), dtype=torch.float32, device=ws.device)
        lib.check(lib.ccnet_lovasz_backward_f32(g.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(), B, C, H, W,
                                                int(ctx.per_image), _stream(ws.device)),
                  "ccnet_lovasz_backward_f32")
        return grad, None, None, None, None, None


def _check_inputs(probas, labels):
    if probas.dim() == 3:
        raise ValueError("lovasz_softmax: 3-D (B, H, W) input is the reference's sigmoid (binary) form, which ccnet_amd does "
                         "not implement; pass (B, C, H, W) class probabilities with C >= 2")
    if probas.dim() != 4 or tuple(labels.shape) != (probas.shape[0],) + tuple(probas.shape[2:]):
        raise ValueError(f"lovasz_softmax: expected probas (B, C, H, W) and labels (B, H, W); got {tuple(probas.shape)} and "
                         f"{tuple(labels.shape)}")
    if probas.shape[1] == 1:
        raise ValueError("lovasz_softmax: C = 1 is the reference's sigmoid (binary) form, which ccnet_amd does not implement")
    if not (probas.is_cuda and labels.is_cuda):
        raise RuntimeError("lovasz_softmax: probas and labels must be HIP device tensors (ccnet_amd has no CPU fallback for "
                           "the Lovász-softmax kernels)")


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None, stats=None):
    """The reference's ``lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=None)`` on the device.

    probas (B, C, H, W) class probabilities, labels (B, H, W) integer ids; ``classes`` is 'present', 'all' or a list of
    ids (a duplicate counts twice); ``ignore`` a void label or None.  Returns an fp32 scalar.  Non-fp32 probabilities are
    cast with autocast off; their gradient comes back in their own dtype.  Divergences from the reference (see
    include/ccnet_lovasz.h): equal errors sort stably; no valid pixel gives 0 with zero gradient; one valid pixel works.
    ``stats`` (a dict, optional) receives ``n_kept`` as a device tensor."""
    _check_inputs(probas, labels)
    with torch.autocast(device_type="cuda", enabled=False):
        p = probas.to(torch.float32).contiguous()
    if not isinstance(classes, str):
        classes = [int(c) for c in classes]
    return LovaszSoftmaxFunction.apply(p, labels.to(torch.int64).contiguous(), classes, bool(per_image), ignore,
                                       {} if stats is None else stats)


class LovaszSoftmax(nn.Module):
    """``lovasz_softmax`` as a module: ``LovaszSoftmax(classes='present', per_image=False, ignore=None)(probas, labels)``.
    After a call, ``last_n_kept`` holds that call's kept class count as a device tensor."""

    def __init__(self, classes="present", per_image=False, ignore=None):
        super().__init__()
        self.classes, self.per_image, self.ignore = classes, per_image, ignore
        self.last_n_kept = None

    def forward(self, probas, labels):
        stats = {}
        loss = lovasz_softmax(probas, labels, self.classes, self.per_image, self.ignore, stats)
        self.last_n_kept = stats["n_kept"]
        return loss


class CriterionOhemDSN2(nn.Module):
    """Cross-entropy + Lovász-softmax of the up-sampled main logits (loss/criterion.py:59-78).  Despite its name it does no
    OHEM and leaves the DSN logits unused, as in the reference (``thresh``, ``min_kept`` and ``use_weight`` are accepted
    and ignored).  The up-sampling, the softmax and the cross-entropy stay stock ops."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduction="mean"):
        super().__init__()
        self.ignore_index = ignore_index
        self.criterion = nn.CrossEntropyLoss(ignore_index=ignore_index, reduction=reduction)
        self.lovasz = LovaszSoftmax(ignore=ignore_index)

    def forward(self, preds, target):
        h, w = target.size(1), target.size(2)
        scale_pred = F.interpolate(preds[0], size=(h, w), mode="bilinear", align_corners=True)
        _check_inputs(scale_pred, target)
        loss1 = self.criterion(scale_pred, target)
        loss2 = self.lovasz(F.softmax(scale_pred, dim=1), target)
        return loss1 + loss2
