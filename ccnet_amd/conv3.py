"""The 3x3, stride-1, dilated convolution (padding = dilation, groups 1) on bf16 channels_last activations as the library's own
implicit GEMM (include/ccnet_conv3.h, ccnet_amd/csrc_conv3/): opt-in, layer for layer.

    conv3x3(x, weight, bias=None, dilation=1)     the autograd function
    DeviceConv3x3                                 an ``nn.Conv2d`` whose forward is that function (same constructor, parameters, keys)
    convert_conv3x3(module)                       swaps the class of every eligible ``nn.Conv2d`` in place, returns the count
    layout_copies                                 how many NCHW -> channels_last copies the function had to make so far
    native_batch_norm_for_bf16_channels_last(m)   what ``train_synthetic --device-conv3`` does to the stock normalisation layers

Forward: ``ccnet_conv3_pack`` (both packs of the CURRENT parameter values, every call: no cache) and ONE launch of
``ccnet_conv3_bf16`` (the bias starts the accumulators).  Backward: the same entry point on dy with the adjoint pack (dx),
``ccnet_conv3_wgrad_bf16`` + ``ccnet_conv3_wgrad_finish`` (dW: fp32 partials of row slabs, added in slab order, written in the
parameter's layout and dtype) and ``ccnet_proj_colsum_bf16`` on dy (db).  No host synchronisation, every launch on the current
stream: a step that uses it can be captured in a graph.  There is no stock fallback and no CPU route: a tensor outside the
contract raises a ``TypeError`` (dtypes) or a ``ValueError`` (shapes, devices) that names it.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _conv3_lib
from .functions import _proj_colsum, _stream

__all__ = ["conv3x3", "DeviceConv3x3", "convert_conv3x3", "eligible", "native_batch_norm_for_bf16_channels_last"]

#: NCHW (or otherwise strided) activations and gradients that had to be copied into channels_last rows, since import
layout_copies = 0

_DTYPES = {torch.bfloat16: _conv3_lib.CCNET_CONV3_BF16, torch.float32: _conv3_lib.CCNET_CONV3_F32}


def _bf16_autocast():
    return torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16


def _rows(t):
    """``t`` (B, C, H, W) bf16 as pixel-major rows: (the tensor whose memory holds them, row stride).  A tensor whose pixels are
    rows of contiguous channels at ONE stride (channels_last, or a channel slice of a wider channels_last tensor) is taken as
    it is; anything else is copied once into dense channels_last rows, and counted."""
    global layout_copies
    B, C, H, W = t.shape
    ps = t.stride(3) if W > 1 else t.stride(2) if H > 1 else t.stride(0) if B > 1 else C
    ok = (t.stride(1) == 1 and ps >= C and ps % 8 == 0 and (W == 1 or t.stride(3) == ps) and (H == 1 or t.stride(2) == W * ps)
          and (B == 1 or t.stride(0) == H * W * ps) and t.data_ptr() % 4 == 0)
    if ok:
        return t, ps
    rows = torch.empty((B, H, W, C), device=t.device, dtype=t.dtype)
    rows.permute(0, 3, 1, 2).copy_(t)
    layout_copies += 1
    return rows.permute(0, 3, 1, 2), C


def _pack(weight):
    """(fwd (Cout, 9 Cin), adj (Cin, 9 Cout)) bf16 from the parameter's current values: one launch"""
    co, ci = weight.shape[:2]
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    fwd = torch.empty((co, 9 * ci), device=w.device, dtype=torch.bfloat16)
    adj = torch.empty((ci, 9 * co), device=w.device, dtype=torch.bfloat16)
    lib = _conv3_lib.get_lib()
    with torch.cuda.device(w.device):
        lib.check(lib.ccnet_conv3_pack(w.data_ptr(), _DTYPES[w.dtype], fwd.data_ptr(), adj.data_ptr(), co, ci, _stream()), "conv3_pack")
    return fwd, adj


def _launch(a, lda, wt, bias, d):
    """``ccnet_conv3_bf16`` on the rows of ``a`` (B, K, H, W): -> (B, N, H, W) bf16, channels_last.  Batches beyond the entry
    point's 31-bit byte offsets run as several launches over whole images, which is exact: no tap crosses an image."""
    B, K, H, W = a.shape
    N = wt.shape[0]
    out = torch.empty((B, H, W, N), device=a.device, dtype=torch.bfloat16)
    plan = _conv3_lib.plan_images(B, H * W, max(lda, N))
    if not plan:
        raise ValueError(f"conv3x3: one {H} x {W} image of {max(lda, N)} channels exceeds 31-bit byte offsets")
    lib = _conv3_lib.get_lib()
    with torch.cuda.device(a.device):
        for b0, nb in plan:
            lib.check(lib.ccnet_conv3_bf16(a.data_ptr() + 2 * b0 * H * W * lda, wt.data_ptr(), None if bias is None else bias.data_ptr(),
                                           None, out.data_ptr() + 2 * b0 * H * W * N, nb, H, W, K, N, d, lda, 0, N, _stream()),
                      "conv3_bf16")
    return out.permute(0, 3, 1, 2)


def _wgrad(dy, ldd, x, ldx, d, dtype, shape):
    """dW in the parameter's layout and dtype: slab partials + the finishing launch (of every image range, where the batch
    exceeds 31-bit byte offsets: their fp32 results are then added in range order)"""
    B, N, H, W = dy.shape
    C = x.shape[1]
    plan = _conv3_lib.plan_images(B, H * W, max(ldd, ldx))
    if not plan:
        raise ValueError(f"conv3x3: one {H} x {W} image of {max(ldd, ldx)} channels exceeds 31-bit byte offsets")
    lib = _conv3_lib.get_lib()
    single = len(plan) == 1
    outs = []
    with torch.cuda.device(dy.device):
        for b0, nb in plan:
            S = lib.ccnet_conv3_wgrad_slabs(nb, H, W, N, C)
            nbytes = lib.ccnet_conv3_wgrad_workspace_bytes(nb, H, W, N, C, S)
            part = torch.empty(nbytes // 4, device=dy.device, dtype=torch.float32)
            dw = torch.empty(shape, device=dy.device, dtype=dtype if single else torch.float32)
            lib.check(lib.ccnet_conv3_wgrad_bf16(dy.data_ptr() + 2 * b0 * H * W * ldd, x.data_ptr() + 2 * b0 * H * W * ldx, part.data_ptr(),
                                                 nbytes, nb, H, W, N, C, d, ldd, ldx, S, _stream()), "conv3_wgrad_bf16")
            lib.check(lib.ccnet_conv3_wgrad_finish(part.data_ptr(), dw.data_ptr(), _DTYPES[dw.dtype], N, C, S, _stream()),
                      "conv3_wgrad_finish")
            outs.append(dw)
    if single:
        return outs[0]
    total = outs[0]
    for t in outs[1:]:
        total = total + t
    return total.to(dtype)


class Conv3x3Function(torch.autograd.Function):
    """y = conv2d(x, weight, bias, stride 1, padding = dilation, dilation) on bf16 rows; see the module docstring."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        co, ci = weight.shape[:2]
        d = int(dilation)
        x, ldx = _rows(x)
        fwd, adj = _pack(weight)
        b32 = None
        if bias is not None:
            b32 = bias.detach().float().contiguous()
        y = _launch(x, ldx, fwd, b32, d)
        if any(ctx.needs_input_grad):
            # (the adjoint pack -- the values this forward saw -- goes through save_for_backward like x: hooks and offload apply)
            ctx.save_for_backward(x, adj)
            ctx.d, ctx.ldx, ctx.wmeta = d, ldx, (weight.dtype, tuple(weight.shape))
            ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, adj = ctx.saved_tensors
        if dy.dtype != torch.bfloat16:
            raise TypeError(f"conv3x3: the output gradient is {dy.dtype}, the kernels take torch.bfloat16")
        dy, ldd = _rows(dy)
        B, N, H, W = dy.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _launch(dy, ldd, adj, None, ctx.d)                            # the same launch on dy with the adjoint pack
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dy, ldd, x, ctx.ldx, ctx.d, *ctx.wmeta)
        if ctx.bias_dtype is not None and ctx.needs_input_grad[2]:
            db = _proj_colsum(dy.as_strided((B * H * W, N), (ldd, 1))).to(ctx.bias_dtype)
        return dx, dw, db, None


def conv3x3(x, weight, bias=None, dilation=1):
    """``F.conv2d(x, weight, bias, stride=1, padding=dilation, dilation=dilation)`` for a 3x3 kernel on the library's own kernels.

    x (B, Cin, H, W) bf16 on a HIP device, channels_last-strided (an NCHW-contiguous x is converted with one copy, counted in
    ``layout_copies``); weight (Cout, Cin, 3, 3) bf16, or fp32 under a bf16 autocast (rounded to nearest even, as autocast's own
    cast does); bias (Cout) of the weight's dtype, or None; Cin % 8 == 0, Cout % 8 == 0; dilation >= 1.  Under a bf16 autocast an
    fp32 x is cast to bf16 first.  Returns y (B, Cout, H, W) bf16, channels_last; gradients come back in each parameter's dtype."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("conv3x3: x and weight are tensors")
    if x.dtype == torch.float32 and _bf16_autocast():
        x = x.to(torch.bfloat16)
    if x.dtype != torch.bfloat16:
        raise TypeError(f"conv3x3: x is {x.dtype}, the kernels take torch.bfloat16 activations (fp32 only under a bf16 autocast)")
    if weight.dtype not in _DTYPES or (weight.dtype == torch.float32 and not _bf16_autocast()):
        raise TypeError(f"conv3x3: weight is {weight.dtype}; it is torch.bfloat16, or torch.float32 under a bf16 autocast")
    if bias is not None and bias.dtype != weight.dtype:
        raise TypeError(f"conv3x3: bias is {bias.dtype}, weight {weight.dtype}")
    if x.dim() != 4:
        raise ValueError(f"conv3x3: x has {x.dim()} dimensions, (B, Cin, H, W) is needed")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"conv3x3: weight has shape {tuple(weight.shape)}, (Cout, Cin, 3, 3) is needed")
    co, ci = weight.shape[:2]
    if x.shape[1] != ci:
        raise ValueError(f"conv3x3: x has {x.shape[1]} channels, weight takes {ci}")
    if ci % 8 or co % 8:
        raise ValueError(f"conv3x3: Cin = {ci} and Cout = {co} must be multiples of 8")
    if bias is not None and tuple(bias.shape) != (co,):
        raise ValueError(f"conv3x3: bias has shape {tuple(bias.shape)}, ({co},) is needed")
    if int(dilation) != dilation or dilation < 1:
        raise ValueError(f"conv3x3: dilation = {dilation} must be an integer >= 1")
    if min(x.shape) < 1:
        raise ValueError(f"conv3x3: x has an empty dimension: {tuple(x.shape)}")
    if not x.is_cuda or weight.device != x.device or (bias is not None and bias.device != x.device):
        raise ValueError("conv3x3: x, weight and bias live on one HIP device (there is no CPU route)")
    return Conv3x3Function.apply(x, weight, bias, int(dilation))


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def eligible(m):
    """what ``convert_conv3x3`` swaps: 3x3, stride 1, padding == dilation (the same in both directions), groups 1, zeros padding,
    Cin % 8 == 0 and Cout % 8 == 0"""
    if not isinstance(m, nn.Conv2d) or isinstance(m.padding, str):
        return False
    d = _pair(m.dilation)
    return (_pair(m.kernel_size) == (3, 3) and _pair(m.stride) == (1, 1) and d[0] == d[1] and _pair(m.padding) == d and m.groups == 1
            and m.padding_mode == "zeros" and m.in_channels % 8 == 0 and m.out_channels % 8 == 0)


class DeviceConv3x3(nn.Conv2d):
    """``nn.Conv2d`` (same constructor, parameter names and ``state_dict`` keys) whose forward is :func:`conv3x3`; a
    configuration outside :func:`eligible` raises at the first forward."""

    def forward(self, x):
        if not eligible(self):
            raise ValueError(f"DeviceConv3x3 takes 3x3, stride 1, padding == dilation, groups 1, zeros padding and channel counts "
                             f"divisible by 8; got {self.extra_repr()}")
        return conv3x3(x, self.weight, self.bias, _pair(self.dilation)[0])


def convert_conv3x3(module):
    """Swap the class of every eligible plain ``nn.Conv2d`` of ``module`` (itself included) for :class:`DeviceConv3x3`, in place
    (parameters, buffers and hooks stay where they are); returns how many were swapped."""
    n = 0
    for m in module.modules():
        if type(m) is nn.Conv2d and eligible(m):
            m.__class__ = DeviceConv3x3
            n += 1
    return n


# ----------------------------------------------------------------------------------------------
# the stock normalisation layers behind channels_last convolutions (train_synthetic --device-conv3 only)
# ----------------------------------------------------------------------------------------------
def bf16_channels_last_fp32_affine(x, weight):
    """the one input of the stock ``inplace_abn`` layers that ``--device-conv3`` creates and the parent never did: a 4-D bfloat16
    activation in channels_last (and not also NCHW-contiguous) with float32 affine parameters"""
    return (x.dim() == 4 and x.dtype == torch.bfloat16 and weight is not None and weight.dtype == torch.float32
            and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous())


_NATIVE_CLASSES = {}


def _native_class(base):
    if base not in _NATIVE_CLASSES:
        import torch.distributed as dist

        import inplace_abn

        class NativeChannelsLast(base):
            """``base`` whose batch norm of a bf16 channels_last CUDA activation with float32 affine parameters runs with the
            vendor library switched off (``torch.backends.cudnn.flags(enabled=False)`` around that one call), i.e. on torch's
            own kernels.  With the vendor library on, that call -- training, the first layer of the model on an MI355X --
            ended the process with a segmentation fault on the host side of batch_norm; why was not established.  Passing
            ``cudnn_enabled=False`` to ``torch.batch_norm`` is not enough: the process died in the same place, so the
            backend is chosen from the process-wide flag, which is why the flag itself is set and restored here.  Every
            other input takes ``base``'s call unchanged."""

            def _normalise(self, x):
                syncs = (isinstance(self, inplace_abn.InPlaceABNSync) and self.training and dist.is_available()
                         and dist.is_initialized() and dist.get_world_size() > 1)
                if x.is_cuda and not syncs and bf16_channels_last_fp32_affine(x, self.weight):
                    with torch.backends.cudnn.flags(enabled=False):
                        return super()._normalise(x)
                return super()._normalise(x)

        NativeChannelsLast.__name__ = NativeChannelsLast.__qualname__ = base.__name__ + "NativeChannelsLast"
        _NATIVE_CLASSES[base] = NativeChannelsLast
    return _NATIVE_CLASSES[base]


def native_batch_norm_for_bf16_channels_last(module):
    """Swap the class of every stock ``inplace_abn`` layer of ``module`` (ABN, InPlaceABN, InPlaceABNSync; not the device ABN
    layers) for its ``NativeChannelsLast`` twin, in place; parameters, buffers and ``state_dict`` keys stay.  Returns the count."""
    import inplace_abn
    n = 0
    for m in module.modules():
        if type(m) in (inplace_abn.ABN, inplace_abn.InPlaceABN, inplace_abn.InPlaceABNSync):
            m.__class__ = _native_class(type(m))
            n += 1
    return n
