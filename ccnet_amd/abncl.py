"""Activated batch normalisation on dense ``torch.channels_last`` tensors: :class:`ABNChannelsLastFunction` over
libccnet_abncl.so (include/ccnet_abncl.h), the twin of :class:`ccnet_amd.abn.ABNFunction`.

A dense channels_last (N, C, H, W) tensor is an (N * H * W, C) row-major matrix in memory; the function hands that matrix
to the pixel-major kernels as it lies, with no layout copy, and returns channels_last tensors.  The arithmetic, both modes
(out of place / in place), the saved tensors and the process-group exchange are ``ABNFunction``'s; the layers of
:mod:`ccnet_amd.abn` dispatch here when they were converted with ``channels_last=True``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abncl_lib as L

__all__ = ["ABNChannelsLastFunction", "is_dense_channels_last"]

_DTYPES = {torch.float32: L.CCNET_ABNCL_F32, torch.bfloat16: L.CCNET_ABNCL_BF16}


def is_dense_channels_last(x) -> bool:
    """4-D and dense in (N, H, W, C) order (C = 1 and H * W = 1 tensors are this and NCHW-contiguous at once)."""
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dense(t, dtype):
    """``t`` as a dense channels_last tensor of ``dtype``: itself when it already is one, else one copy"""
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if is_dense_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


def _empty_like(t):
    """torch.empty_like keeps the strides of a dense tensor; a C = 1 or H * W = 1 tensor, dense in both orders, is pinned here"""
    return torch.empty_like(t, memory_format=torch.channels_last)


class ABNChannelsLastFunction(torch.autograd.Function):
    """y = act(gamma (x - mean) invstd + beta [+ residual]) on a dense channels_last ``x``; ``cfg`` as in
    :class:`ccnet_amd.abn.ABNFunction`: (training, momentum, eps, activation code, activation parameter, inplace, process
    group or None)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, cfg):
        from .abn import _exchange
        training, momentum, eps, act, param, inplace, group = cfg
        if not is_dense_channels_last(x):
            raise ValueError(f"ABNChannelsLastFunction: the input must be a dense channels_last 4-D tensor, got shape "
                             f"{tuple(x.shape)} with strides {tuple(x.stride())}")
        lib = L.get_lib()
        C = x.shape[1]
        M = x.numel() // max(C, 1)
        d = L.make_desc(_DTYPES[x.dtype], M, C, act, param,
                        L.CCNET_ABNCL_GAMMA_ABS_EPS if inplace else L.CCNET_ABNCL_GAMMA_WEIGHT, eps)
        dp = ctypes.byref(d)
        dev, s = x.device, _stream(x.device)
        w = None if weight is None else weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        if residual is not None:
            residual = _dense(residual, x.dtype)
        saved = None
        if training:
            nbytes = lib.ccnet_abncl_workspace_bytes(dp)
            if nbytes == 0:
                raise RuntimeError(f"ABN: unsupported shape {tuple(x.shape)}: {lib.last_error()}")
            buf = torch.empty(6 * C + nbytes // 8, dtype=torch.float64, device=dev)    # one allocation: local, saved, ws
            local, saved, ws = buf[:3 * C].view(3, C), buf[3 * C:6 * C].view(3, C), buf[6 * C:]
            lib.check(lib.ccnet_abncl_stats(dp, x.data_ptr(), local.data_ptr(), ws.data_ptr(), nbytes, s),
                      "ccnet_abncl_stats")
            table = local.unsqueeze(0) if group is None else _exchange(local, group)
            lib.check(lib.ccnet_abncl_stats_combine(dp, table.data_ptr(), table.shape[0], momentum, _p(running_mean),
                                                    _p(running_var), saved.data_ptr(), s), "ccnet_abncl_stats_combine")
        y = x if inplace else _empty_like(x)
        lib.check(lib.ccnet_abncl_forward(dp, x.data_ptr(), _p(residual), y.data_ptr(), _p(saved), _p(running_mean),
                                          _p(running_var), _p(w), _p(b), s), "ccnet_abncl_forward")
        ctx.desc, ctx.training, ctx.inplace, ctx.group = d, training, inplace, group
        ctx.has_residual, ctx.weight_dtype = residual is not None, None if weight is None else weight.dtype
        if inplace:
            ctx.mark_dirty(x)
            ctx.save_for_backward(y, residual, saved, running_mean, running_var, w, b)
        else:
            ctx.save_for_backward(x, y if act != L.CCNET_ABNCL_IDENTITY else None, saved, running_mean, running_var, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .abn import _exchange
        lib = L.get_lib()
        d = ctx.desc
        dp = ctypes.byref(d)
        if ctx.inplace:
            y, residual, saved, rm, rv, w, b = ctx.saved_tensors
            src, source = y, L.CCNET_ABNCL_FROM_OUTPUT
        else:
            src, y, saved, rm, rv, w, b = ctx.saved_tensors
            residual, source = None, L.CCNET_ABNCL_FROM_INPUT
        if not ctx.training:
            saved = None
        dy = _dense(dy, src.dtype)
        dev, s = dy.device, _stream(dy.device)
        C = d.C
        nbytes = lib.ccnet_abncl_workspace_bytes(dp)
        buf = torch.empty(2 * C + nbytes // 8, dtype=torch.float64, device=dev)         # one allocation: sums, ws
        sums, ws = buf[:2 * C].view(2, C), buf[2 * C:]
        want_w = ctx.needs_input_grad[1] and w is not None
        want_b = ctx.needs_input_grad[2] and b is not None
        dw = torch.empty(C, dtype=torch.float32, device=dev) if want_w else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if want_b else None
        lib.check(lib.ccnet_abncl_backward_reduce(dp, source, src.data_ptr(), _p(y), dy.data_ptr(), _p(residual), _p(saved),
                                                  _p(rm), _p(rv), _p(w), _p(b), sums.data_ptr(), _p(dw), _p(db),
                                                  ws.data_ptr(), nbytes, s), "ccnet_abncl_backward_reduce")
        dx = dres = None
        if ctx.needs_input_grad[0] or (ctx.has_residual and ctx.needs_input_grad[5]):
            table = sums.unsqueeze(0) if (ctx.group is None or saved is None) else _exchange(sums, ctx.group)
            dx = _empty_like(dy)
            dres = _empty_like(dy) if ctx.has_residual and ctx.needs_input_grad[5] else None
            lib.check(lib.ccnet_abncl_backward_apply(dp, source, src.data_ptr(), _p(y), dy.data_ptr(), _p(residual),
                                                     _p(saved), _p(rm), _p(rv), _p(w), _p(b), table.data_ptr(),
                                                     table.shape[0], dx.data_ptr(), _p(dres), s),
                      "ccnet_abncl_backward_apply")
        if dw is not None and ctx.weight_dtype != torch.float32:
            dw = dw.to(ctx.weight_dtype)
        if db is not None and ctx.weight_dtype != torch.float32:
            db = db.to(ctx.weight_dtype)
        return (dx if ctx.needs_input_grad[0] else None), dw, db, None, None, dres, None
