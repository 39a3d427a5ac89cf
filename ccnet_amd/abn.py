"""Activated batch normalisation on the device: ``ABN``, ``InPlaceABN`` and ``InPlaceABNSync`` over libccnet_abn.so
(include/ccnet_abn.h), and :func:`convert_abn`, which swaps them into a built model.

The classes subclass the ``inplace_abn`` restatement (same constructor, same parameter and buffer names, so ``state_dict``
keys do not change) and run each layer as HIP kernels: a statistics pass, one fused normalise + activation (+ residual)
pass, and in backward one reduction and one apply pass.  Two arithmetics, one per mode (``module.inplace``):

- out of place (``ABN``'s default): gamma = ``weight`` as is, what ``inplace_abn.ABN`` computes; backward reads the saved
  input (and the output for the activation's derivative);
- in place (``InPlaceABN`` / ``InPlaceABNSync``'s default): the output overwrites the input (``ctx.mark_dirty``: reusing the
  overwritten input elsewhere raises autograd's version-counter error) and backward rebuilds the normalised input from the
  output, inverting the activation and the affine step.  That needs an invertible affine step, so gamma = |weight| + eps
  (this library's rule), and an invertible activation: identity, leaky_relu with slope > 0 or elu; relu raises ValueError.

``InPlaceABNSync`` reduces its training statistics over the ranks of the default process group: every rank's per-channel
(count, mean, M2) is exchanged and merged in rank order with Chan's formula, and backward exchanges the two per-channel sums
the same way.  There is no CPU fallback.

Layers converted with ``convert_abn(model, mode, channels_last=True)`` hand a dense ``torch.channels_last`` input to
:class:`ccnet_amd.abncl.ABNChannelsLastFunction` (libccnet_abncl.so, the same arithmetic on pixel-major rows) as it lies and
return channels_last; every other input, and every layer without the attribute, runs as described above.
"""
from __future__ import annotations

import ctypes

import torch
import torch.distributed as dist

import inplace_abn

from . import _abn_lib as L
from . import abncl as _cl

__all__ = ["ABN", "InPlaceABN", "InPlaceABNSync", "ABNFunction", "convert_abn"]

_DTYPES = {torch.float32: L.CCNET_ABN_F32, torch.bfloat16: L.CCNET_ABN_BF16}


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _exchange(local, group):
    """(world, *local.shape) fp64: every rank's ``local`` in rank order.  An all-reduce of a zero-padded table is an exact
    all-gather (x + 0 = x) that both RCCL and gloo run on device tensors."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    table = torch.zeros((world,) + tuple(local.shape), dtype=torch.float64, device=local.device)
    table[rank] = local
    dist.all_reduce(table, group=group)
    return table


class ABNFunction(torch.autograd.Function):
    """y = act(gamma (x - mean) invstd + beta [+ residual]) on the device; ``cfg`` = (training, momentum, eps, activation
    code, activation parameter, inplace, process group or None)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, cfg):
        training, momentum, eps, act, param, inplace, group = cfg
        lib = L.get_lib()
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // max(N * C, 1)
        d = L.make_desc(_DTYPES[x.dtype], N, C, HW, 1, act, param,
                        L.CCNET_ABN_GAMMA_ABS_EPS if inplace else L.CCNET_ABN_GAMMA_WEIGHT, eps)
        dp = ctypes.byref(d)
        dev, s = x.device, _stream(x.device)
        w = None if weight is None else weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        saved = None
        if training:
            nbytes = lib.ccnet_abn_workspace_bytes(dp)
            if nbytes == 0:
                raise RuntimeError(f"ABN: unsupported shape {tuple(x.shape)}: {lib.last_error()}")
            buf = torch.empty(6 * C + nbytes // 8, dtype=torch.float64, device=dev)    # one allocation: local, saved, ws
            local, saved, ws = buf[:3 * C].view(3, C), buf[3 * C:6 * C].view(3, C), buf[6 * C:]
            lib.check(lib.ccnet_abn_stats(dp, x.data_ptr(), local.data_ptr(), ws.data_ptr(), nbytes, s), "ccnet_abn_stats")
            table = local.unsqueeze(0) if group is None else _exchange(local, group)
            lib.check(lib.ccnet_abn_stats_combine(dp, table.data_ptr(), table.shape[0], momentum, _p(running_mean),
                                                  _p(running_var), saved.data_ptr(), s), "ccnet_abn_stats_combine")
        y = x if inplace else torch.empty_like(x)
        lib.check(lib.ccnet_abn_forward(dp, x.data_ptr(), _p(residual), y.data_ptr(), _p(saved), _p(running_mean),
                                        _p(running_var), _p(w), _p(b), s), "ccnet_abn_forward")
        ctx.desc, ctx.training, ctx.inplace, ctx.group = d, training, inplace, group
        ctx.has_residual, ctx.weight_dtype = residual is not None, None if weight is None else weight.dtype
        if inplace:
            ctx.mark_dirty(x)
            ctx.save_for_backward(y, residual, saved, running_mean, running_var, w, b)
        else:
            ctx.save_for_backward(x, y if act != L.CCNET_ABN_IDENTITY else None, saved, running_mean, running_var, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.get_lib()
        d = ctx.desc
        dp = ctypes.byref(d)
        if ctx.inplace:
            y, residual, saved, rm, rv, w, b = ctx.saved_tensors
            src, source = y, L.CCNET_ABN_FROM_OUTPUT
        else:
            src, y, saved, rm, rv, w, b = ctx.saved_tensors
            residual, source = None, L.CCNET_ABN_FROM_INPUT
        if not ctx.training:
            saved = None
        dy = dy.contiguous()
        if dy.dtype != src.dtype:
            dy = dy.to(src.dtype)
        dev, s = dy.device, _stream(dy.device)
        C = d.C
        nbytes = lib.ccnet_abn_workspace_bytes(dp)
        buf = torch.empty(2 * C + nbytes // 8, dtype=torch.float64, device=dev)         # one allocation: sums, ws
        sums, ws = buf[:2 * C].view(2, C), buf[2 * C:]
        want_w = ctx.needs_input_grad[1] and w is not None
        want_b = ctx.needs_input_grad[2] and b is not None
        dw = torch.empty(C, dtype=torch.float32, device=dev) if want_w else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if want_b else None
        lib.check(lib.ccnet_abn_backward_reduce(dp, source, src.data_ptr(), _p(y), dy.data_ptr(), _p(residual), _p(saved),
                                                _p(rm), _p(rv), _p(w), _p(b), sums.data_ptr(), _p(dw), _p(db), ws.data_ptr(),
                                                nbytes, s), "ccnet_abn_backward_reduce")
        dx = dres = None
        if ctx.needs_input_grad[0] or (ctx.has_residual and ctx.needs_input_grad[5]):
            table = sums.unsqueeze(0) if (ctx.group is None or saved is None) else _exchange(sums, ctx.group)
            dx = torch.empty_like(dy)
            dres = torch.empty_like(dy) if ctx.has_residual and ctx.needs_input_grad[5] else None
            lib.check(lib.ccnet_abn_backward_apply(dp, source, src.data_ptr(), _p(y), dy.data_ptr(), _p(residual),
                                                   _p(saved), _p(rm), _p(rv), _p(w), _p(b), table.data_ptr(), table.shape[0],
                                                   dx.data_ptr(), _p(dres), s), "ccnet_abn_backward_apply")
        if dw is not None and ctx.weight_dtype != torch.float32:
            dw = dw.to(ctx.weight_dtype)
        if db is not None and ctx.weight_dtype != torch.float32:
            db = db.to(ctx.weight_dtype)
        return (dx if ctx.needs_input_grad[0] else None), dw, db, None, None, dres, None


class _DeviceABN:
    """The device forward shared by the three classes (a mixin in front of the ``inplace_abn`` class)."""

    inplace = False
    sync = False
    channels_last = False      # convert_abn(..., channels_last=True): dense channels_last inputs run on libccnet_abncl.so

    @property
    def fused_epilogues(self):
        """True when this layer can take segmodel's relu and residual epilogues (out-of-place mode only: relu has no
        inverse)."""
        return not self.inplace

    def _check(self, x, activation):
        if activation not in L.ACTIVATIONS:
            raise ValueError(f"ABN: unknown activation '{activation}'")
        if self.inplace and (activation == inplace_abn.ACT_RELU or
                             (activation == inplace_abn.ACT_LEAKY_RELU and not self.activation_param > 0)):
            raise ValueError(f"in-place ABN cannot invert activation '{activation}' (relu, or leaky_relu with slope "
                             f"{self.activation_param}): use identity, leaky_relu with slope > 0 or elu, or out-of-place mode")
        if self.momentum is None:
            raise ValueError("ABN: momentum=None (a cumulative average) is not supported by the device layers")
        if not x.is_cuda:
            raise RuntimeError("ABN: the input must be a HIP device tensor (ccnet_amd has no CPU fallback for the ABN "
                               "kernels)")
        if x.dtype not in _DTYPES:
            raise TypeError(f"ABN: {x.dtype} input; the device layers take float32 or bfloat16")
        if x.dim() < 2:
            raise ValueError(f"ABN: expected (N, C, ...) input, got {tuple(x.shape)}")
        if self.running_mean.dtype != torch.float32 or self.running_var.dtype != torch.float32:
            raise TypeError("ABN: the running statistics must stay float32")

    def forward(self, x, residual=None, activation=None):
        """``residual`` is added before the activation; ``activation`` overrides the module's own for this call (segmodel's
        fused epilogues pass 'relu')."""
        activation = self.activation if activation is None else activation
        self._check(x, activation)
        # a dense channels_last input that is not NCHW-contiguous as well (C = 1 and H * W = 1 tensors are both, and stay on
        # the NCHW kernels) goes to the pixel-major kernels as it lies
        pixel_major = self.channels_last and _cl.is_dense_channels_last(x) and not x.is_contiguous()
        if self.inplace and not pixel_major and not x.is_contiguous():
            raise ValueError("in-place ABN needs a contiguous NCHW or a dense channels_last input" if self.channels_last
                             else "in-place ABN needs a contiguous NCHW input")
        if not pixel_major:
            x = x.contiguous()
        if residual is not None:
            if residual.shape != x.shape:
                raise ValueError(f"ABN: residual {tuple(residual.shape)} does not match the input {tuple(x.shape)}")
            residual = _cl._dense(residual, x.dtype) if pixel_major else residual.to(x.dtype).contiguous()
        training = self.training
        if training and x.numel() // x.shape[1] <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        group = None
        if (self.sync and training and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            group = dist.group.WORLD
        param = float(self.activation_param) if activation in (inplace_abn.ACT_LEAKY_RELU, inplace_abn.ACT_ELU) else 0.0
        cfg = (training, float(self.momentum), float(self.eps), L.ACTIVATIONS[activation], param, self.inplace, group)
        function = _cl.ABNChannelsLastFunction if pixel_major else ABNFunction
        return function.apply(x, self.weight, self.bias, self.running_mean, self.running_var, residual, cfg)

    def extra_repr(self):
        return super().extra_repr() + f", inplace={self.inplace}, device=True"


class ABN(_DeviceABN, inplace_abn.ABN):
    """Device twin of ``inplace_abn.ABN``: batch norm + activation in fused HIP kernels, out of place by default."""


class InPlaceABN(_DeviceABN, inplace_abn.InPlaceABN):
    """Device twin of ``inplace_abn.InPlaceABN``: the output overwrites the input (gamma = |weight| + eps)."""

    inplace = True


class InPlaceABNSync(_DeviceABN, inplace_abn.InPlaceABNSync):
    """Device twin of ``inplace_abn.InPlaceABNSync``: in place, with statistics over the default process group's ranks."""

    inplace = True
    sync = True


_TWINS = {inplace_abn.ABN: ABN, inplace_abn.InPlaceABN: InPlaceABN, inplace_abn.InPlaceABNSync: InPlaceABNSync,
          ABN: ABN, InPlaceABN: InPlaceABN, InPlaceABNSync: InPlaceABNSync}


def convert_abn(model, mode, channels_last=False):
    """Swap every ``inplace_abn`` module of ``model`` (in place, returned) for its device twin, keeping the parameter and
    buffer tensors themselves (an optimiser built before stays valid).  ``mode``: 'device' (out-of-place arithmetic, what
    the stock layer computes) or 'inplace' (the output overwrites the input, gamma = |weight| + eps).  ``channels_last``:
    the layers take a dense channels_last input as it lies and return channels_last (libccnet_abncl.so, no layout copy);
    every other input, and every input when it is false, runs on the NCHW kernels.  Converting again switches the mode."""
    if mode not in ("device", "inplace"):
        raise ValueError(f"convert_abn: mode must be 'device' or 'inplace', not {mode!r}")
    inplace = mode == "inplace"
    for parent in list(model.modules()):
        for name, m in list(parent.named_children()):
            cls = _TWINS.get(type(m))
            if cls is None:
                continue
            if inplace and m.activation == inplace_abn.ACT_RELU:
                raise ValueError(f"convert_abn: {name} uses relu, which in-place mode cannot invert")
            new = cls(m.num_features, m.eps, m.momentum, m.affine, m.activation, m.activation_param)
            if m.affine:
                new.weight, new.bias = m.weight, m.bias
            new.running_mean, new.running_var = m.running_mean, m.running_var
            new.inplace = inplace
            new.channels_last = bool(channels_last)
            new.train(m.training)
            setattr(parent, name, new)
    return model
