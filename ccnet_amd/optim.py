"""The optimiser of the training recipe on the device (train.py:126-133, 182-183, 216-217): momentum SGD with weight decay over
the whole parameter list in ONE launch of libccnet_sgd.so, the gradients zeroed in the same pass and, optionally, the poly
learning rate read from a table on the device.

    opt = DeviceSGD(model.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4, zero_grads=True,
                    schedule=poly_schedule(1e-2, max_iter))
    loss.backward(); opt.step()            # no zero_grad() call, no LR loop: step k uses schedule[k]

The arithmetic is torch.optim.SGD's (dampening 0, no Nesterov, no maximize), every float operation rounded on its own, so the
result is bit-exact against a NumPy float32 restatement and within a few units in the last place of torch's own kernels.
There is no CPU fallback: CPU tensors, and a missing library, raise.  DeviceSGD takes float32 parameters only; bf16 parameters
with fp32 master copies are DeviceMixedSGD's (libccnet_sgdmp.so), and bf16_parameters() casts a model for it:

    bf16_parameters(model)                 # normalisation layers keep float32 affine parameters and statistics
    opt = DeviceMixedSGD(model.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4, zero_grads=True,
                         schedule=poly_schedule(1e-2, max_iter))
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _sgd_lib, _sgdmp_lib
from ._sgd_lib import SgdError
from ._sgdmp_lib import SgdmpError

__all__ = ["DeviceSGD", "DeviceMixedSGD", "bf16_parameters", "poly_schedule", "SgdError", "SgdmpError"]


def poly_schedule(base_lr: float, max_iter: int, power: float = 0.9) -> torch.Tensor:
    """float32 (max_iter,): ``base_lr * (1 - it / max_iter) ** power`` for it = 0 ... max_iter - 1, computed in Python doubles as
    train_synthetic.lr_poly does (train.py:126-127) and rounded to float32 once."""
    if max_iter < 1:
        raise ValueError(f"poly_schedule needs max_iter >= 1, got {max_iter}")
    values = [base_lr * (1.0 - float(it) / max_iter) ** power for it in range(max_iter)]
    return torch.from_numpy(np.array(values, np.float64).astype(np.float32))


class DeviceSGD(torch.optim.Optimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay=...) as one HIP launch per step.

    ``param_groups``, ``add_param_group``, ``zero_grad`` and ``state_dict`` are the stock ones: every group's ``lr``,
    ``momentum`` and ``weight_decay`` are read on every step (so torch.optim.lr_scheduler and a loop over ``param_groups`` keep
    working), ``state[p]["momentum_buffer"]`` is the buffer the kernel updates (zero-filled at construction, which makes the
    first step torch's "buffer = gradient"), and a ``state_dict()`` loads into a torch.optim.SGD over the same parameters and
    back; a buffer missing from a loaded state counts as zeros.  A parameter whose ``.grad`` is None is skipped, as in torch.

    ``zero_grads=True``: the kernel also writes zeros over every gradient it has used, and the ``.grad`` tensors stay
    allocated: the reference's in-place ``optimizer.zero_grad()``, fused.  The caller must then NOT call
    ``zero_grad(set_to_none=True)`` (the default of ``zero_grad()``): it frees the gradients, the next backward allocates new
    ones and the tables below are rebuilt on every step.

    ``schedule=`` (a float32 tensor, such as :func:`poly_schedule`'s): the learning rate of step k is ``schedule[min(k, len - 1)]``,
    read on the device from a counter that the step advances (``self.counter``, int32 on the device), times the group's
    ``lr_mult`` (default 1.0, exact); the groups' ``lr`` is then unused.  A step captured into a graph therefore replays with
    the schedule moving on, which a host-side ``lr`` cannot do.

    The tables of pointers the kernel reads are built once and reused while every ``p.data_ptr()`` and ``p.grad.data_ptr()``
    stays what it was (one host loop per step checks); when one changes they are rebuilt and uploaded from pinned memory without
    a synchronise, except during stream capture, where a changed pointer raises.  After a step every updated parameter's
    ``_version`` has risen by one.
    """

    _NAME = "DeviceSGD"                        # (in the messages that DeviceMixedSGD inherits)

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, *, zero_grads=False, schedule=None, **not_offered):
        if not_offered:                        # dampening, nesterov, maximize, foreach, fused ...
            raise ValueError(f"{self._NAME} does not offer {sorted(not_offered)}: it is momentum SGD with weight decay, dampening 0, "
                             "no Nesterov momentum and no maximize")
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        params = list(params)
        if len(params) > _sgd_lib.MAX_GROUPS and all(isinstance(g, dict) for g in params):
            raise ValueError(f"{self._NAME} takes at most {_sgd_lib.MAX_GROUPS} parameter groups, got {len(params)}")
        self.zero_grads = bool(zero_grads)
        self._device: Optional[torch.device] = None
        self._key = None                       # the pointers the tables were built from
        self._numels = None
        self._tables = None
        # (the keys torch.optim.SGD's groups carry, at the only values offered here, so that a state_dict loads there)
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=None, differentiable=False, fused=None, lr_mult=1.0)
        super().__init__(params, defaults)
        self.schedule = self.counter = None
        if schedule is not None:
            table = torch.as_tensor(schedule)
            if table.dtype != torch.float32 or table.dim() != 1 or table.numel() < 1:
                raise ValueError(f"schedule must be a float32 vector of at least one entry, got {table.dtype} {tuple(table.shape)}")
            self.schedule = table.detach().to(self._device, copy=True).contiguous()
            self.counter = torch.zeros(1, dtype=torch.int32, device=self._device)
        for group in self.param_groups:
            for p in group["params"]:
                self._buffer(p)

    # -- what is refused ------------------------------------------------------------------------------------------------
    def _check_param(self, p):
        if p.dtype != torch.float32:
            raise ValueError(f"DeviceSGD takes float32 parameters, got {p.dtype} (bf16 parameters with fp32 masters are not offered)")
        if p.device.type != "cuda":
            raise ValueError("DeviceSGD needs parameters on a HIP device (ccnet_amd has no CPU fallback for the optimiser kernels)")
        if p.is_sparse or p.layout != torch.strided or not p.is_contiguous():
            raise ValueError(f"DeviceSGD takes dense contiguous parameters, got layout {p.layout}, strides {p.stride()}")
        if self._device is None:
            self._device = p.device
        elif p.device != self._device:
            raise ValueError(f"DeviceSGD takes parameters of one device, got {self._device} and {p.device}")

    @staticmethod
    def _check_grad(p, g):
        if g.is_sparse or g.layout != torch.strided:
            raise ValueError("DeviceSGD does not take sparse gradients")
        if g.dtype != torch.float32:
            raise ValueError(f"DeviceSGD takes float32 gradients, got {g.dtype}")
        if not g.is_contiguous() or g.numel() != p.numel() or g.device != p.device:
            raise ValueError(f"DeviceSGD takes contiguous gradients on the parameter's device, got strides {g.stride()} on {g.device}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if len(self.param_groups) > _sgd_lib.MAX_GROUPS:
            raise ValueError(f"{self._NAME} takes at most {_sgd_lib.MAX_GROUPS} parameter groups, got {len(self.param_groups)}")
        if sum(len(g["params"]) for g in self.param_groups) > _sgd_lib.MAX_TENSORS:
            raise ValueError(f"{self._NAME} takes at most {_sgd_lib.MAX_TENSORS} tensors")
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._key = None                       # the buffers are new tensors

    # -- tables -----------------------------------------------------------------------------------------------------------
    def _buffer(self, p):
        state = self.state[p]
        buf = state.get("momentum_buffer")
        if buf is None:
            buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return buf

    def _rebuild(self, lib, rows, key):
        if torch.cuda.is_current_stream_capturing():
            raise SgdError("DeviceSGD: a parameter, gradient or momentum buffer has moved since the tables were built; they "
                           "cannot be rebuilt during stream capture (run one step before capturing and keep the .grad tensors)")
        for p, g, buf, _ in rows:
            self._check_param(p)
            if g is not None:
                self._check_grad(p, g)
            if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() != p.numel() or buf.device != p.device:
                raise ValueError("DeviceSGD: a momentum buffer is not a contiguous float32 tensor of its parameter's size and device")
        n = len(rows)
        host = torch.empty((n, _sgd_lib.TENSOR_WORDS), dtype=torch.int64, pin_memory=True)
        table = host.numpy()
        table[:, :3] = np.array(key, np.int64).reshape(n, 3)
        table[:, _sgd_lib.NUMEL] = [p.numel() for p, _, _, _ in rows]
        table[:, _sgd_lib.GROUP] = [k for _, _, _, k in rows]
        numels = table[:, _sgd_lib.NUMEL].tolist()
        if self._tables is None or numels != self._numels:
            chunks = lib.plan(numels)
            chunks_host = torch.empty(chunks.shape, dtype=torch.int32, pin_memory=True)
            chunks_host.numpy()[:] = chunks
            chunks_dev = chunks_host.to(self._device, non_blocking=True)
        else:
            chunks_host, chunks_dev = self._tables[2], self._tables[3]
        self._tables = (host, host.to(self._device, non_blocking=True), chunks_host, chunks_dev)
        self._key, self._numels = key, numels

    # -- the step ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        if len(groups) > _sgd_lib.MAX_GROUPS:
            raise ValueError(f"DeviceSGD takes at most {_sgd_lib.MAX_GROUPS} parameter groups, got {len(groups)}")
        rows, key = [], []
        hyper = np.zeros((3, len(groups)), np.float32)
        for k, group in enumerate(groups):
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise ValueError("DeviceSGD offers neither dampening nor Nesterov momentum nor maximize")
            hyper[:, k] = (float(group.get("lr_mult", 1.0)) if self.schedule is not None else float(group["lr"]),
                           float(group["weight_decay"]), float(group["momentum"]))
            for p in group["params"]:
                g, buf = p.grad, self._buffer(p)
                rows.append((p, g, buf, k))
                key += (p.data_ptr(), 0 if g is None else g.data_ptr(), buf.data_ptr())
        if not rows:
            return loss
        lib = _sgd_lib.get_lib()
        if key != self._key:
            self._rebuild(lib, rows, key)
        tensors_host, tensors_dev, chunks_host, chunks_dev = self._tables
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            lib.check(lib.ccnet_sgd_step(
                tensors_host.data_ptr(), tensors_dev.data_ptr(), len(rows), chunks_host.data_ptr(), chunks_dev.data_ptr(),
                chunks_host.shape[0], hyper[0].ctypes.data, hyper[1].ctypes.data, hyper[2].ctypes.data, len(groups),
                None if self.schedule is None else self.schedule.data_ptr(),
                0 if self.schedule is None else self.schedule.numel(),
                None if self.counter is None else self.counter.data_ptr(), int(self.zero_grads), 0, stream),
                "ccnet_sgd_step")
        # the kernel wrote behind autograd's back: say so (a cache keyed on _version must see the update)
        touched = [t for p, g, buf, _ in rows if g is not None for t in ((p, buf, g) if self.zero_grads else (p, buf))]
        if touched:
            torch.autograd.graph.increment_version(touched)
        return loss


class DeviceMixedSGD(DeviceSGD):
    """:class:`DeviceSGD` over a list that mixes float32 parameters with bf16 parameters, one launch of libccnet_sgdmp.so per step
    (DESIGN.md §23).

    A float32 parameter is updated exactly as DeviceSGD updates it, bit for bit.  A bf16 parameter takes a bf16 gradient and has
    a float32 master, ``state[p]["master_param"]`` (created as ``p.detach().float()``), beside its float32
    ``state[p]["momentum_buffer"]``: the kernel widens the gradient, steps the master in float32 with DeviceSGD's arithmetic and
    writes ``p = bf16(master)``, to nearest, ties to even.  The parameter itself is never read: the master is the truth, and an
    update too small to move a bf16 number still accumulates.  Whoever writes the parameters behind the optimiser's back (a
    checkpoint loaded into the model) calls :meth:`masters_from_params` afterwards.

    Groups, ``zero_grads``, ``schedule``, the cached tables and their rebuild rule, the error under capture and the version
    increments are DeviceSGD's.  ``state_dict()`` carries masters and buffers in float32 and ``load_state_dict()`` keeps them so
    (the stock loader would cast them to the parameter's bf16); after a load every bf16 parameter is rewritten as ``bf16(master)``.
    A buffer missing from a loaded state counts as zeros, a missing master is seeded from the parameter.  The state loads into a
    torch.optim.SGD over float32 copies of the parameters (which ignores ``master_param``) and that optimiser's state loads back;
    the float32 copies themselves then go into the masters by hand, ``opt.state[p]["master_param"].copy_(q)``.
    """

    _NAME = "DeviceMixedSGD"

    # -- what is refused ------------------------------------------------------------------------------------------------
    def _check_param(self, p):
        if p.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"DeviceMixedSGD takes float32 and bfloat16 parameters, got {p.dtype}")
        if p.device.type != "cuda":
            raise ValueError("DeviceMixedSGD needs parameters on a HIP device (ccnet_amd has no CPU fallback for the optimiser kernels)")
        if p.is_sparse or p.layout != torch.strided or not p.is_contiguous():
            raise ValueError(f"DeviceMixedSGD takes dense contiguous parameters, got layout {p.layout}, strides {p.stride()}")
        if self._device is None:
            self._device = p.device
        elif p.device != self._device:
            raise ValueError(f"DeviceMixedSGD takes parameters of one device, got {self._device} and {p.device}")

    @staticmethod
    def _check_grad(p, g):
        if g.is_sparse or g.layout != torch.strided:
            raise ValueError("DeviceMixedSGD does not take sparse gradients")
        if g.dtype != p.dtype:
            raise ValueError(f"DeviceMixedSGD takes a gradient of its parameter's dtype, got {g.dtype} for a {p.dtype} parameter")
        if not g.is_contiguous() or g.numel() != p.numel() or g.device != p.device:
            raise ValueError(f"DeviceMixedSGD takes contiguous gradients on the parameter's device, got strides {g.stride()} on {g.device}")

    # -- state ------------------------------------------------------------------------------------------------------------
    def _buffer(self, p):
        state = self.state[p]
        buf = state.get("momentum_buffer")
        if buf is None:
            buf = state["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        if p.dtype == torch.bfloat16 and state.get("master_param") is None:
            state["master_param"] = p.detach().to(torch.float32, memory_format=torch.contiguous_format)
        return buf

    def _bf16_params(self):
        return [p for group in self.param_groups for p in group["params"] if p.dtype == torch.bfloat16]

    @torch.no_grad()
    def masters_from_params(self):
        """Every master <- float(its bf16 parameter), in place: call it after the parameters were written from outside."""
        for p in self._bf16_params():
            self._buffer(p)
            self.state[p]["master_param"].copy_(p)

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the stock loader has cast every state tensor to its parameter's dtype: take the float32 ones again from the source
        saved = [k for group in state_dict["param_groups"] for k in group["params"]]
        own = [p for group in self.param_groups for p in group["params"]]
        for key, p in zip(saved, own):
            source = state_dict["state"].get(key, {})
            for name in ("momentum_buffer", "master_param"):
                value = source.get(name)
                if p.dtype == torch.bfloat16 and isinstance(value, torch.Tensor):
                    self.state[p][name] = value.detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
                elif name == "master_param":
                    self.state[p].pop(name, None)          # (a float32 parameter has none; a missing one is seeded below)
            self._buffer(p)
            if p.dtype == torch.bfloat16:
                p.copy_(self.state[p]["master_param"])
        self._key = None

    # -- tables -----------------------------------------------------------------------------------------------------------
    def _rebuild(self, lib, rows, key):
        if torch.cuda.is_current_stream_capturing():
            raise SgdmpError("DeviceMixedSGD: a parameter, gradient, master or momentum buffer has moved since the tables were "
                             "built; they cannot be rebuilt during stream capture (run one step before capturing and keep the "
                             ".grad tensors)")
        for p, g, buf, master, _ in rows:
            self._check_param(p)
            if g is not None:
                self._check_grad(p, g)
            for what, t in (("momentum buffer", buf), ("master", master)):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != p.device):
                    raise ValueError(f"DeviceMixedSGD: a {what} is not a contiguous float32 tensor of its parameter's size and device")
        n = len(rows)
        host = torch.empty((n, _sgdmp_lib.TENSOR_WORDS), dtype=torch.int64, pin_memory=True)
        table = host.numpy()
        pointers = np.array(key, np.int64).reshape(n, 4)
        table[:, :3] = pointers[:, :3]
        table[:, _sgdmp_lib.M] = pointers[:, 3]
        table[:, _sgdmp_lib.NUMEL] = [row[0].numel() for row in rows]
        table[:, _sgdmp_lib.GROUP] = [row[4] for row in rows]
        numels = table[:, _sgdmp_lib.NUMEL].tolist()
        if self._tables is None or numels != self._numels:
            chunks = lib.plan(numels)
            chunks_host = torch.empty(chunks.shape, dtype=torch.int32, pin_memory=True)
            chunks_host.numpy()[:] = chunks
            chunks_dev = chunks_host.to(self._device, non_blocking=True)
        else:
            chunks_host, chunks_dev = self._tables[2], self._tables[3]
        self._tables = (host, host.to(self._device, non_blocking=True), chunks_host, chunks_dev)
        self._key, self._numels = key, numels

    # -- the step ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        if len(groups) > _sgdmp_lib.MAX_GROUPS:
            raise ValueError(f"DeviceMixedSGD takes at most {_sgdmp_lib.MAX_GROUPS} parameter groups, got {len(groups)}")
        rows, key = [], []
        hyper = np.zeros((3, len(groups)), np.float32)
        for k, group in enumerate(groups):
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise ValueError("DeviceMixedSGD offers neither dampening nor Nesterov momentum nor maximize")
            hyper[:, k] = (float(group.get("lr_mult", 1.0)) if self.schedule is not None else float(group["lr"]),
                           float(group["weight_decay"]), float(group["momentum"]))
            for p in group["params"]:
                g, buf = p.grad, self._buffer(p)
                master = self.state[p].get("master_param") if p.dtype == torch.bfloat16 else None
                rows.append((p, g, buf, master, k))
                key += (p.data_ptr(), 0 if g is None else g.data_ptr(), buf.data_ptr(), 0 if master is None else master.data_ptr())
        if not rows:
            return loss
        lib = _sgdmp_lib.get_lib()
        if key != self._key:
            self._rebuild(lib, rows, key)
        tensors_host, tensors_dev, chunks_host, chunks_dev = self._tables
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            lib.check(lib.ccnet_sgdmp_step(
                tensors_host.data_ptr(), tensors_dev.data_ptr(), len(rows), chunks_host.data_ptr(), chunks_dev.data_ptr(),
                chunks_host.shape[0], hyper[0].ctypes.data, hyper[1].ctypes.data, hyper[2].ctypes.data, len(groups),
                None if self.schedule is None else self.schedule.data_ptr(),
                0 if self.schedule is None else self.schedule.numel(),
                None if self.counter is None else self.counter.data_ptr(), int(self.zero_grads), 0, stream),
                "ccnet_sgdmp_step")
        # the kernel wrote behind autograd's back: say so (a cache keyed on _version must see the update)
        touched = [t for p, g, buf, master, _ in rows if g is not None
                   for t in (p, buf, master, g if self.zero_grads else None) if t is not None]
        if touched:
            torch.autograd.graph.increment_version(touched)
        return loss


def bf16_parameters(model: torch.nn.Module) -> torch.nn.Module:
    """Cast every floating-point parameter of ``model`` to bf16 in place (the Parameter objects stay, gradients of another dtype are
    dropped), except those of normalisation layers: ABN / InPlaceABN / InPlaceABNSync (the stock restatement and both device
    kinds, which all derive from ``inplace_abn.ABN``), BatchNorm*, InstanceNorm*, GroupNorm and LayerNorm keep float32 affine
    parameters; buffers (running statistics) are not touched.  Returns the model: what DeviceMixedSGD then optimises."""
    import inplace_abn
    norms = (inplace_abn.ABN, torch.nn.modules.batchnorm._NormBase, torch.nn.GroupNorm, torch.nn.LayerNorm)
    for module in model.modules():
        if isinstance(module, norms):
            continue
        for p in module._parameters.values():
            if p is None or not p.is_floating_point() or p.dtype == torch.bfloat16:
                continue
            p.data = p.data.to(torch.bfloat16)
            if p.grad is not None and p.grad.dtype != torch.bfloat16:
                p.grad = None
    return model
