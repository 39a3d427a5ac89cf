"""Synthetic-data DDP training driver for the Cityscapes-shape half of BASELINE.json's metric
("imgs/sec 1/2/4/8 GPU").

It replaces the reference's ``train.py`` + ``engine.py`` (which need apex-era APIs and the Cityscapes files) with
the same training step on random data, one process per GPU:

    model      ccnet_amd.segmodel.Seg_Model(19, CriterionDSN(), recurrence=2)       train.py:160-164
               --ohem: CriterionOhemDSN(thresh=--ohem-thres, min_kept=--ohem-keep)   train.py:117-122,168-171
               --lovasz: CriterionOhemDSN2 (CE + Lovász-softmax, DSN head unused)   loss/criterion.py:59-78
               --fused-dsn: ccnet_amd.dsn.CriterionDSN (the up-sample inside the loss kernels); with --ohem,
               CriterionOhemDSN(fused_aux=True); refused with --lovasz
               --fused-ohem: ccnet_amd.ohemdsn.CriterionOhemDSN (implies --ohem: the OHEM head up-samples inside its kernels
               too); refused with --lovasz and with --fused-dsn
               --fused-lovasz: ccnet_amd.celovasz.CriterionOhemDSN2 (implies --lovasz: the up-sample, the softmax and the
               cross-entropy inside the Lovász criterion's kernels); refused with --ohem, --fused-dsn and --fused-ohem
               --abn device|inplace: every inplace_abn layer swapped for its HIP twin (ccnet_amd.abn.convert_abn)
    data       images randn(b,3,769,769), labels randint(0,19) with ~5 % set to 255 train.py:28-33 (crop 769)
               --device-augment: synthetic uint8 1024 x 2048 frames and Cityscapes id labels, made once; every step draws
               the reference's scale, offsets and mirror and builds its batch with ccnet_amd.augment.DeviceAugment
               (dataset/datasets.py:173-210 as one HIP gather); composes with every criterion flag
    optimiser  SGD(lr 1e-2, momentum 0.9, weight decay 1e-4 ... 5e-4), poly LR      train.py:126-133,183
               --device-sgd: ccnet_amd.optim.DeviceSGD (the whole update, the gradient zeroing and the poly LR in one HIP
               launch per step, the LR from a table on the device); composes with every other flag
               --bf16-params: bf16 parameters, gradients and images without autocast (ccnet_amd.optim.bf16_parameters; the
               normalisation layers keep float32 affine parameters), both heads' logits cast to float32 in front of the
               criterion, and ccnet_amd.optim.DeviceMixedSGD (float32 masters inside the one launch); refused with --bf16,
               --device-sgd and --cpu
    convs      --device-conv3: every eligible 3x3 convolution (stride 1, padding == dilation) swapped for the library's implicit
               GEMM (ccnet_amd.conv3.convert_conv3x3), the images -- and with the stock optimiser the model -- in
               torch.channels_last (DeviceSGD and DeviceMixedSGD walk contiguous parameters: there the activations alone
               carry the format); needs --bf16 or --bf16-params; refused with --cpu, and with --abn device|inplace
               (NCHW-only layers) unless --abn-channels-last puts those layers on their pixel-major kernels
               (ccnet_amd.abncl: no layout copy between a converted convolution and its normalisation layer)
    parallel   DistributedDataParallel over RCCL (backend "nccl"), SyncBN statistics engine.py:52-57,75
               per-rank seed = rank                                                  train.py:154-155

Launch:   python -m ccnet_amd.train_synthetic --steps 10 --batch-per-gpu 1
          python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
                 -m ccnet_amd.train_synthetic --steps 10 --batch-per-gpu 1
Rank 0 prints one JSON line with images/s over the timed steps (max over ranks, barrier + synchronize on both
sides) -- the optimiser step and the gradient all-reduce are inside the timed region.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def lr_poly(base_lr, it, max_it, power=0.9):
    """train.py:126-127"""
    return base_lr * (1.0 - float(it) / max_it) ** power


def synthetic_batch(batch, size, num_classes, device, generator):
    images = torch.randn(batch, 3, size, size, device=device, generator=generator)
    labels = torch.randint(0, num_classes, (batch, size, size), device=device, generator=generator)
    ignore = torch.rand(batch, size, size, device=device, generator=generator) < 0.05
    return images, labels.masked_fill(ignore, 255)


class AugmentedSource:
    """--device-augment: ``batch`` synthetic uint8 frames and id labels, packed on the device once; ``next()`` draws each
    sample's parameters as the reference's dataset would (generators of its own, seeded per rank) and returns the batch that
    DeviceAugment makes of them."""

    def __init__(self, batch, frame, size, device, seed):
        import random

        import numpy as np

        from . import augment
        if device.type != "cuda":
            raise RuntimeError("--device-augment needs a HIP device (ccnet_amd has no CPU fallback for the input-pipeline kernel)")
        self.augment, self.crop, self.frame = augment, (size, size), tuple(frame)
        self.rng, self.np_rng = random.Random(seed), np.random.RandomState(seed)
        data = np.random.RandomState(seed)
        h, w = self.frame
        self.frames = [data.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(batch)]
        self.labels = [data.randint(0, 34, (h, w)).astype(np.uint8) for _ in range(batch)]
        frames, labels, _ = augment.pack(self.frames, self.labels, self.draw())
        self.frames_dev, self.labels_dev = frames.to(device), labels.to(device)
        self.run = augment.DeviceAugment(self.crop, (104.00698793, 116.66876762, 122.67891434), 255,
                                         augment.CITYSCAPES_ID_TO_TRAINID, "rgb")       # train.py's IMG_MEAN

    def draw(self):
        h, w = self.frame
        return [self.augment.draw_params(h, w, self.crop, rng=self.rng, np_rng=self.np_rng) for _ in self.frames]

    def next(self):
        # (only the descriptor table changes from step to step: the frames stay where they are)
        desc = self.augment.descriptors([f.shape[:2] for f in self.frames], self.draw(), pin=True)
        return self.run(self.frames_dev, self.labels_dev, desc)


class Float32Logits(torch.nn.Module):
    """--bf16-params: the criterion behind a cast of every head's logits to float32 (the criteria's kernels take float32)"""

    def __init__(self, criterion):
        super().__init__()
        self.criterion = criterion

    def forward(self, preds, target):
        return self.criterion([p.float() for p in preds], target)


def run(args, model_factory=None, quiet=False):
    """One training job on the calling rank; returns the result dict (rank 0) or None.  ``quiet`` suppresses the
    JSON line (bench.py embeds the result in its own line)."""
    check_args(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = torch.cuda.is_available() and not args.cpu
    device = torch.device("cuda", local) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
        # train.py:152 sets cudnn.benchmark unconditionally.  On ROCm that makes MIOpen search its solvers per convolution
        # configuration at first use: for ResNet-101 at 769 x 769 the search alone ran past a 10-minute limit on an MI355X box with
        # an empty MIOpen cache (measured, round 4) -- opt-in only.  Tri-state: without the option the process-wide flag is left as
        # the embedding process set it; --cudnn-benchmark / --no-cudnn-benchmark set it.
        if getattr(args, "cudnn_benchmark", None) is not None:
            torch.backends.cudnn.benchmark = bool(args.cudnn_benchmark)
    ddp = world > 1 or getattr(args, "force_ddp", False)      # (--force-ddp: the RCCL / DDP path on a single GPU)
    if ddp and not dist.is_initialized():
        dist.init_process_group("nccl" if use_cuda else "gloo")
    torch.manual_seed(args.seed + rank)                       # per-rank seed (train.py:154-155)
    source = None
    if getattr(args, "device_augment", False):
        source = AugmentedSource(args.batch_per_gpu, args.augment_frame, args.size, device, args.seed + rank)

    if model_factory is None:
        from .segmodel import CriterionDSN, CriterionOhemDSN, CriterionOhemDSN2, Seg_Model
        fused_dsn = getattr(args, "fused_dsn", False)
        if getattr(args, "fused_lovasz", False):
            from .celovasz import CriterionOhemDSN2 as FusedCriterionOhemDSN2
            criterion = FusedCriterionOhemDSN2()
        elif getattr(args, "lovasz", False):
            criterion = CriterionOhemDSN2()
        elif getattr(args, "fused_ohem", False):
            from .ohemdsn import CriterionOhemDSN as FusedCriterionOhemDSN
            criterion = FusedCriterionOhemDSN(thresh=args.ohem_thres, min_kept=args.ohem_keep)
        elif getattr(args, "ohem", False):
            criterion = CriterionOhemDSN(thresh=args.ohem_thres, min_kept=args.ohem_keep, fused_aux=fused_dsn)
        elif fused_dsn:
            from .dsn import CriterionDSN as FusedCriterionDSN
            criterion = FusedCriterionDSN()
        else:
            criterion = CriterionDSN()
        model = Seg_Model(args.num_classes, criterion=criterion, recurrence=args.recurrence)
    else:
        model = model_factory()
    abn_mode = getattr(args, "abn", None)
    abn_channels_last = getattr(args, "abn_channels_last", False)
    if abn_mode in ("device", "inplace"):
        from .abn import convert_abn
        # (--abn-channels-last: the layers take the converted convolutions' channels_last activations as they lie, and
        # native_batch_norm_for_bf16_channels_last below finds no stock layer left to swap)
        convert_abn(model, abn_mode, channels_last=abn_channels_last)
    device_conv3 = getattr(args, "device_conv3", False)
    if device_conv3:
        if not use_cuda:
            raise RuntimeError("--device-conv3 needs a HIP device (ccnet_amd has no CPU fallback for the convolution kernels)")
        from . import conv3 as conv3_module
        from .conv3 import convert_conv3x3, native_batch_norm_for_bf16_channels_last
        copies_before = conv3_module.layout_copies
        converted = convert_conv3x3(model)
        # (the stock normalisation layers now see bf16 channels_last activations: conv3.NativeChannelsLast says what that needs)
        native_batch_norm_for_bf16_channels_last(model)
    model = model.to(device).train()
    if device_conv3:
        # the activations carry the format from the images on (a convolution's output follows a channels_last input).  The
        # parameters follow only where the optimiser takes strided ones: DeviceSGD and DeviceMixedSGD walk contiguous memory, and
        # the converted layers pack their weight from the parameter's own (Cout, Cin, 3, 3) layout
        if not (getattr(args, "bf16_params", False) or getattr(args, "device_sgd", False)):
            from .conv3 import DeviceConv3x3
            model = model.to(memory_format=torch.channels_last)
            for m in model.modules():
                if isinstance(m, DeviceConv3x3):
                    m.weight.data = m.weight.data.contiguous()
    bf16_params = getattr(args, "bf16_params", False)
    if bf16_params:
        if not use_cuda:
            raise RuntimeError("--bf16-params needs a HIP device (ccnet_amd has no CPU fallback for the optimiser kernels)")
        from .optim import bf16_parameters
        bf16_parameters(model)
        if getattr(model, "criterion", None) is not None:
            model.criterion = Float32Logits(model.criterion)
    if use_cuda and (abn_mode is not None or getattr(args, "fused_dsn", False) or getattr(args, "fused_ohem", False)
                     or getattr(args, "fused_lovasz", False)):
        torch.cuda.reset_peak_memory_stats(device)
    net = model
    if ddp:
        # CriterionOhemDSN2 leaves the DSN head's output unused: DDP must not wait for its gradients
        lovasz = getattr(args, "lovasz", False) or getattr(args, "fused_lovasz", False)
        extra = {"find_unused_parameters": True} if lovasz else {}
        net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local] if use_cuda else None,
                                                        broadcast_buffers=False, **extra)
    total = args.warmup + args.steps
    device_sgd = getattr(args, "device_sgd", False)
    if bf16_params:
        from .optim import DeviceMixedSGD, poly_schedule
        # (as with --device-sgd: the kernel zeroes the gradients and reads step k's LR from the table)
        opt = DeviceMixedSGD(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=args.weight_decay, zero_grads=True,
                             schedule=poly_schedule(args.lr, max(total, 1)))
        device_sgd = True                                     # (for the step below: no zero_grad() call, no LR loop)
    elif device_sgd:
        if not use_cuda:
            raise RuntimeError("--device-sgd needs a HIP device (ccnet_amd has no CPU fallback for the optimiser kernels)")
        from .optim import DeviceSGD, poly_schedule
        # (the kernel zeroes the gradients and reads step k's LR from the table: no zero_grad() call and no LR loop below)
        opt = DeviceSGD(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=args.weight_decay, zero_grads=True,
                        schedule=poly_schedule(args.lr, max(total, 1)))
    else:
        opt = torch.optim.SGD(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=args.weight_decay)
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed + rank)

    def step(it):
        if not device_sgd:
            for g in opt.param_groups:
                g["lr"] = lr_poly(args.lr, it, max(total, 1))
        if source is not None:
            images, labels = source.next()
        else:
            images, labels = synthetic_batch(args.batch_per_gpu, args.size, args.num_classes, device, gen)
        if bf16_params:
            images = images.to(torch.bfloat16)
        if device_conv3:
            images = images.contiguous(memory_format=torch.channels_last)
        if not device_sgd:
            opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.bf16 and use_cuda):
            loss = net(images, labels)
        loss.backward()
        opt.step()
        return loss

    def fence():
        if ddp:
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    loss = None
    losses = []                                               # (--abn given) every step's loss, read after the timed window
    for it in range(args.warmup):
        loss = step(it)
        if abn_mode is not None:
            losses.append(loss.detach())
    fence()
    t0 = time.perf_counter()
    for it in range(args.warmup, total):
        loss = step(it)
        if abn_mode is not None:
            losses.append(loss.detach())
    fence()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if ddp:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    result = None
    if rank == 0:
        result = {
            "metric": "CCNet (ResNet-101 + RCCA R=%d) synthetic train step, images/s" % args.recurrence,
            "value": round(args.steps * args.batch_per_gpu * world / elapsed, 3), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 2), "scaling": "weak",
            "dtype": "bf16-params" if bf16_params else "bf16-autocast" if args.bf16 else "f32", "data": "synthetic",
            "config": {"image": [3, args.size, args.size], "per_gpu_batch": args.batch_per_gpu,
                       "global_batch": args.batch_per_gpu * world, "parallelism": f"ddp{world}+syncbn",
                       "optimizer": "sgd+poly"},
            "final_loss": round(float(loss.detach().float().item()), 4) if loss is not None else None,
        }
        if getattr(args, "ohem", False):
            result["criterion"] = "ohem"
        if getattr(args, "lovasz", False):
            result["criterion"] = "lovasz"
        if getattr(args, "fused_dsn", False):
            result["criterion"] = "ohem+dsn-fused" if getattr(args, "ohem", False) else "dsn-fused"
            if use_cuda:
                result["max_memory_allocated_mb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
        if getattr(args, "fused_ohem", False):
            result["criterion"] = "ohem-fused"
            if use_cuda:
                result["max_memory_allocated_mb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
        if getattr(args, "fused_lovasz", False):
            result["criterion"] = "lovasz-fused"
            if use_cuda:
                result["max_memory_allocated_mb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
        if device_sgd:
            result["config"]["optimizer"] = "device-mixed-sgd+poly" if bf16_params else "device-sgd+poly"
        if device_conv3:
            result["config"]["conv3"] = "device"
            result["config"]["conv3_layers"] = converted
            result["layout_copies"] = conv3_module.layout_copies - copies_before
        if source is not None:
            result["data"] = "synthetic uint8 %d x %d frames through DeviceAugment" % source.frame
        if abn_mode is not None:
            result["abn"] = abn_mode
            if abn_channels_last:
                result["abn_channels_last"] = True
            result["step_losses"] = [round(float(v.float().item()), 6) for v in losses]
            if use_cuda:
                result["max_memory_allocated_mb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
        if not quiet:
            print(json.dumps(result), flush=True)
    if ddp and args.destroy_group:
        dist.destroy_process_group()
    return result


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-per-gpu", type=int, default=1)
    ap.add_argument("--size", type=int, default=769, help="square crop (train.py: 769)")
    ap.add_argument("--num-classes", type=int, default=19)
    ap.add_argument("--recurrence", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bf16", action="store_true", help="autocast to bf16: convolutions in bf16, the attention core on the pixel-major bf16 kernels (fp32 attention / softmax / accumulate)")
    ap.add_argument("--cudnn-benchmark", dest="cudnn_benchmark", action="store_true", default=None,
                    help="set torch.backends.cudnn.benchmark as train.py:152 does (MIOpen then searches its solvers per convolution "
                         "configuration at first use: minutes with an empty cache); default: leave the process-wide flag untouched")
    ap.add_argument("--no-cudnn-benchmark", dest="cudnn_benchmark", action="store_false")
    crit = ap.add_mutually_exclusive_group()
    crit.add_argument("--ohem", action="store_true", help="train with CriterionOhemDSN (OHEM cross-entropy on the device), as "
                                                          "train.py --ohem True")
    crit.add_argument("--lovasz", action="store_true", help="train with CriterionOhemDSN2: cross-entropy + Lovász-softmax (on the "
                                                            "device) of the main logits, as loss/criterion.py:59-78")
    ap.add_argument("--fused-dsn", action="store_true",
                    help="cross-entropy heads that up-sample inside their HIP kernels (ccnet_amd.dsn): the device CriterionDSN, or "
                         "with --ohem the DSN head of CriterionOhemDSN (fused_aux=True); refused with --lovasz, whose criterion "
                         "needs the full-resolution map; the JSON line then reports criterion dsn-fused (ohem+dsn-fused) and "
                         "max_memory_allocated_mb")
    ap.add_argument("--fused-ohem", action="store_true",
                    help="the whole --ohem criterion on kernels that up-sample as they read (ccnet_amd.ohemdsn.CriterionOhemDSN: "
                         "threshold search, keep decision and both heads' gradients from the low-resolution logits); implies "
                         "--ohem; refused with --lovasz and with --fused-dsn; the JSON line then reports criterion ohem-fused "
                         "and max_memory_allocated_mb")
    ap.add_argument("--fused-lovasz", action="store_true",
                    help="the whole --lovasz criterion on kernels that up-sample and soft-max as they read "
                         "(ccnet_amd.celovasz.CriterionOhemDSN2: the Lovász errors, the cross-entropy and the gradient from the "
                         "low-resolution logits); implies --lovasz; refused with --ohem, --fused-dsn and --fused-ohem; the JSON "
                         "line then reports criterion lovasz-fused and max_memory_allocated_mb")
    ap.add_argument("--abn", choices=("torch", "device", "inplace"), default=None,
                    help="normalisation layers: torch (the default: the stock inplace_abn restatement), device (the HIP ABN "
                         "kernels, out of place, relu and residual adds fused in the residual units) or inplace (HIP ABN "
                         "kernels writing over their input, gamma = |weight| + eps); when given, the JSON line also reports "
                         "abn, step_losses and max_memory_allocated_mb")
    ap.add_argument("--device-augment", action="store_true",
                    help="feed the step through the device input pipeline (ccnet_amd.augment): synthetic uint8 frames and "
                         "Cityscapes id labels made once, each step's random scale 0.7 ... 2.1, pad, crop to --size, mirror and "
                         "label remap done by one HIP kernel; composes with every criterion flag; needs a HIP device")
    ap.add_argument("--augment-frame", type=int, nargs=2, default=[1024, 2048], metavar=("H", "W"),
                    help="source frame size of --device-augment (Cityscapes: 1024 2048)")
    ap.add_argument("--device-sgd", action="store_true",
                    help="the optimiser step on the device (ccnet_amd.optim.DeviceSGD): momentum, weight decay, the zeroing of "
                         "the gradients and the poly learning rate, read from a table on the device, in one HIP launch over "
                         "every parameter; composes with every criterion flag, --abn, --bf16 and --device-augment; needs a HIP "
                         "device; the JSON line then reports optimizer device-sgd+poly")
    ap.add_argument("--bf16-params", action="store_true",
                    help="bf16 parameters and gradients with float32 masters in the optimiser (ccnet_amd.optim.bf16_parameters + "
                         "DeviceMixedSGD, one HIP launch per step with the zeroing and the poly learning rate): bf16 images, no "
                         "autocast, the normalisation layers' parameters and both heads' logits in float32; refused with "
                         "--bf16, --device-sgd and --cpu; needs a HIP device; the JSON line then reports dtype bf16-params and "
                         "optimizer device-mixed-sgd+poly")
    ap.add_argument("--device-conv3", action="store_true",
                    help="every eligible 3x3 convolution (stride 1, padding == dilation, groups 1, channel counts divisible by 8) "
                         "on the library's implicit-GEMM kernels (ccnet_amd.conv3.convert_conv3x3), the images (and, with the stock "
                         "optimiser, the model) in torch.channels_last; needs --bf16 or --bf16-params; refused with --abn device|inplace, whose layers are "
                         "NCHW-only (unless --abn-channels-last is given), and with --cpu; the JSON line then reports config.conv3 device")
    ap.add_argument("--abn-channels-last", action="store_true",
                    help="with --abn device|inplace and --device-conv3: the device ABN layers on their pixel-major kernels "
                         "(ccnet_amd.abncl), which take the converted convolutions' channels_last activations with no layout "
                         "copy; the JSON line then reports abn_channels_last true")
    ap.add_argument("--ohem-thres", type=float, default=0.6, help="OHEM probability threshold (train.py: 0.6)")
    ap.add_argument("--ohem-keep", type=int, default=200000, help="OHEM minimum kept pixels (train.py: 200000)")
    ap.add_argument("--cpu", action="store_true", help="tests only: gloo on CPU with an injected model")
    ap.add_argument("--no-destroy-group", dest="destroy_group", action="store_false")
    ap.add_argument("--force-ddp", action="store_true", help="wrap the model in DistributedDataParallel (RCCL process group) even at "
                                                             "WORLD_SIZE = 1: the multi-GPU code path on the one GPU a test box has")
    return ap


def check_args(args):
    """Combinations the criteria and the optimisers cannot serve; raises ValueError."""
    if getattr(args, "bf16_params", False):
        if getattr(args, "bf16", False):
            raise ValueError("--bf16-params cannot be combined with --bf16: the parameters are bf16 already and nothing is left "
                             "for autocast to cast")
        if getattr(args, "device_sgd", False):
            raise ValueError("--bf16-params cannot be combined with --device-sgd: DeviceSGD takes float32 parameters only, "
                             "--bf16-params brings DeviceMixedSGD")
        if getattr(args, "cpu", False):
            raise ValueError("--bf16-params cannot be combined with --cpu: it needs a HIP device (ccnet_amd has no CPU fallback "
                             "for the optimiser kernels)")
    if getattr(args, "abn_channels_last", False):
        if getattr(args, "abn", None) not in ("device", "inplace"):
            raise ValueError("--abn-channels-last needs --abn device or --abn inplace: it selects the device ABN layers' "
                             "channels_last kernels")
        if not getattr(args, "device_conv3", False):
            raise ValueError("--abn-channels-last needs --device-conv3: only the converted convolutions put the activations "
                             "in channels_last")
    if getattr(args, "device_conv3", False):
        if not (getattr(args, "bf16", False) or getattr(args, "bf16_params", False)):
            raise ValueError("--device-conv3 needs --bf16 or --bf16-params: the convolution kernels take bf16 activations")
        if getattr(args, "abn", None) in ("device", "inplace") and not getattr(args, "abn_channels_last", False):
            raise ValueError("--device-conv3 cannot be combined with --abn device|inplace: the device ABN layers are NCHW-only, "
                             "the convolution kernels channels_last")
        if getattr(args, "cpu", False):
            raise ValueError("--device-conv3 cannot be combined with --cpu: it needs a HIP device (ccnet_amd has no CPU fallback "
                             "for the convolution kernels)")
    if getattr(args, "fused_dsn", False) and getattr(args, "lovasz", False):
        raise ValueError("--fused-dsn cannot be combined with --lovasz: CriterionOhemDSN2 takes the Lovász-softmax of the "
                         "full-resolution map and leaves the DSN head unused")
    if getattr(args, "fused_ohem", False) and getattr(args, "lovasz", False):
        raise ValueError("--fused-ohem cannot be combined with --lovasz: it selects the OHEM criterion, CriterionOhemDSN2 is "
                         "another one")
    if getattr(args, "fused_ohem", False) and getattr(args, "fused_dsn", False):
        raise ValueError("--fused-ohem cannot be combined with --fused-dsn: it already up-samples both heads inside its kernels "
                         "(--ohem --fused-dsn keeps the stock up-sample of the OHEM head)")
    if getattr(args, "fused_lovasz", False):
        if getattr(args, "fused_ohem", False):
            raise ValueError("--fused-lovasz cannot be combined with --fused-ohem: it selects CriterionOhemDSN2, the OHEM "
                             "criterion is another one")
        if getattr(args, "ohem", False):
            raise ValueError("--fused-lovasz cannot be combined with --ohem: it selects CriterionOhemDSN2, which does no OHEM "
                             "despite its name")
        if getattr(args, "fused_dsn", False):
            raise ValueError("--fused-lovasz cannot be combined with --fused-dsn: CriterionOhemDSN2 leaves the DSN head unused "
                             "and already up-samples the main head inside its kernels")


def parse_args(argv=None):
    """build_parser().parse_args with the cross-option checks reported as usage errors."""
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        ap.error(str(e))
    if args.fused_ohem:
        args.ohem = True                                      # (--fused-ohem implies --ohem)
    if args.fused_lovasz:
        args.lovasz = True                                    # (--fused-lovasz implies --lovasz)
    return args


if __name__ == "__main__":
    run(parse_args())
