"""The training input pipeline on the device: the reference's ``dataset/datasets.py`` (CSDataSet, VOCDataSet) with its random
scale, mean subtraction, pad, crop, mirror and label remap done by one HIP kernel (include/ccnet_augment.h,
libccnet_augment.so) instead of a CPU worker.

The reference resizes the whole frame by 0.7 ... 2.1 on the host, converts it to float32, pads it and only then cuts the
769 x 769 crop.  Here a dataset's ``__getitem__`` only decodes the files and draws the random parameters -- in the reference's
order and from the same generators, so a seeded run picks the same scale, offsets and mirror -- and :class:`DeviceAugment`
gathers every output pixel straight from the packed ``uint8`` frames: four source pixels and one label each, nothing of
scaled-frame size anywhere.  The arithmetic is an exact integer definition (the header states it; DESIGN.md §21 says which of
``cv2``'s properties it takes from ``cv2``'s documentation and source).  There is no CPU fallback.

    ds = CSDataSet(root, list_path, crop_size=(769, 769), mean=IMG_MEAN)
    loader = DataLoader(ds, batch_size=8, collate_fn=collate, num_workers=8, pin_memory=True)
    for images, labels, batch in DevicePrefetcher(loader, ds.device_augment(), device):
        loss = model(images, labels)

Worker processes never touch the device: :func:`collate` packs into ordinary host memory there, and the batch is pinned in the
consumer process -- by the DataLoader's pin thread (``pin_memory=True``, as above) or, failing that, by the prefetcher itself.
"""
from __future__ import annotations

import os.path as osp
import random
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import _augment_lib as A

# dataset/datasets.py:146-151 for uint8 labels: the listed ids map to their train ids, every other value stays as it is
_CITYSCAPES_TRAIN_IDS = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13,
                         27: 14, 28: 15, 31: 16, 32: 17, 33: 18}


def cityscapes_table(ignore_label: int = 255) -> np.ndarray:
    """The 256-entry uint8 table of ``CSDataSet.id2trainId``: ids 0 ... 33 to train ids or ``ignore_label``, the rest unchanged."""
    table = np.arange(256, dtype=np.uint8)
    for k in range(34):
        table[k] = _CITYSCAPES_TRAIN_IDS.get(k, ignore_label)
    return table


CITYSCAPES_ID_TO_TRAINID = cityscapes_table(255)
CITYSCAPES_SCALES = (7, 14, 10)          # f_scale = 0.7 + randint(0, 14) / 10   (datasets.py:158)
VOC_SCALES = (5, 11, 10)                 # f_scale = 0.5 + randint(0, 11) / 10   (datasets.py:40)


def _round_half_even_div(p: int, q: int) -> int:
    d, r2 = p // q, 2 * (p % q)
    return d + (1 if r2 > q or (r2 == q and d & 1) else 0)


def scaled_size(h: int, w: int, num: int, den: int):
    """(Hz, Wz) of an h x w frame resized by num/den: ``max(1, round_half_even(n * num / den))`` per axis, in integers."""
    return max(1, _round_half_even_div(h * num, den)), max(1, _round_half_even_div(w * num, den))


class AugmentParams(NamedTuple):
    """One sample's random choices: the scale num/den, the scaled size it gives, the crop offsets and the mirror flag."""
    num: int
    den: int
    hz: int
    wz: int
    h_off: int
    w_off: int
    mirror: bool


def draw_params(height: int, width: int, crop_size, scale: bool = True, mirror: bool = True, scales=CITYSCAPES_SCALES,
                rng=random, np_rng=np.random) -> AugmentParams:
    """The reference's random choices for one height x width frame, in its order and from its generators (``random`` and
    ``numpy.random`` unless others are given): ``randint(0, steps)`` for the scale ``(first + k) / den`` when ``scale``
    (datasets.py:157-161; ``scales`` is (first, steps, den): CITYSCAPES_SCALES or VOC_SCALES), ``randint`` for the row and then
    the column offset on the padded scaled size (197-199), ``choice(2)`` for the mirror when ``mirror`` (205-208: the reference
    flips when the draw is 0)."""
    crop_h, crop_w = crop_size
    num, den = 1, 1
    if scale:
        first, steps, den = scales
        num = first + rng.randint(0, steps)
    hz, wz = scaled_size(height, width, num, den)
    h_off = rng.randint(0, max(hz, crop_h) - crop_h)
    w_off = rng.randint(0, max(wz, crop_w) - crop_w)
    flip = bool(mirror) and int(np_rng.choice(2)) == 0
    return AugmentParams(num, den, hz, wz, h_off, w_off, flip)


def descriptors(sizes, params: Sequence[AugmentParams], pin: bool = False):
    """The CPU int32 (B, 16) descriptor table (include/ccnet_augment.h) of frames of the given (H, W) ``sizes`` packed end to
    end without padding, with each sample's drawn parameters."""
    desc = torch.zeros(len(sizes), A.DESC_INTS, dtype=torch.int32, pin_memory=pin)
    rows, at = desc.numpy(), 0
    for b, ((h, w), p) in enumerate(zip(sizes, params)):
        rows[b, :A.MIRROR + 1] = [3 * at, at, h, w, w, p.num, p.den, p.hz, p.wz, p.h_off, p.w_off, int(p.mirror)]
        at += h * w
    return desc


def pack(frames: Sequence[np.ndarray], labels: Sequence[np.ndarray], params: Sequence[AugmentParams], pin: bool = False):
    """Pack uint8 (H, W, 3) frames and (H, W) labels of any sizes end to end, without padding, and write the descriptor table:
    returns (frames uint8[sum 3HW], labels uint8[sum HW], desc int32 (B, 16)) as CPU tensors, pinned when ``pin``."""
    B = len(frames)
    assert B == len(labels) == len(params) and B > 0
    pixels = 0
    for f, l in zip(frames, labels):
        if f.dtype != np.uint8 or l.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or l.shape != f.shape[:2]:
            raise ValueError(f"pack: expected uint8 (H, W, 3) frames and uint8 (H, W) labels, got {f.dtype} {f.shape} and "
                             f"{l.dtype} {l.shape}")
        pixels += f.shape[0] * f.shape[1]
    if 3 * pixels > 0x7fffffff:
        raise ValueError(f"pack: {3 * pixels} bytes of frames in one batch; the descriptor's offsets are int32")
    fbuf = torch.empty(3 * pixels, dtype=torch.uint8, pin_memory=pin)
    lbuf = torch.empty(pixels, dtype=torch.uint8, pin_memory=pin)
    fnp, lnp, at = fbuf.numpy(), lbuf.numpy(), 0
    for f, l in zip(frames, labels):
        n = l.size
        fnp[3 * at:3 * (at + n)] = f.reshape(-1)
        lnp[at:at + n] = l.reshape(-1)
        at += n
    return fbuf, lbuf, descriptors([l.shape for l in labels], params, pin=pin)


class DeviceAugment:
    """The reference's scale + mean + pad + crop + mirror (+ label table) for a packed batch, on the device.

    ``crop_size`` is (crop_h, crop_w); ``mean`` the three values the reference subtracts from its B, G, R planes, in that
    order; ``label_table`` an optional 256-entry uint8 table (``CITYSCAPES_ID_TO_TRAINID``; None: labels pass unchanged, the
    VOC case); ``source_order`` says whether the frames' bytes are "rgb" (PIL) or "bgr" (``cv2.imread``): the output is always
    the reference's, B, G, R.  Calling it with (frames, labels, desc) -- the packed uint8 device tensors and the CPU int32
    descriptor table of :func:`pack` -- returns (images float32 (B, 3, crop_h, crop_w), labels int64 (B, crop_h, crop_w)) on
    the frames' device.  The one launch goes on the current stream and nothing is read back; ``desc_device`` (the same table
    already on the device) makes the call free of copies, e.g. for graph capture."""

    def __init__(self, crop_size, mean, ignore_label: int = 255, label_table=None, source_order: str = "rgb"):
        if source_order not in ("rgb", "bgr"):
            raise ValueError(f"DeviceAugment: source_order is 'rgb' or 'bgr', got {source_order!r}")
        self.crop_h, self.crop_w = (int(v) for v in crop_size)
        self.mean = tuple(float(v) for v in mean)
        if len(self.mean) != 3:
            raise ValueError(f"DeviceAugment: three means expected, got {mean!r}")
        self.ignore_label = int(ignore_label)
        self.source_order = source_order
        self.label_table = None
        if label_table is not None:
            table = np.ascontiguousarray(label_table)
            if table.shape != (256,) or table.min() < 0 or table.max() > 255:
                raise ValueError("DeviceAugment: label_table holds 256 values in 0 ... 255")
            self.label_table = torch.from_numpy(table.astype(np.uint8))
        self._tables = {}                # device -> the table there

    def _table_on(self, device):
        """The label table on ``device``.  The first call per device uploads it on that device's default stream and waits for
        it, so every later launch, on whichever stream, finds it complete (make that first call outside a graph capture)."""
        if self.label_table is None:
            return None
        if device not in self._tables:
            default = torch.cuda.default_stream(device)
            with torch.cuda.stream(default):
                self._tables[device] = self.label_table.to(device)
            default.synchronize()
        return self._tables[device]

    def __call__(self, frames, labels, desc, desc_device=None):
        if not (frames.is_cuda and labels.is_cuda and labels.device == frames.device):
            raise RuntimeError("DeviceAugment: frames and labels must be HIP device tensors on one device (ccnet_amd has no CPU "
                               "fallback for the input-pipeline kernel)")
        if frames.dtype != torch.uint8 or labels.dtype != torch.uint8 or not (frames.is_contiguous() and labels.is_contiguous()):
            raise RuntimeError(f"DeviceAugment: packed contiguous uint8 frames and labels expected, got {frames.dtype} and "
                               f"{labels.dtype}")
        if desc.is_cuda or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != A.DESC_INTS or not desc.is_contiguous():
            raise RuntimeError(f"DeviceAugment: desc is the CPU int32 (B, {A.DESC_INTS}) table of pack(), got {desc.dtype} "
                               f"{tuple(desc.shape)} on {desc.device}")
        dev = frames.device
        lib = A.get_lib()
        B = desc.shape[0]
        if desc_device is None:
            desc_device = desc.to(dev, non_blocking=True)
        elif desc_device.device != dev or desc_device.dtype != torch.int32 or tuple(desc_device.shape) != tuple(desc.shape) \
                or not desc_device.is_contiguous():
            raise RuntimeError("DeviceAugment: desc_device is desc on the frames' device")
        table = self._table_on(dev)
        with torch.cuda.device(dev):
            images = torch.empty(B, 3, self.crop_h, self.crop_w, dtype=torch.float32, device=dev)
            out = torch.empty(B, self.crop_h, self.crop_w, dtype=torch.int64, device=dev)
            lib.check(lib.ccnet_augment_crop_u8(frames.data_ptr(), frames.numel(), labels.data_ptr(), labels.numel(),
                                                desc.data_ptr(), desc_device.data_ptr(),
                                                None if table is None else table.data_ptr(), images.data_ptr(), out.data_ptr(),
                                                B, self.crop_h, self.crop_w, *self.mean, self.ignore_label,
                                                int(self.source_order == "rgb"), torch.cuda.current_stream(dev).cuda_stream),
                      "ccnet_augment_crop_u8")
        return images, out


def _decode(img_file, label_file):
    """(uint8 (H, W, 3) RGB frame, uint8 (H, W) label) with PIL.  PNG decoding is lossless, so the frame's pixels are
    ``cv2.imread``'s up to the channel order; a label that is not 8-bit grey is converted as IMREAD_GRAYSCALE would."""
    from PIL import Image
    with Image.open(img_file) as im:
        frame = np.asarray(im.convert("RGB"), dtype=np.uint8)
    with Image.open(label_file) as im:
        label = np.asarray(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)
    return np.ascontiguousarray(frame), np.ascontiguousarray(label)


class _AugmentedDataSet(torch.utils.data.Dataset):
    """What the two datasets share.  ``__getitem__`` decodes and draws; it returns (frame uint8 (H, W, 3) in R, G, B, label
    uint8 (H, W) of raw ids, AugmentParams, size, name), ``size`` and ``name`` as the reference's."""

    SCALES = None                        # (first, steps, den) of the subclass's random scale

    def __init__(self, root, list_path, max_iters=None, crop_size=(321, 321), mean=(128, 128, 128), scale=True, mirror=True,
                 ignore_label=255):
        self.root, self.list_path = root, list_path
        self.crop_h, self.crop_w = crop_size
        self.scale, self.ignore_label, self.mean, self.is_mirror = scale, ignore_label, mean, mirror
        with open(list_path) as f:
            self.img_ids = [self._parse(line.strip()) for line in f if line.strip()]
        if max_iters is not None:
            self.img_ids = self.img_ids * int(np.ceil(float(max_iters) / len(self.img_ids)))
        self.files = [self._files(item) for item in self.img_ids]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        datafiles = self.files[index]
        frame, label = _decode(datafiles["img"], datafiles["label"])
        params = draw_params(label.shape[0], label.shape[1], (self.crop_h, self.crop_w), self.scale, self.is_mirror, self.SCALES)
        return frame, label, params, np.array(frame.shape), datafiles["name"]

    def label_table(self):
        return None

    def device_augment(self) -> DeviceAugment:
        """The DeviceAugment that finishes this dataset's samples (its crop, mean, ignore label and label table; RGB source)."""
        return DeviceAugment((self.crop_h, self.crop_w), self.mean, self.ignore_label, self.label_table(), "rgb")


class CSDataSet(_AugmentedDataSet):
    """The reference's ``CSDataSet`` (datasets.py:121-210), same constructor: lines of "<image path> <label path>" under
    ``root``; scales 0.7 ... 2.1; label ids remapped to train ids by the kernel's table."""

    SCALES = CITYSCAPES_SCALES

    @staticmethod
    def _parse(line):
        return line.split()

    def _files(self, item):
        image_path, label_path = item
        return {"img": osp.join(self.root, image_path), "label": osp.join(self.root, label_path),
                "name": osp.splitext(osp.basename(label_path))[0]}

    def label_table(self):
        return cityscapes_table(self.ignore_label)


class VOCDataSet(_AugmentedDataSet):
    """The reference's ``VOCDataSet`` (datasets.py:12-81), same constructor: one name per line, JPEGImages/<name>.jpg and
    SegmentationClassAug/<name>.png under ``root``; scales 0.5 ... 1.6; labels unchanged.  (JPEG decoders may differ in the
    last bit between PIL's and cv2's builds; PNG frames decode identically.)"""

    SCALES = VOC_SCALES

    @staticmethod
    def _parse(line):
        return line

    def _files(self, name):
        return {"img": osp.join(self.root, "JPEGImages/%s.jpg" % name),
                "label": osp.join(self.root, "SegmentationClassAug/%s.png" % name), "name": name}


def collate(samples, pin: bool = False):
    """``collate_fn`` for a DataLoader over the datasets above: packs the samples' frames and labels into uint8 buffers plus
    the descriptor table.  Returns a dict: frames, labels, desc, params, size, name.  It never calls the device API unless
    ``pin`` is given, and never inside a DataLoader worker (a forked worker must not open the device, and what it pinned
    would reach the consumer as shared memory anyway): there ``pin`` is ignored.  Pin in the consumer process instead --
    ``DataLoader(pin_memory=True)`` does, and :class:`DevicePrefetcher` pins what arrives unpinned."""
    frames, labels, params, sizes, names = zip(*samples)
    pin = bool(pin) and torch.utils.data.get_worker_info() is None
    fbuf, lbuf, desc = pack(frames, labels, params, pin=pin)
    return {"frames": fbuf, "labels": lbuf, "desc": desc, "params": list(params), "size": np.stack(sizes), "name": list(names)}


def _pinned(tensor):
    """``tensor`` in page-locked host memory: itself if it is there already, else a pinned copy (made in the calling process)"""
    return tensor if tensor.is_pinned() else tensor.pin_memory()


class DevicePrefetcher:
    """Iterates a DataLoader (or any iterable) of :func:`collate` batches as (images, labels, batch): batch i + 1 is copied with
    ``non_blocking=True`` and run through ``augment`` on a side stream while the consumer trains on batch i; the consumer's
    current stream waits on an event before it is handed a batch.  The copies are asynchronous only from page-locked memory:
    a batch that arrives unpinned (a DataLoader without ``pin_memory=True`` hands over shared memory) is pinned here, in the
    consumer process, at the price of one more host copy."""

    def __init__(self, loader, augment: DeviceAugment, device):
        self.loader, self.augment, self.device = loader, augment, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DevicePrefetcher: a HIP device is needed (ccnet_amd has no CPU fallback for the input-pipeline kernel)")
        self.stream = torch.cuda.Stream(self.device)

    def __len__(self):
        return len(self.loader)

    def _start(self, batch):
        if batch is None:
            return None
        with torch.cuda.stream(self.stream):
            frames = _pinned(batch["frames"]).to(self.device, non_blocking=True)
            labels = _pinned(batch["labels"]).to(self.device, non_blocking=True)
            images, out = self.augment(frames, labels, _pinned(batch["desc"]))
            ready = torch.cuda.Event()
            ready.record(self.stream)
        return images, out, batch, ready

    def __iter__(self):
        it = iter(self.loader)
        pending = self._start(next(it, None))
        while pending is not None:
            images, out, batch, ready = pending
            consumer = torch.cuda.current_stream(self.device)
            consumer.wait_event(ready)
            images.record_stream(consumer)
            out.record_stream(consumer)
            pending = self._start(next(it, None))
            yield images, out, batch
