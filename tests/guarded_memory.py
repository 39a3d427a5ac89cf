"""Guarded buffers for tests that drive a C ABI directly: ``Buf`` puts a tensor between two guard bands of a fixed bit
pattern inside one allocation of a back end -- ``HostMemory`` (numpy, for the SIMT emulator builds) or ``DeviceMemory`` (torch
byte tensors on the current device and stream).  Shared by tests/abn_cases.py and tests/cca_cases.py.  Test infrastructure only."""
import numpy as np

GUARD = 64                                   # guard elements on each side of every buffer
_KINDS = {"f32": (4, np.uint32, 0xCDCDCDCD), "bf16": (2, np.uint16, 0xCDCD),
          "f64": (8, np.uint64, 0x7FF8000000000000),        # fp64 bands hold NaN
          "u8": (1, np.uint8, 0xCD), "i64": (8, np.uint64, 0xCDCDCDCDCDCDCDCD)}


class HostMemory:
    """numpy arrays standing in for device memory (the emulator's back end)"""
    name = "emu"
    stream = None

    def new(self, nbytes):
        raw = np.empty(nbytes, np.uint8)
        return raw, raw.ctypes.data

    def upload(self, raw, at, data):
        raw[at:at + data.size] = data

    def download(self, raw):
        return raw


class DeviceMemory:
    """torch byte tensors on the current device; copies and launches go on the current stream"""
    name = "gpu"

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device())

    @property
    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def new(self, nbytes):
        raw = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
        return raw, raw.data_ptr()

    def upload(self, raw, at, data):
        raw[at:at + data.size].copy_(self.torch.from_numpy(np.ascontiguousarray(data)))

    def download(self, raw):
        return raw.cpu().numpy()


class Buf:
    """``n`` elements of ``kind`` starting ``offset`` elements past an ``align``-byte boundary (16 by default), ``guard``
    elements of a fixed bit pattern on each side (GUARD by default; ``pattern`` replaces the kind's own).  The offset is a
    whole number of elements and the data lie inside the allocation."""

    def __init__(self, mem, name, kind, n, offset=0, data=None, guard=GUARD, align=16, pattern=None):
        size, self.utype, pat = _KINDS[kind]
        pat = pat if pattern is None else pattern
        assert 0 <= offset * size < 16 and align % 16 == 0 and guard >= 0
        self.mem, self.name, self.n, self.size, self.kind = mem, name, n, size, kind
        total = 2 * guard * size + 2 * align + n * size
        self.raw, base = mem.new(total)
        self.start = guard * size + (-(base + guard * size)) % align + offset * size
        assert self.start + n * size + guard * size <= total and (base + self.start) % size == 0
        assert (base + self.start) % align == offset * size
        self.ptr = base + self.start
        # the pattern is laid from the data's first byte, so it is element-aligned on both sides
        self.image = np.array([pat], self.utype).view(np.uint8)[(np.arange(total) - self.start) % size]
        if data is not None:
            self.image[self.start:self.start + n * size] = np.ascontiguousarray(data).view(np.uint8).ravel()
        mem.upload(self.raw, 0, self.image)

    def read(self, dtype):
        """the data, and whether both guard bands still hold their pattern"""
        got = np.asarray(self.mem.download(self.raw))
        a, b = self.start, self.start + self.n * self.size
        intact = np.array_equal(got[:a], self.image[:a]) and np.array_equal(got[b:], self.image[b:])
        return got[a:b].copy().view(dtype), intact
