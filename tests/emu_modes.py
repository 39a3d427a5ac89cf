"""The SIMT emulator's modes (tests/emu/hip_emu.hpp) for the tests that run under them.  A plain module, test
infrastructure only.  The variables are read at every launch, so a test sets them with ``monkeypatch`` around the calls it means."""
import ctypes

LATE = "CCA_EMU_LATE_DMA"           # LDS-DMAs land when a wait retires them, the latest the device may complete them
REVERSE = "CCA_EMU_REVERSE"         # the scheduler visits wavefronts, and lanes within them, in descending order
KEEP_PLUS = "CCA_EMU_KEEP_PLUS"     # every counted barrier keeps one instruction more in flight than it asks for
ALL = (LATE, REVERSE, KEEP_PLUS)


def set_mode(monkeypatch, *on):
    """exactly the variables of ``on`` set; the rest unset"""
    for name in ALL:
        if name in on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def vmem_stats(dll, reset=False):
    """the vector-memory model's counters of the emulator library ``dll`` (a ctypes handle):
    {"dma_issued": n, "retired_by_counted_barriers": n, "sites": {"file.hpp:line": (runs, runs with an un-landed DMA, largest keep,
    largest keep with an un-landed DMA)}}"""
    dll.emu_vmem_stats.restype = ctypes.c_size_t
    dll.emu_vmem_stats.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    n = dll.emu_vmem_stats(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    dll.emu_vmem_stats(buf, n + 1)
    out = {"sites": {}}
    for line in buf.value.decode().splitlines():
        f = line.split()
        if f[0] == "site":
            out["sites"][f[1]] = tuple(int(v) for v in f[2:6])
        else:
            out[f[0]] = int(f[1])
    if reset:
        dll.emu_vmem_reset_stats()
    return out
