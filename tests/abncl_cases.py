"""The driver and the case table of the channels_last device ABN (include/ccnet_abncl.h), shared by the SIMT-emulator tests
(tests/test_abncl_host.py) and the device tests (tests/test_gpu_abncl.py).  A plain module, test infrastructure only.

``run_abncl`` takes what ``abn_cases.run_abn`` takes -- NCHW NumPy inputs -- lays every tensor out pixel-major, (M = N H W, C)
row-major, in guarded buffers, drives the whole C ABI and returns ``run_abn``'s dict transposed back to NCHW.  The oracle, the
bars (``abn_cases.check_case``), the semantics, the parameter variations, the numeric edges and the case runners are
abn_cases' own: ``pixel_major()`` points them at this driver and at this module's shapes for the length of a call, so nothing
of them is restated here."""
import contextlib
import ctypes

import numpy as np

import abn_cases as K
import abn_oracle as O
from guarded_memory import Buf, DeviceMemory, HostMemory  # noqa: F401  (the tests reach them through here)


def run_abncl(lib, mem, x, weight, bias, rm, rv, dy, training=True, act=0, p=0.01, gamma_mode=0, eps=1e-5, momentum=0.1,
              residual=None, source=0, bf16=False, ranks=1, offsets=None, want_dweight=True, want_dbias=True,
              want_dresidual=True):
    """``abn_cases.run_abn`` on the pixel-major ABI: same arguments, same result.  A 'rank' is a slice of the batch, that is
    a block of consecutive rows."""
    from ccnet_amd._abncl_lib import make_desc
    offsets = offsets or {}
    assert set(offsets) <= set(K.TENSORS)
    N, C = x.shape[:2]
    HW = int(np.prod(x.shape[2:]))
    kind = "bf16" if bf16 else "f32"
    conv = (lambda a: O.to_bf16_bits(a)) if bf16 else (lambda a: np.ascontiguousarray(a, np.float32))
    back = (lambda a: O.from_bf16_bits(a)) if bf16 else (lambda a: a)
    bufs = []

    def buf(name, kind_, n, offset=0, data=None):
        bufs.append(Buf(mem, name, kind_, n, offset, data))
        return bufs[-1]

    def split(a, name, off):
        rows = np.ascontiguousarray(conv(a).reshape(N, C, HW).transpose(0, 2, 1))            # (N, HW, C)
        return [buf(f"{name}[{r}]", kind, q.size, off, q) for r, q in enumerate(np.array_split(rows, ranks))]

    x_off = offsets.get("y", offsets.get("x", 0)) if source == 1 else offsets.get("x", 0)
    xs = split(x, "x", x_off)
    counts = [b.n // (C * HW) for b in xs]
    assert all(counts), "a rank without a sample"
    rs = None if residual is None else split(residual, "residual", offsets.get("residual", 0))
    dys = split(dy, "dy", offsets.get("dy", 0))
    f32 = lambda name, a: None if a is None else buf(name, "f32", C, 0, np.ascontiguousarray(a, np.float32))  # noqa: E731
    w, b = f32("weight", weight), f32("bias", bias)
    rmb, rvb = f32("running_mean", rm), f32("running_var", rv)
    ptr = lambda q: None if q is None else q.ptr                                                              # noqa: E731
    descs = [make_desc(int(bf16), n * HW, C, act, p, gamma_mode, eps) for n in counts]
    nws = [lib.ccnet_abncl_workspace_bytes(ctypes.byref(d)) for d in descs]
    assert all(nws), lib.last_error()
    assert all(nws[r] == 16 * C * lib.ccnet_abncl_splits(ctypes.byref(descs[r])) for r in range(ranks))
    wss = [buf(f"workspace[{r}]", "f64", nws[r] // 8) for r in range(ranks)]
    s = mem.stream

    def table(parts, name):
        rows = [q.read(np.float64)[0] for q in parts]
        return buf(name, "f64", sum(r.size for r in rows), 0, np.concatenate(rows))

    saved = None
    if training:
        locs = [buf(f"local[{r}]", "f64", 3 * C) for r in range(ranks)]
        for r in range(ranks):
            lib.check(lib.ccnet_abncl_stats(ctypes.byref(descs[r]), xs[r].ptr, locs[r].ptr, wss[r].ptr, nws[r], s), "stats")
        saved = buf("saved", "f64", 3 * C)
        lib.check(lib.ccnet_abncl_stats_combine(ctypes.byref(descs[0]), table(locs, "all").ptr, ranks, momentum, ptr(rmb),
                                                ptr(rvb), saved.ptr, s), "combine")
    ys = xs if source == 1 else [buf(f"y[{r}]", kind, xs[r].n, offsets.get("y", 0)) for r in range(ranks)]
    for r in range(ranks):
        lib.check(lib.ccnet_abncl_forward(ctypes.byref(descs[r]), xs[r].ptr, ptr(rs and rs[r]), ys[r].ptr, ptr(saved),
                                          ptr(rmb), ptr(rvb), ptr(w), ptr(b), s), "forward")
    rback = rs if source == 1 else None           # as ccnet_amd.abncl does: out of place the backward needs y only
    sums = [buf(f"sums[{r}]", "f64", 2 * C) for r in range(ranks)]
    dws = [buf(f"dweight[{r}]", "f32", C) if want_dweight else None for r in range(ranks)]
    dbs = [buf(f"dbias[{r}]", "f32", C) if want_dbias else None for r in range(ranks)]
    for r in range(ranks):
        src = ys[r] if source == 1 else xs[r]
        lib.check(lib.ccnet_abncl_backward_reduce(ctypes.byref(descs[r]), source, src.ptr, ys[r].ptr, dys[r].ptr,
                                                  ptr(rback and rback[r]), ptr(saved), ptr(rmb), ptr(rvb), ptr(w), ptr(b),
                                                  sums[r].ptr, ptr(dws[r]), ptr(dbs[r]), wss[r].ptr, nws[r], s), "reduce")
    all_sums = table(sums, "all_sums")
    dxs = [buf(f"dx[{r}]", kind, xs[r].n, offsets.get("dx", 0)) for r in range(ranks)]
    want_dres = residual is not None and want_dresidual
    dress = [buf(f"dresidual[{r}]", kind, xs[r].n, offsets.get("dresidual", 0)) if want_dres else None
             for r in range(ranks)]
    for r in range(ranks):
        src = ys[r] if source == 1 else xs[r]
        lib.check(lib.ccnet_abncl_backward_apply(ctypes.byref(descs[r]), source, src.ptr, ys[r].ptr, dys[r].ptr,
                                                 ptr(rback and rback[r]), ptr(saved), ptr(rmb), ptr(rvb), ptr(w), ptr(b),
                                                 all_sums.ptr, ranks, dxs[r].ptr, ptr(dress[r]), s), "apply")
    got = {q.name: q.read(np.float64 if q.size == 8 else np.float32 if q.size == 4 else np.uint16) for q in bufs}
    touched = [name for name, (_, intact) in got.items() if not intact]
    assert not touched, ("guard bands written", touched)

    def cat(parts):                                # the ranks' (n HW, C) rows back to (N, C, ...)
        rows = back(np.concatenate([got[q.name][0] for q in parts])).reshape(N, HW, C)
        return np.ascontiguousarray(rows.transpose(0, 2, 1)).reshape(x.shape)

    rows = lambda parts: np.stack([got[q.name][0] for q in parts])                                            # noqa: E731
    out = {"y": cat(ys), "dx": cat(dxs), "running_mean": got["running_mean"][0], "running_var": got["running_var"][0],
           "saved": got["saved"][0].reshape(3, C) if training else None, "sums": rows(sums).sum(0).reshape(2, C),
           "dweight": rows(dws).sum(0) if want_dweight else None, "dbias": rows(dbs).sum(0) if want_dbias else None}
    if want_dres:
        out["dresidual"] = cat(dress)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the smallest shapes that reach each edge.  V = 4 (fp32) or 8 (bf16) channels per 16-byte group; a tile is at
# most 8 groups (32 or 64 channels); kMinRows = 256, kTargetBlocks = 2048, kMaxSlabs = 64 (abncl_kernels.hpp, plan() of
# abncl_api.hip)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "c5": (2, 5, 3, 7),               # C % V != 0 in both dtypes: every row ends in a short group
    "c12": (2, 12, 5, 5),             # the vector path in fp32, short groups in bf16
    "c8": (3, 8, 1, 3),               # one group per row (bf16), M = 9 smaller than the row lanes
    "tile_exact": (1, 64, 9, 11),     # one full bf16 tile, two fp32 tiles
    "tile_tail": (2, 72, 9, 11),      # one full tile plus an 8-channel tile
    "many_tiles": (1, 200, 7, 9),
    "m1_eval": (1, 16, 1, 1),         # eval semantics only
    "m2": (2, 16, 1, 1),              # the smallest training count
    "slabs": (2, 72, 37, 41),         # M = 3034: 12 slabs of 253 rows, the last of 251
    "row_blocks": (1, 8, 129, 129),   # M = 16641 > 64 * 256: the reductions stop at kMaxSlabs = 64 slabs (of 261 rows), the
                                      # elementwise passes cut 66 row blocks (of 253): the smallest M at which the two differ
    "odd": K.SHAPES["odd"],           # (abn_cases.run_nonfinite_case names it: C = 3, one short group per row)
}

_ALL = tuple(K.SEMANTICS)
# every semantic meets a short-group shape (c5) and slabs; every shape meets both modes, a residual and eval mode
GRID = {
    "c5": _ALL,
    "c12": ("oop_identity", "oop_relu_res", "oop_eval_elu", "ip_leaky01_res", "ip_eval_elu_res"),
    "c8": ("oop_leaky", "oop_eval_relu_res", "ip_elu_res", "ip_eval_leaky"),
    "tile_exact": ("oop_relu_res_nodres", "oop_eval_elu", "ip_identity", "ip_leaky01_res", "ip_eval_elu"),
    "tile_tail": ("oop_relu_res", "oop_leaky0", "oop_eval_relu_res", "ip_elu", "ip_elu_res", "ip_eval_elu_res"),
    "many_tiles": ("oop_elu", "oop_relu_res", "oop_eval_relu_res", "ip_leaky001", "ip_leaky01_res", "ip_eval_elu"),
    "m1_eval": ("oop_eval_relu_res", "oop_eval_elu", "ip_eval_leaky", "ip_eval_elu_res", "ip_eval_elu"),
    "m2": ("oop_identity", "oop_relu_res", "oop_eval_elu", "ip_leaky001", "ip_elu_res", "ip_eval_elu_res"),
    "slabs": _ALL,
    "row_blocks": ("oop_relu_res", "oop_eval_elu", "ip_leaky01_res", "ip_eval_elu_res"),
}
GRID_CASES = [(shape, sem) for shape in GRID for sem in GRID[shape]]
# Both shapes meet every variation out of place and in place.  In place they run WITHOUT a residual: 'signed0' holds a weight of
# exactly 0, where gamma = eps = 1e-5, and the fp32 rebuild xhat = (act^-1(y) - beta - residual) / gamma then rounds
# act^-1(y) - beta at the residual's size: 2^-24 |residual| / 1e-5 = 6e-3 of a standard deviation per element, which a sum
# over more than a handful of rows carries past the 1e-4 bar in any layout (dz_xhat is csrc_abn's own function; on these inputs
# libccnet_abn's emulator build shows the same 5.05e-4 in channel 1 of sum dz xhat and 1.5e-7 elsewhere; abn_cases runs that
# pair at 4 values per channel).  Without a residual act^-1(y) - beta is a difference of neighbours and exact.  The in-place
# residual is met by every shape of GRID.
PARAMETER_CASES = [(par, shape, sem) for par in K.PARAMETERS
                   for shape, sem in (("c5", "oop_leaky"), ("c5", "ip_leaky001"), ("tile_tail", "oop_relu_res"),
                                      ("tile_tail", "ip_leaky001"))]
NUMERIC_CASES = [(name, shape, bf16) for name in K.NUMERIC for shape in ("c12", "slabs")
                 for bf16 in ((False,) if K.NUMERIC[name][1] else (False, True))]
# C % V == 0 in both dtypes, so the aligned run takes the vector path and every offset run the element path
MISALIGNED_CASES = [(sem, shape) for sem in ("oop_relu_res", "ip_leaky01_res", "ip_eval_elu")
                    for shape in ("c8", "tile_tail")]
RANK_CASES = K.RANK_CASES
NONFINITE_CASES = ("oop_relu_res", "ip_leaky01_res")


def splits(lib, shape, bf16):
    """(S, rows per slab) of a case's shape"""
    from ccnet_amd._abncl_lib import make_desc
    N, C = shape[:2]
    M = N * int(np.prod(shape[2:]))
    S = lib.ccnet_abncl_splits(ctypes.byref(make_desc(int(bf16), M, C, 0, 0.0, 0, 1e-5)))
    return S, -(-M // max(S, 1))


@contextlib.contextmanager
def pixel_major():
    """abn_cases' runners on this module's driver and shapes"""
    keep = K.run_abn, K.SHAPES
    K.run_abn, K.SHAPES = run_abncl, SHAPES
    try:
        yield
    finally:
        K.run_abn, K.SHAPES = keep


def run_grid_case(lib, mem, shape, sem, bf16):
    with pixel_major():
        K.run_grid_case(lib, mem, shape, sem, bf16)


def run_parameter_case(lib, mem, par, shape, sem, bf16):
    with pixel_major():
        K.run_parameter_case(lib, mem, par, shape, sem, bf16)


def run_numeric_case(lib, mem, name, shape, bf16):
    with pixel_major():
        return K.run_numeric_case(lib, mem, name, shape, bf16)


def run_misaligned_case(lib, mem, sem, shape, bf16):
    with pixel_major():
        K.run_misaligned_case(lib, mem, sem, shape, bf16)


def run_rank_case(lib, mem, N, R, sem):
    with pixel_major():
        K.run_rank_case(lib, mem, N, R, sem)


def run_nonfinite_case(lib, mem, sem):
    with pixel_major():
        K.run_nonfinite_case(lib, mem, sem)


def run_repeat_case(lib, mem, shape, sem, bf16):
    """two runs of one case: every output the same bits"""
    kw, residual, want_dres = K._sem_kwargs(sem)
    x, w, b, rm, rv, dy, res = K.table_inputs(SHAPES[shape], K._seed("repeat", shape, sem), residual=residual)
    run = lambda: run_abncl(lib, mem, x, w, b, rm, rv, dy, residual=res, gamma_mode=kw["source"], bf16=bf16, **kw)  # noqa
    a, c = run(), run()
    for k in K.OUTPUTS:
        if a.get(k) is not None:
            assert np.array_equal(a[k], c[k], equal_nan=True), k
