"""One driver and one case table for the device ABN (include/ccnet_abn.h), shared by the SIMT-emulator tests
(tests/test_abn_host.py) and the device tests (tests/test_gpu_abn_edges.py).  A plain module, test infrastructure only.

``run_abn`` drives the whole C ABI -- stats, combine, forward, reduce, apply, optionally split into uneven 'ranks' -- through
a library (the emulator build or the gfx950 one) over a buffer back end (host memory, or device memory on the current
stream).  Every buffer a kernel writes sits between two guard bands that are checked after the run, and every tensor can be
placed at a chosen element offset from a 16-byte boundary (the kernels' element path).  ``check_case`` holds a run to the
header's tolerance bar against the float64 oracles of tests/abn_oracle.py."""
import ctypes

import numpy as np

import abn_oracle as O
from guarded_memory import GUARD, Buf, DeviceMemory, HostMemory  # noqa: F401  (the tests reach them through here)

TENSORS = ("x", "residual", "dy", "y", "dx", "dresidual")
OFFSETS = {False: (1, 2, 3), True: (1, 3, 4)}        # elements past a 16-byte boundary: fp32 4/8/12 bytes, bf16 2/6/8 bytes


def run_abn(lib, mem, x, weight, bias, rm, rv, dy, training=True, act=0, p=0.01, gamma_mode=0, eps=1e-5, momentum=0.1,
            residual=None, source=0, bf16=False, ranks=1, offsets=None, want_dweight=True, want_dbias=True,
            want_dresidual=True):
    """forward + backward through the C ABI of ``lib`` on buffers of ``mem``.  ``source`` 1 rebuilds xhat from y, which is
    written over x (in place).  ``ranks`` > 1 splits the batch as np.array_split does (unevenly when N does not divide) into
    that many 'ranks' whose statistics and sums are exchanged as the Python layer does.  ``offsets`` maps a tensor's name
    (TENSORS; in place the shared x / y buffer takes 'y') to its element offset from a 16-byte boundary.  Returns y, dx,
    dresidual, dweight, dbias, the running statistics, saved and the summed sums, after asserting every guard band intact."""
    from ccnet_amd._abn_lib import make_desc
    offsets = offsets or {}
    assert set(offsets) <= set(TENSORS)
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
        parts = np.array_split(conv(a).reshape(N, C, HW), ranks)
        return [buf(f"{name}[{r}]", kind, q.size, off, q) for r, q in enumerate(parts)]

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
    descs = [make_desc(int(bf16), n, C, HW, 1, act, p, gamma_mode, eps) for n in counts]
    nws = [lib.ccnet_abn_workspace_bytes(ctypes.byref(d)) for d in descs]
    assert all(nws), lib.last_error()
    wss = [buf(f"workspace[{r}]", "f64", nws[r] // 8) for r in range(ranks)]
    s = mem.stream

    def table(parts, name):
        """the ranks' fp64 rows gathered in rank order, as the Python layer's exchange does"""
        rows = [q.read(np.float64)[0] for q in parts]
        return buf(name, "f64", sum(r.size for r in rows), 0, np.concatenate(rows))

    saved = None
    if training:
        locs = [buf(f"local[{r}]", "f64", 3 * C) for r in range(ranks)]
        for r in range(ranks):
            lib.check(lib.ccnet_abn_stats(ctypes.byref(descs[r]), xs[r].ptr, locs[r].ptr, wss[r].ptr, nws[r], s), "stats")
        saved = buf("saved", "f64", 3 * C)
        lib.check(lib.ccnet_abn_stats_combine(ctypes.byref(descs[0]), table(locs, "all").ptr, ranks, momentum, ptr(rmb),
                                              ptr(rvb), saved.ptr, s), "combine")
    ys = xs if source == 1 else [buf(f"y[{r}]", kind, xs[r].n, offsets.get("y", 0)) for r in range(ranks)]
    for r in range(ranks):
        lib.check(lib.ccnet_abn_forward(ctypes.byref(descs[r]), xs[r].ptr, ptr(rs and rs[r]), ys[r].ptr, ptr(saved),
                                        ptr(rmb), ptr(rvb), ptr(w), ptr(b), s), "forward")
    # as ccnet_amd.abn does: out of place the backward is not given the residual (dz needs y only)
    rback = rs if source == 1 else None
    sums = [buf(f"sums[{r}]", "f64", 2 * C) for r in range(ranks)]
    dws = [buf(f"dweight[{r}]", "f32", C) if want_dweight else None for r in range(ranks)]
    dbs = [buf(f"dbias[{r}]", "f32", C) if want_dbias else None for r in range(ranks)]
    for r in range(ranks):
        src = ys[r] if source == 1 else xs[r]
        lib.check(lib.ccnet_abn_backward_reduce(ctypes.byref(descs[r]), source, src.ptr, ys[r].ptr, dys[r].ptr,
                                                ptr(rback and rback[r]), ptr(saved), ptr(rmb), ptr(rvb), ptr(w), ptr(b),
                                                sums[r].ptr, ptr(dws[r]), ptr(dbs[r]), wss[r].ptr, nws[r], s), "reduce")
    all_sums = table(sums, "all_sums")
    dxs = [buf(f"dx[{r}]", kind, xs[r].n, offsets.get("dx", 0)) for r in range(ranks)]
    want_dres = residual is not None and want_dresidual
    dress = [buf(f"dresidual[{r}]", kind, xs[r].n, offsets.get("dresidual", 0)) if want_dres else None
             for r in range(ranks)]
    for r in range(ranks):
        src = ys[r] if source == 1 else xs[r]
        lib.check(lib.ccnet_abn_backward_apply(ctypes.byref(descs[r]), source, src.ptr, ys[r].ptr, dys[r].ptr,
                                               ptr(rback and rback[r]), ptr(saved), ptr(rmb), ptr(rvb), ptr(w), ptr(b),
                                               all_sums.ptr, ranks, dxs[r].ptr, ptr(dress[r]), s), "apply")
    got = {q.name: q.read(np.float64 if q.size == 8 else np.float32 if q.size == 4 else np.uint16) for q in bufs}
    touched = [name for name, (_, intact) in got.items() if not intact]
    assert not touched, ("guard bands written", touched)
    cat = lambda parts: back(np.concatenate([got[q.name][0] for q in parts])).reshape(x.shape)                # noqa: E731
    rows = lambda parts: np.stack([got[q.name][0] for q in parts])                                            # noqa: E731
    out = {"y": cat(ys), "dx": cat(dxs), "running_mean": got["running_mean"][0], "running_var": got["running_var"][0],
           "saved": got["saved"][0].reshape(3, C) if training else None, "sums": rows(sums).sum(0).reshape(2, C),
           "dweight": rows(dws).sum(0) if want_dweight else None, "dbias": rows(dbs).sum(0) if want_dbias else None}
    if want_dres:
        out["dresidual"] = cat(dress)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparing with the oracles
# ---------------------------------------------------------------------------------------------------------------------
MEASURED = {}            # (back end, family, dtype, oracle, quantity) -> (largest error seen, its bar): for reports only


def close(a, b, tol, name, scale=None, record=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), scale or 0.0, 1e-30)
    err = np.abs(a - b).max() / scale
    if record is not None:
        key = record + (name,)
        MEASURED[key] = (max(err, MEASURED.get(key, (0.0, tol))[0]), tol)
    assert err <= tol, (name, err, tol)


def make_inputs(shape, seed, mean=0.0, scale=1.0, residual=False, dy_signal=0.0):
    rng = np.random.default_rng(seed)
    C = shape[1]
    xn = rng.standard_normal(shape)
    x = (xn * scale + mean).astype(np.float32)
    w = rng.uniform(-1.5, 1.5, C).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    rm = rng.uniform(-0.2, 0.2, C).astype(np.float32)
    rv = rng.uniform(0.5, 2.0, C).astype(np.float32)
    dy = (rng.standard_normal(shape) + dy_signal * (1.0 + xn)).astype(np.float32)
    res = rng.standard_normal(shape).astype(np.float32) if residual else None
    return x, w, b, rm, rv, dy, res


def dx_scale(f, g, w, gamma_mode, eps=1e-5):
    """the scale dx is measured against: that of gamma invstd dz (dx itself nearly cancels at two values per channel)"""
    k = O.gamma_of(w, len(f["invstd"]), gamma_mode, eps) * f["invstd"]
    dz = g["dresidual"].reshape(g["dresidual"].shape[0], len(k), -1)
    return float(np.abs(dz * k[None, :, None]).max())


def bf16_round(a):
    return None if a is None else O.from_bf16_bits(O.to_bf16_bits(a))


def check_case(r, x, w, b, rm, rv, dy, res, training=True, act=0, p=0.01, source=0, eps=1e-5, momentum=0.1, bf16=False,
               record=None, tol=None, tol_y=None, sum_floor=False):
    """The header's bar.  Against the exact oracle, on the same (for bf16: the same bf16-rounded) inputs: y and the running
    statistics within 1e-5 of scale (bf16 y 2^-7); out of place dx, dweight, dbias and dresidual within 1e-4 (2^-6 for bf16
    tensors).  In place (``source`` 1) the gradients are held to the same bar against the from-output oracle instead: the
    float64 rebuild from the y this run stored, with the exact oracle's mean and invstd; dweight, dbias and the sums, fp64
    sums over the same stored values, within 1e-4 in both dtypes.  ``tol`` / ``tol_y`` replace the fp32 bars where a case's
    inputs cost precision that is not the kernels' (the large mean).  ``sum_floor``: sum dz xhat and dweight are measured
    against no less than sum |dz|, their size at |xhat| = 1 -- for a tensor whose every channel is constant, where the exact
    values are 0 and have no scale of their own."""
    if bf16:
        x, dy, res = bf16_round(x), bf16_round(dy), bf16_round(res)
    rec = lambda oracle: None if record is None else record + ("bf16" if bf16 else "f32", oracle)           # noqa: E731
    p = float(np.float32(p))                  # the descriptor's act_param is a float: 0.01f is the library's slope
    f = O.forward(x, w, b, rm, rv, training, momentum=momentum, eps=eps, act=act, p=p, gamma_mode=source, residual=res)
    ty, tg = (2 ** -7, 2 ** -6) if bf16 else (tol_y or 1e-5, tol or 1e-4)
    close(r["y"], f["y"], ty, "y", record=rec("exact"))
    close(r["running_mean"], f["running_mean"], 1e-5, "running_mean", record=rec("exact"))
    close(r["running_var"], f["running_var"], 1e-5, "running_var", record=rec("exact"))
    if source == 0:
        g, name, ts = O.backward(f, dy, w, training, eps=eps, act=act, p=p, gamma_mode=0), "exact", tg
    else:
        g = O.backward_from_output(r["y"], dy, res, w, b, f["mean"], f["invstd"], f["n"], training, act=act, p=p, eps=eps)
        name, ts = "from_output", tol or 1e-4
    if r.get("dx") is not None:               # a front-end run may not have asked for it, and has no sums to show
        close(r["dx"], g["dx"], tg, "dx", scale=dx_scale(f, g, w, source, eps), record=rec(name))
    floor = float(np.abs(g["dresidual"]).reshape(len(dy), len(f["mean"]), -1).sum(axis=(0, 2)).max()) if sum_floor else None
    if r.get("sums") is not None:
        close(r["sums"], np.stack([g["sum_dz"], g["sum_dzx"]]), ts, "sums", scale=floor, record=rec(name))
    if r["dweight"] is not None:
        close(r["dweight"], g["dweight"], ts, "dweight", scale=floor, record=rec(name))
    if r["dbias"] is not None:
        close(r["dbias"], g["dbias"], ts, "dbias", record=rec(name))
    if r.get("dresidual") is not None:
        close(r["dresidual"], g["dresidual"], tg, "dresidual", record=rec(name))
    return f, g


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the smallest shapes that reach each edge (kBlockElems = 4096, kMinSplit = 8192 in plan() of abn_api.hip)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "hw1": (4, 300, 1, 1),            # every 16-byte group cut by a plane; C > 256, not a multiple: 2 channel blocks, tail
    "hw3": (3, 5, 1, 3),              # planes smaller than a group, several planes inside one group
    "odd": (2, 3, 9, 11),             # odd H * W: bf16 planes start 2 bytes off a 4-byte word
    "block_exact": (2, 2, 64, 64),    # H * W = 4096: one elementwise chunk, no tail
    "block_tail": (1, 2, 64, 65),     # H * W = 4160: a second chunk of 64 elements
    "many_planes": (9, 2, 31, 33),    # M = 9207: S = 2, chunk 4604, a reduction slice spans 4.5 planes of 1023
    "cut_plane": (3, 1, 97, 97),      # S = 4, chunk 7057 < H * W: slices begin and end mid-plane; C = 1
}

# activation, slope / alpha, source (= gamma convention: 1 in place), residual, training, dresidual requested
SEMANTICS = {
    "oop_identity": (O.IDENTITY, 0.0, 0, False, True, True),
    "oop_relu_res": (O.RELU, 0.0, 0, True, True, True),
    "oop_relu_res_nodres": (O.RELU, 0.0, 0, True, True, False),
    "oop_leaky": (O.LEAKY_RELU, 0.01, 0, False, True, True),
    "oop_leaky0": (O.LEAKY_RELU, 0.0, 0, False, True, True),
    "oop_elu": (O.ELU, 1.0, 0, False, True, True),
    "oop_eval_relu_res": (O.RELU, 0.0, 0, True, False, True),
    "oop_eval_elu": (O.ELU, 1.0, 0, False, False, True),
    "ip_identity": (O.IDENTITY, 0.0, 1, False, True, True),
    "ip_leaky001": (O.LEAKY_RELU, 0.01, 1, False, True, True),
    "ip_leaky01_res": (O.LEAKY_RELU, 0.1, 1, True, True, True),
    "ip_elu": (O.ELU, 1.0, 1, False, True, True),
    "ip_elu_res": (O.ELU, 1.0, 1, True, True, True),
    "ip_eval_leaky": (O.LEAKY_RELU, 0.01, 1, False, False, True),
    "ip_eval_elu_res": (O.ELU, 1.0, 1, True, False, True),
    "ip_eval_elu": (O.ELU, 1.0, 1, False, False, True),
}

# shapes x semantics without the full product: every semantic meets a shape with cut groups (hw1 / hw3 / odd) and one whose
# reduction slices cut planes (many_planes / cut_plane); every shape meets both modes, a residual and eval mode
GRID = {
    "hw1": ("oop_relu_res", "oop_elu", "oop_eval_relu_res", "ip_identity", "ip_leaky01_res", "ip_elu"),
    "hw3": ("oop_identity", "oop_leaky0", "oop_relu_res_nodres", "ip_leaky001", "ip_elu_res", "ip_eval_leaky"),
    "odd": ("oop_relu_res", "oop_leaky", "oop_eval_elu", "ip_identity", "ip_leaky01_res", "ip_elu", "ip_eval_elu_res"),
    "block_exact": ("oop_identity", "oop_elu", "ip_leaky001", "ip_elu_res", "ip_eval_elu_res"),
    "block_tail": ("oop_relu_res", "oop_leaky0", "oop_leaky", "oop_eval_elu", "ip_leaky01_res", "ip_eval_leaky"),
    "many_planes": ("oop_relu_res_nodres", "oop_elu", "oop_leaky", "oop_eval_relu_res", "ip_elu", "ip_leaky001",
                    "ip_eval_leaky"),
    "cut_plane": ("oop_relu_res", "oop_identity", "oop_leaky0", "oop_eval_elu", "ip_identity", "ip_leaky01_res",
                  "ip_elu_res", "ip_eval_elu_res"),
}
GRID_CASES = [(shape, sem) for shape in GRID for sem in GRID[shape]]

# parameter variations: weight / bias ('signed0': negative values and one exact 0), which gradients are requested,
# momentum and eps; each out of place and in place
PARAMETERS = {
    "signed0": dict(weights="signed0"),
    "no_affine": dict(weights="none"),
    "no_bias": dict(weights="no_bias"),
    "no_param_grads": dict(want_dweight=False, want_dbias=False),
    "momentum0": dict(momentum=0.0),
    "momentum1": dict(momentum=1.0),
    "eps1e-3": dict(eps=1e-3),
}
PARAMETER_CASES = [(par, shape, sem) for par in PARAMETERS
                   for shape, sem in (("odd", "oop_leaky"), ("hw1", "ip_leaky01_res"))]

# numeric edges on cut_plane and odd: (semantic, fp32 only, what is done to the inputs)
NUMERIC = {
    "constant_channel_oop": ("oop_leaky", False, "constant"),          # variance exactly 0
    "constant_channel_ip": ("ip_leaky001", False, "constant"),
    "large_mean": ("oop_identity", True, "large_mean"),                # bf16 cannot hold 1000 +- 0.1: fp32 only
    "dy_zero_oop": ("oop_relu_res", False, "dy_zero"),
    "dy_zero_ip": ("ip_elu_res", False, "dy_zero"),
    "elu_weight4": ("ip_elu_res", False, 4.0),                         # from-output oracle only: the exact one cannot
    "elu_weight20": ("ip_elu_res", False, 20.0),                       # be met here (include/ccnet_abn.h)
}
NUMERIC_CASES = [(name, shape, bf16) for name in NUMERIC for shape in ("cut_plane", "odd")
                 for bf16 in ((False,) if NUMERIC[name][1] else (False, True))]

MISALIGNED_CASES = [(sem, shape) for sem in ("oop_relu_res", "ip_leaky01_res", "ip_eval_elu")
                    for shape in ("odd", "block_tail")]
RANK_CASES = [(5, 2, "oop_leaky"), (5, 2, "ip_leaky001"), (7, 3, "oop_leaky"), (7, 3, "ip_leaky01_res")]
OUTPUTS = ("y", "dx", "dresidual", "dweight", "dbias", "running_mean", "running_var", "saved", "sums")


def table_inputs(shape, seed, **kw):
    """make_inputs with dy = noise + 0.25 (1 + the input's own normal draw).  A dy that is independent of x and of mean 0
    makes both gradient sums cancel to a residue of about sqrt(n), and with C = 1 or an unlucky draw to far less.  The bars
    are relative to the sums' scale, and measured against such a residue they are met or missed by the draw, not by the
    kernel: a few per cent of it can be the rounding of a stored bf16 y (elu' = y + alpha carries 2^-9 per element below
    y = -0.5) or the fp32 rounding of a mean of 1000.  With this dy, sum dz and sum dz xhat are both about n / 4."""
    return make_inputs(shape, seed, dy_signal=0.25, **kw)


def _seed(*names):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(map(str, names)))) % 100003


def _sem_kwargs(sem):
    act, p, source, residual, training, want_dres = SEMANTICS[sem]
    return dict(act=act, p=p, source=source, training=training), residual, want_dres


def _run_and_check(lib, mem, inputs, kw, bf16, family, want_dres=True, run_kw=None, **check_kw):
    x, w, b, rm, rv, dy, res = inputs
    r = run_abn(lib, mem, x, w, b, rm, rv, dy, residual=res, gamma_mode=kw["source"], bf16=bf16,
                want_dresidual=want_dres, **kw, **(run_kw or {}))
    check_case(r, x, w, b, rm, rv, dy, res, bf16=bf16, record=(mem.name, family), **kw, **check_kw)
    return r


def run_grid_case(lib, mem, shape, sem, bf16):
    kw, residual, want_dres = _sem_kwargs(sem)
    inputs = table_inputs(SHAPES[shape], _seed(shape, sem), residual=residual)
    family = ("in place" if kw["source"] else "out of place") + (", eval" if not kw["training"] else "")
    r = _run_and_check(lib, mem, inputs, kw, bf16, family, want_dres)
    assert ("dresidual" in r) == (residual and want_dres)
    if not kw["training"]:                    # eval mode leaves the running statistics as they were
        assert np.array_equal(r["running_mean"], inputs[3]) and np.array_equal(r["running_var"], inputs[4])
        assert r["saved"] is None


def run_parameter_case(lib, mem, par, shape, sem, bf16):
    kw, residual, want_dres = _sem_kwargs(sem)
    opts = dict(PARAMETERS[par])
    x, w, b, rm, rv, dy, res = table_inputs(SHAPES[shape], _seed(par, shape, sem), residual=residual)
    weights = opts.pop("weights", None)
    if weights == "signed0":
        w[0], w[1], w[2] = -1.25, 0.0, 0.75
    elif weights == "none":
        w = b = None
    elif weights == "no_bias":
        b = None
    run_kw = {k: opts.pop(k) for k in ("want_dweight", "want_dbias") if k in opts}
    kw.update(opts)                                                      # momentum, eps: the oracle takes them too
    r = _run_and_check(lib, mem, (x, w, b, rm, rv, dy, res), kw, bf16, "parameters", want_dres, run_kw=run_kw)
    if run_kw:
        assert r["dweight"] is None and r["dbias"] is None
    if weights == "signed0":
        assert all(np.isfinite(r[k]).all() for k in ("y", "dx", "dweight", "dbias", "sums"))
        if kw["source"] == 1:
            assert r["dweight"][1] == 0.0                                # d|w|/dw = sign(0) = 0


def run_numeric_case(lib, mem, name, shape, bf16):
    sem, _, what = NUMERIC[name]
    kw, residual, want_dres = _sem_kwargs(sem)
    seed = _seed(name, shape)
    check_kw = {}
    if what == "large_mean":
        x, w, b, rm, rv, dy, res = table_inputs(SHAPES[shape], seed, mean=1000.0, scale=0.1, residual=residual)
        # y and dx carry the fp32 rounding of the mean (ulp(1000) / 0.1 = 6e-4 of a standard deviation), as torch's do
        check_kw = dict(tol=2e-3, tol_y=1e-3)
    else:
        x, w, b, rm, rv, dy, res = table_inputs(SHAPES[shape], seed, residual=residual)
    if what == "constant":
        x[:, 0] = 0.75
        check_kw = dict(sum_floor=x.shape[1] == 1)
    elif what == "dy_zero":
        dy[:] = 0.0
    elif isinstance(what, float):
        w[:] = what
    family = "mean 1000 (its own bars)" if what == "large_mean" else "numeric edges"
    r = _run_and_check(lib, mem, (x, w, b, rm, rv, dy, res), kw, bf16, family, want_dres, **check_kw)
    f = O.forward(x, w, b, rm, rv, True, act=kw["act"], p=kw["p"], gamma_mode=kw["source"], residual=res)
    if what == "constant":
        assert r["saved"][0][0] == 0.75 and r["saved"][1][0] == 1.0 / np.sqrt(np.float64(np.float32(1e-5)))
    elif what == "large_mean":
        close(r["saved"][0], f["mean"], 1e-12, "mean")
        close(1.0 / r["saved"][1] ** 2, f["var"] + 1e-5, 1e-9, "var")
    elif what == "dy_zero":
        assert all(not np.any(r[k]) for k in ("dx", "dresidual", "dweight", "dbias", "sums"))
    return r, f


def run_misaligned_case(lib, mem, sem, shape, bf16):
    """every tensor, then only x (in place: only the shared x / y buffer), at each offset: bitwise the aligned result"""
    kw, residual, want_dres = _sem_kwargs(sem)
    x, w, b, rm, rv, dy, res = table_inputs(SHAPES[shape], _seed(sem, shape), residual=residual)
    run = lambda offsets: run_abn(lib, mem, x, w, b, rm, rv, dy, residual=res, gamma_mode=kw["source"], bf16=bf16,  # noqa
                                  offsets=offsets, **kw)
    aligned = run(None)
    check_case(aligned, x, w, b, rm, rv, dy, res, bf16=bf16, **kw)
    names = [t for t in TENSORS if res is not None or "residual" not in t]
    for off in OFFSETS[bf16]:
        for offsets in ({t: off for t in names}, {"y" if kw["source"] else "x": off}):
            got = run(offsets)
            for k in OUTPUTS:
                if aligned.get(k) is not None:
                    assert np.array_equal(got[k], aligned[k], equal_nan=True), (k, offsets)


def run_rank_case(lib, mem, N, R, sem):
    """fp32 only: the comparison with one rank is at 1e-6, far below a bf16 rounding of y"""
    kw, residual, want_dres = _sem_kwargs(sem)
    shape = (N, 3, 9, 11)
    x, w, b, rm, rv, dy, res = table_inputs(shape, _seed(N, R, sem), residual=residual)
    run = lambda ranks: run_abn(lib, mem, x, w, b, rm, rv, dy, residual=res, gamma_mode=kw["source"], ranks=ranks,  # noqa
                                **kw)
    one, many = run(1), run(R)
    check_case(many, x, w, b, rm, rv, dy, res, record=(mem.name, "uneven ranks"), **kw)
    for k in ("y", "dx", "running_mean", "running_var", "dweight", "dbias", "sums") + (("dresidual",) if residual else ()):
        close(many[k], one[k], 1e-6, k)
    assert many["saved"][2][0] == N * 99 and np.array_equal(many["saved"][2], one["saved"][2])


def run_nonfinite_case(lib, mem, sem):
    """fp32 on 'odd': one NaN, then one +inf, in channel 1.  The other channels' outputs and statistics are bitwise those
    of the clean run; channel 1's statistics are what the float64 oracle gives: NaN for running_var and invstd, and for
    running_mean NaN (NaN input) or +inf (the mean of a set that holds +inf)."""
    kw, residual, want_dres = _sem_kwargs(sem)
    shape = SHAPES["odd"]
    x, w, b, rm, rv, dy, res = table_inputs(shape, _seed("nonfinite", sem), residual=residual)
    run = lambda xx: run_abn(lib, mem, xx, w, b, rm, rv, dy, residual=res, gamma_mode=kw["source"], **kw)        # noqa: E731
    clean = run(x)
    check_case(clean, x, w, b, rm, rv, dy, res, **kw)
    others = [0, 2]
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[1, 1, 4, 5] = bad
        got = run(xb)
        with np.errstate(invalid="ignore"):
            f = O.forward(xb, w, b, rm, rv, True, act=kw["act"], p=kw["p"], gamma_mode=kw["source"], residual=res)
        for k in ("y", "dx", "dresidual"):
            if k in clean:
                assert np.array_equal(got[k][:, others], clean[k][:, others]), (k, bad)
        for k in ("dweight", "dbias", "running_mean", "running_var"):
            assert np.array_equal(got[k][others], clean[k][others]), (k, bad)
        for k in ("saved", "sums"):
            assert np.array_equal(got[k][:, others], clean[k][:, others]), (k, bad)
        assert np.isnan(f["running_var"][1]) and np.isnan(f["invstd"][1])
        assert np.isnan(got["running_var"][1]) and np.isnan(got["saved"][1][1]), (bad, got["running_var"], got["saved"])
        if np.isnan(bad):
            assert np.isnan(f["running_mean"][1]) and np.isnan(got["running_mean"][1]), (bad, got["running_mean"])
        else:
            assert f["running_mean"][1] == np.inf and got["running_mean"][1] == np.inf, (bad, got["running_mean"])


def in_place_design_error(act, p, weight, bf16, shape=(2, 5, 19, 21), seed=1):
    """What in-place mode costs by design, from the oracles alone: backward_from_output fed the exact y rounded to the storage
    type, against the exact backward.  Errors relative to scale (dx against gamma invstd dz), and the most negative z."""
    x, w, b, rm, rv, dy, res = make_inputs(shape, seed, residual=True)
    w[:] = weight
    if bf16:
        x, dy, res = bf16_round(x), bf16_round(dy), bf16_round(res)
    f = O.forward(x, w, b, rm, rv, True, act=act, p=p, gamma_mode=1, residual=res)
    g = O.backward(f, dy, w, True, act=act, p=p, gamma_mode=1)
    y = bf16_round(f["y"]) if bf16 else f["y"].astype(np.float32)
    h = O.backward_from_output(y, dy, res, w, b, f["mean"], f["invstd"], f["n"], True, act=act, p=p)
    rel = lambda k, scale=None: float(np.abs(h[k] - g[k]).max() / max(np.abs(g[k]).max(), scale or 0.0))    # noqa: E731
    return {"dx": rel("dx", dx_scale(f, g, w, 1)), "dweight": rel("dweight"), "dbias": rel("dbias"),
            "min_z": float(f["z"].min())}
