"""What the DSN cross-entropy tests share: the case table, the seeded inputs, the fixture loader and the numerics bar.

The fixtures (tests/golden/dsn_*.npz, written by tests/golden/make_dsn_golden.py from the unmodified reference criterion run
in float64) hold the truth; :func:`stock_reference` is the same composition from stock torch ops (F.interpolate +
F.cross_entropy), for cases no fixture covers.  Everything here is test infrastructure.
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_RTOL = 1e-5                 # loss within 1e-5 relative of the float64 reference (DESIGN.md §11's bar for a device criterion)
GRAD_RTOL = 1e-5                 # every gradient element within 1e-5 of that head's max|grad|
WEIGHTS = (1.0, 0.4)             # loss/criterion.py:31

# name: (B, C, h, w, H, W, seed, heads, logit scale, all_ignored)
CASES = {
    "s8": (2, 19, 13, 13, 97, 97, 1, 2, 3.0, False),             # the recipe's exact 1/8 ratio; batch > 1
    "nonsquare": (1, 19, 9, 17, 65, 129, 2, 2, 3.0, False),      # h != w, different tap counts per axis
    "frac": (1, 19, 7, 11, 50, 83, 3, 2, 3.0, False),            # inexact fp32 scale; footprint membership
    "identity": (1, 19, 33, 33, 33, 33, 4, 2, 3.0, False),       # scale 1, l1 = 0, last row and column with i1 == i0
    "line": (1, 19, 1, 5, 9, 33, 5, 2, 3.0, False),              # h = 1, scale 0 on one axis
    "c150": (1, 150, 6, 6, 41, 41, 6, 2, 3.0, False),            # ADE20K's class count
    "hot": (1, 19, 13, 13, 97, 97, 7, 2, 90.0, False),           # logits x 30: softmax stability
    "none_valid": (1, 19, 5, 5, 33, 33, 8, 2, 3.0, True),        # NaN loss, zero gradient
    "one_head": (1, 19, 13, 13, 97, 97, 9, 1, 3.0, False),       # len(preds) == 1
    "recipe": (1, 19, 97, 97, 769, 769, 10, 2, 3.0, False),      # the workload once
}


def fixture_path(name):
    return os.path.join(GOLDEN, "dsn_" + name + ".npz")


def fixture_names():
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "dsn_*.npz")))


def make_case_inputs(B, C, h, w, H, W, seed, heads=2, scale=3.0, all_ignored=False, ignored=0.10):
    """Seeded ([fp32 (B, C, h, w) logits per head], int64 (B, H, W) target with about `ignored` of the labels 255)."""
    rng = np.random.default_rng(seed)
    logits = [(rng.standard_normal((B, C, h, w)) * scale).astype(np.float32) for _ in range(heads)]
    target = rng.integers(0, C, (B, H, W)).astype(np.int64)
    target[rng.random((B, H, W)) < ignored] = 255
    if all_ignored:
        target[:] = 255
    return logits, target


def load_fixture(name):
    """The fixture as a dict, with its inputs regenerated from the stored seed."""
    z = np.load(fixture_path(name))
    fx = {k: z[k] for k in z.files}
    B, C, h, w, H, W = (int(v) for v in fx["shape"])
    fx["heads"] = int(fx["heads"])
    fx["logits"], fx["target"] = make_case_inputs(B, C, h, w, H, W, int(fx["seed"]), fx["heads"], float(fx["scale"]),
                                                  bool(fx["all_ignored"]))
    fx["name"] = name
    return fx


def check_against_fixture(fx, loss, grads, valid, out=print):
    """Hold a (loss, [gradient per head], valid count) to the bar against the fixture's float64 reference; the figures are
    printed before they are asserted."""
    assert int(valid) == int(fx["valid"]), (int(valid), int(fx["valid"]))
    ref = float(fx["loss"])
    if np.isnan(ref):
        out(f"{fx['name']}: loss {loss!r} (reference NaN)")
        assert np.isnan(loss)
    else:
        rel = abs(float(loss) - ref) / abs(ref)
        out(f"{fx['name']}: loss {float(loss)!r} reference {ref!r} relative error {rel:.3g} (bar {LOSS_RTOL:g})")
        assert rel <= LOSS_RTOL, (float(loss), ref, rel)
    assert len(grads) == fx["heads"]
    for k, g in enumerate(grads):
        g = np.asarray(g, np.float32)
        assert np.isfinite(g).all(), f"head {k}: gradient elements not written or not finite"
        if f"grad{k}" in fx:
            got, want = g.ravel().astype(np.float64), fx[f"grad{k}"].ravel()
        else:
            got, want = g.ravel()[fx[f"grad{k}_index"]].astype(np.float64), fx[f"grad{k}_sample"]
        top = float(fx[f"grad{k}_max"])
        err = float(np.abs(got - want).max())
        out(f"{fx['name']}: head {k} max|grad| {top:.6g} max error {err:.3g} = {err / top if top else 0:.3g} of max|grad| "
            f"(bar {GRAD_RTOL:g})")
        assert err <= GRAD_RTOL * top, (k, err, top)
        if top == 0:
            assert not g.any()


def stock_reference(logits, target, ignore_index=255, weights=WEIGHTS, dtype=None):
    """(loss, [gradient per head]) of the stock composition on the CPU: F.interpolate(align_corners=True) + F.cross_entropy
    per head, float64 unless ``dtype`` says otherwise."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    xs = [torch.from_numpy(np.asarray(l)).to(dtype).requires_grad_(True) for l in logits]
    t = torch.from_numpy(np.asarray(target))
    loss = sum(wt * F.cross_entropy(F.interpolate(x, size=t.shape[1:], mode="bilinear", align_corners=True), t,
                                    ignore_index=ignore_index) for wt, x in zip(weights, xs))
    loss.backward()
    return float(loss.detach()), [x.grad.numpy() for x in xs]


def run_raw(lib, mem, logits, target, weights=WEIGHTS, ignore_index=255, grad_out=1.0):
    """forward + backward through the C ABI on guarded buffers of ``mem`` (guarded_memory.HostMemory for the emulator build,
    DeviceMemory on the GPU).  Gradients, loss and workspace start as NaN; returns the results and whether every guard band
    is intact."""
    from guarded_memory import Buf
    heads = len(logits)
    B, C, h, w = logits[0].shape
    H, W = target.shape[1:]
    n = lib.ccnet_dsn_workspace_bytes(B, C, h, w, H, W, heads)
    assert 0 < n <= 16 * B * H * W + 65536 and n % 4 == 0, n
    nan = np.full(1, np.nan, np.float32)
    x = [Buf(mem, f"logits{k}", "f32", l.size, data=np.ascontiguousarray(l, np.float32)) for k, l in enumerate(logits)]
    g = [Buf(mem, f"grad{k}", "f32", l.size, data=np.full(l.size, np.nan, np.float32)) for k, l in enumerate(logits)]
    t = Buf(mem, "target", "f64", target.size, data=np.ascontiguousarray(target, np.int64))
    loss = Buf(mem, "loss", "f32", 1, data=nan)
    head_loss = Buf(mem, "head_loss", "f32", 2, data=np.repeat(nan, 2))
    counts = Buf(mem, "counts", "f32", 2, data=np.full(2, -7, np.int32))
    ws = Buf(mem, "workspace", "f32", n // 4, data=np.full(n // 4, np.nan, np.float32))
    go = Buf(mem, "grad_out", "f32", 1, data=np.full(1, grad_out, np.float32))
    second = (lambda bufs: bufs[1].ptr if heads == 2 else None)
    lib.check(lib.ccnet_dsn_forward_f32(x[0].ptr, second(x), t.ptr, weights[0], weights[1], loss.ptr, head_loss.ptr, counts.ptr,
                                        ws.ptr, n, B, C, h, w, H, W, heads, ignore_index, mem.stream), "forward")
    lib.check(lib.ccnet_dsn_backward_f32(go.ptr, x[0].ptr, second(x), g[0].ptr, second(g), weights[0], weights[1], ws.ptr, n,
                                         B, C, h, w, H, W, heads, mem.stream), "backward")
    intact, res = True, {}
    for buf, key, dt in [(loss, "loss", np.float32), (head_loss, "head_loss", np.float32), (counts, "counts", np.int32),
                         (ws, "workspace", np.uint8)] + [(b, f"grad{k}", np.float32) for k, b in enumerate(g)]:
        res[key], ok = buf.read(dt)
        assert ok, f"guard band of {key} overwritten"
        intact = intact and ok
    for buf in x + [t, go]:
        intact = intact and buf.read(np.uint8)[1]
    return {"loss": float(res["loss"][0]), "head_loss": res["head_loss"], "valid": int(res["counts"][0]),
            "out_of_range": int(res["counts"][1]), "grads": [res[f"grad{k}"].reshape(logits[k].shape) for k in range(heads)],
            "workspace": res["workspace"], "intact": intact}
