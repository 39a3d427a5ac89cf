"""numpy restatement of multi-scale evaluation (include/ccnet_mseval.h): the scaled size, ndimage.zoom's exact-ratio bilinear
resample in float64, the zoomed (and mirrored) zero-padded tiles, and the multi-scale score composed from
:func:`eval_oracle.sliding_scores`.  numpy only: scipy is needed to WRITE the fixtures (tests/golden/make_mseval_golden.py),
not to check against them.  Everything here is test infrastructure.
"""
from math import ceil

import numpy as np

import eval_oracle as O


def scaled_size(H, W, s):
    """ndimage.zoom's output size: Python's round (half to even) of H * s, W * s."""
    return max(int(round(H * float(s))), 1), max(int(round(W * float(s))), 1)


def axis(n_in, n_out):
    """Taps of every output index of an axis zoomed from n_in to n_out positions: (i0, i1, lambda), lambda the exact ratio
    rem / (n_out - 1) in float64 (the device rounds it to fp32)."""
    o = np.arange(n_out, dtype=np.int64)
    if n_out == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1)
    num = o * (n_in - 1)
    i0 = num // (n_out - 1)
    lam = (num % (n_out - 1)) / float(n_out - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), lam


def resample(a, out_h, out_w):
    """ndimage.zoom(a, (..., out_h / h, out_w / w), order=1, prefilter=False) on the last two axes, in float64."""
    a = np.asarray(a, np.float64)
    y0, y1, ly = axis(a.shape[-2], out_h)
    x0, x1, lx = axis(a.shape[-1], out_w)
    rows = (1 - ly)[:, None] * a[..., y0, :] + ly[:, None] * a[..., y1, :]
    return (1 - lx) * rows[..., x0] + lx * rows[..., x1]


def tile_grid(H, W, tile):
    """The reference's origins, with the project's divergence: at least one tile per axis."""
    stride = ceil(tile[0] * (1 - 1 / 3))
    rows, cols = max(int(ceil((H - tile[0]) / stride) + 1), 1), max(int(ceil((W - tile[1]) / stride) + 1), 1)
    return [(max(min(r * stride + tile[0], H) - tile[0], 0), max(min(c * stride + tile[1], W) - tile[1], 0))
            for r in range(rows) for c in range(cols)]


def geometry(H, W, s, tile, whole):
    """(Hs, Ws, origins, tile size) of one scale: the tile grid on the scaled image."""
    Hs, Ws = scaled_size(H, W, s)
    if whole:
        return Hs, Ws, [(0, 0)], (Hs, Ws)
    return Hs, Ws, tile_grid(Hs, Ws, tile), (int(tile[0]), int(tile[1]))


def zoom_tiles(image, Hs, Ws, origins, tile, flip):
    """(N, T + T_flip, Cin, th, tw) float64: the zero-padded tiles of the image zoomed to (Hs, Ws), then those of its copy
    mirrored along W."""
    z = resample(image, Hs, Ws)
    th, tw = tile
    out = []
    for v in ([z, z[..., ::-1]] if flip else [z]):
        for y1, x1 in origins:
            t = v[:, :, y1:y1 + th, x1:x1 + tw]
            out.append(np.pad(t, ((0, 0), (0, 0), (0, th - t.shape[2]), (0, tw - t.shape[3]))))
    return np.stack(out, 1)


def multiscale_scores(logits, geo, H, W, flip):
    """(N, C, H, W) float64: the mean over the scales of sliding_scores on (Hs, Ws) resampled to (H, W).  ``logits[i]`` is
    (N, T + T_flip, C, h, w) for ``geo[i]`` = (Hs, Ws, origins, tile)."""
    total = 0.0
    for lg, (Hs, Ws, origins, tile) in zip(logits, geo):
        total = total + resample(O.sliding_scores(lg, origins, tile, Hs, Ws, flip), H, W)
    return total / len(geo)


# ---- the fixtures of tests/golden/make_mseval_golden.py ----
def load_fixture(path):
    fx = O.load_fixture(path)
    fx["scales"] = [float(s) for s in fx["scales"]]
    fx["flip"] = bool(fx["flip"])
    fx["H"], fx["W"], fx["C"] = int(fx["H"]), int(fx["W"]), int(fx["C"])
    return fx


def fixture_geometry(fx):
    return [geometry(fx["H"], fx["W"], s, fx["tile"], fx["whole"]) for s in fx["scales"]]


def fixture_logits(fx):
    """Per scale, the toy net's (1, T + T_flip, C, h, w) fp32 outputs over the tiles of the fp32 zoomed image, on the CPU."""
    out = []
    for Hs, Ws, origins, tile in fixture_geometry(fx):
        zoomed = resample(fx["image"], Hs, Ws).astype(np.float32)
        out.append(O.fixture_tiles(dict(fx, image=zoomed, tile=tile), origins, fx["flip"]))
    return out


def fixture_scores(fx, logits=None):
    logits = fixture_logits(fx) if logits is None else logits
    return multiscale_scores(logits, fixture_geometry(fx), fx["H"], fx["W"], fx["flip"])


def check_against_fixture(fx, probs=None, pred=None, conf=None, rel=1e-5):
    """eval_oracle.check_against_fixture's rules against a multi-scale fixture: score within ``rel`` x max|logit| of the
    fixture's sample; pred identical except where the top-2 gap (of the oracle's multi-scale score) is below that bound;
    confusion off by at most one count per such pixel in each of the two cells it touches.  Returns the number of such pixels."""
    tol = rel * float(fx["max_abs_logit"])
    if probs is not None:
        got = np.asarray(probs, np.float64).ravel()[fx["probs_index"]]
        err = float(np.abs(got - fx["probs_sample"]).max())
        assert err <= tol, (err, tol)
    n_diff = 0
    if pred is not None:
        diff = np.asarray(pred) != fx["pred"]
        n_diff = int(diff.sum())
        if n_diff:
            gap = O.top2_gap(fixture_scores(fx))
            assert np.all(gap[diff] < tol), gap[diff]
        if conf is not None:
            d = np.abs(np.asarray(conf, np.int64) - fx["confusion"])
            assert int(d.sum()) <= 2 * n_diff and int(d.max(initial=0)) <= n_diff, (int(d.sum()), n_diff)
    elif conf is not None:
        np.testing.assert_array_equal(np.asarray(conf, np.int64), fx["confusion"])
    return n_diff
