"""The drivers and the case table of the multi-scale evaluation library (include/ccnet_mseval.h) at its limits, shared by the
SIMT-emulator tests (tests/test_mseval_host.py) and the device tests (tests/test_gpu_mseval.py).  A plain module, test
infrastructure only.

``run_tiles`` and ``run_accumulate`` call the C ABI directly on buffers of tests/guarded_memory.py: every tensor lies between
two bands of GUARD elements of a fixed bit pattern inside an allocation of its own, on ``HostMemory`` for the emulator build or
``DeviceMemory`` for the shipped library.  What the bands can show: a stray WRITE within 64 elements in front of or behind a
tensor.  What they cannot: a read outside a tensor (it goes unseen; that the kernels read none follows from their clamped
indices, by reading them), and a write further away than the bands reach.

The references are the float64 oracles (mseval_oracle.zoom_tiles / multiscale_scores, eval_oracle.argmax / top2_gap /
confusion) and the project's bars: a gathered tile within 1e-6 max|image|; a score within 1e-5 max|logit|; a prediction may
differ from the oracle's only where the oracle's top-2 gap is below that bar, and on at most 1 % of the pixels; the confusion
matrix equals confusion(label, the device's prediction) exactly.  Every check prints its error against its bar; ``WORST`` keeps
the largest ratio per kernel."""
import numpy as np

import eval_oracle as O
import mseval_oracle as M
from guarded_memory import Buf, DeviceMemory, HostMemory  # noqa: F401  (the tests reach them through here)

PRED_FILL = 0xEE                               # pred_out before the call: no class of a case with C <= 238
NEAR_TIE_SHARE = 0.01                          # of the pixels may differ from the oracle's prediction, all of them near ties
WORST = {"tiles": 0.0, "accumulate": 0.0}      # the largest error / bar seen per kernel in this process


def _note(kernel, name, err, bar, extra=""):
    WORST[kernel] = max(WORST[kernel], err / bar)
    print(f"{name}: max err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.3f}{extra}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def confusion_seed(C):
    """what the confusion buffer holds before a call: no cell is 0, so a kernel that stored its counts would be seen"""
    return (np.arange(C * C, dtype=np.int64).reshape(C, C) % 7 + 1) * 1000003


def pred_guard(C):
    """the byte of pred_out's guard bands: 0xCD unless that is a class of the case (then no byte is not; the bands still tell
    a stray write of any other value, and PRED_FILL differs from it)"""
    return 0xCD if C <= 0xCD else 0x5A


# ---------------------------------------------------------------------------------------------------------------------
# the two drivers
# ---------------------------------------------------------------------------------------------------------------------
def run_tiles(lib, mem, image, Hs, Ws, origins, tile, flip, first=0, count=None, offset=0):
    """One ccnet_mseval_tiles_f32 call on guarded buffers: (rc, tiles (N, count, Cin, th, tw), guards_intact).  ``tiles_out``
    starts as NaN and lies ``offset`` elements past a 16-byte boundary.  ``guards_intact``: the bands of tiles_out and of the
    image hold their pattern and the image holds the bytes uploaded -- stray writes only, a read outside the image goes unseen."""
    from ccnet_amd._mseval_lib import origins_array
    image = np.ascontiguousarray(image, np.float32)
    N, Cin, H, W = image.shape
    T = len(origins)
    count = T * (2 if flip else 1) - first if count is None else count
    shape = (N, count, Cin, tile[0], tile[1])
    n = int(np.prod(shape))
    src = Buf(mem, "image", "f32", image.size, 0, image)
    out = Buf(mem, "tiles_out", "f32", n, offset, np.full(n, np.nan, np.float32))
    rc = lib.ccnet_mseval_tiles_f32(src.ptr, N, Cin, H, W, Hs, Ws, T, T if flip else 0, origins_array(origins), tile[0],
                                    tile[1], first, count, out.ptr, mem.stream)
    tiles, ok = out.read(np.float32)
    back, ok_src = src.read(np.uint8)
    return rc, tiles.reshape(shape), ok and ok_src and np.array_equal(back, _bits(image))


def run_accumulate(lib, mem, logits, geo, H, W, flip, score_in=None, divide_by=0, labels=None, ignore_label=255,
                   want=("score", "pred", "conf"), in_place=False, offsets=None):
    """One ccnet_mseval_accumulate_f32 call on guarded buffers for ``geo`` = (Hs, Ws, origins, tile) and ``logits``
    (N, T + T_flip, C, h, w): (rc, score, pred, conf, guards_intact, inputs_unchanged).

    ``want`` names the outputs that are passed; the others are NULL and come back as None.  They start as NaN (score_out),
    PRED_FILL (pred_out) and ``confusion_seed(C)`` (confusion, returned as the buffer holds it: the counts are conf - seed), so
    an element that is not written and a ``=`` in place of ``+=`` both show.  ``labels`` without "conf" passes labels with a
    NULL confusion.  ``in_place`` passes score_in's buffer as score_out.  ``offsets`` = {"score_in", "score_out", "pred"} places
    those tensors that many elements past a 16-byte boundary (pred_out: at that byte); the kernels use element-wide accesses
    only, so nothing may depend on the alignment.  ``guards_intact``: every band of every buffer, inputs included, holds its
    pattern -- stray writes only, within GUARD elements; reads are not seen.  ``inputs_unchanged``: the bytes of the logits,
    the labels and (out of place) score_in after the call are those uploaded."""
    from ccnet_amd._mseval_lib import origins_array
    Hs, Ws, origins, tile = geo
    logits = np.ascontiguousarray(logits, np.float32)
    N, entries, C, h, w = logits.shape
    T = len(origins)
    assert entries == T * (2 if flip else 1) and set(want) <= {"score", "pred", "conf"}
    assert "conf" not in want or labels is not None
    assert not in_place or (score_in is not None and "score" in want)
    off = dict({"score_in": 0, "score_out": 0, "pred": 0}, **(offsets or {}))
    n = N * C * H * W
    bufs = [Buf(mem, "logits", "f32", logits.size, 0, logits)]
    inputs = [(bufs[0], logits)]
    lab = sin = sout = pred = conf = None
    if labels is not None:
        labels = np.ascontiguousarray(labels, np.int64)
        assert labels.shape == (N, H, W)
        lab = Buf(mem, "labels", "i64", labels.size, 0, labels)
        bufs.append(lab)
        inputs.append((lab, labels))
    if score_in is not None:
        score_in = np.ascontiguousarray(score_in, np.float32)
        assert score_in.shape == (N, C, H, W)
        sin = Buf(mem, "score_in", "f32", n, off["score_in"], score_in)
        bufs.append(sin)
        if not in_place:
            inputs.append((sin, score_in))
    if "score" in want:
        sout = sin if in_place else Buf(mem, "score_out", "f32", n, off["score_out"], np.full(n, np.nan, np.float32))
        bufs.append(sout)
    if "pred" in want:
        pred = Buf(mem, "pred_out", "u8", N * H * W, off["pred"], np.full(N * H * W, PRED_FILL, np.uint8),
                   pattern=pred_guard(C))
        bufs.append(pred)
    if "conf" in want:
        conf = Buf(mem, "confusion", "i64", C * C, 0, confusion_seed(C))
        bufs.append(conf)
    ptr = lambda b: None if b is None else b.ptr                                # noqa: E731
    rc = lib.ccnet_mseval_accumulate_f32(bufs[0].ptr, T, T if flip else 0, origins_array(origins), N, C, h, w, tile[0], tile[1],
                                         Hs, Ws, H, W, ptr(sin), ptr(sout), int(divide_by), ptr(lab), int(ignore_label),
                                         ptr(pred), ptr(conf), mem.stream)
    intact = all([b.read(np.uint8)[1] for b in bufs])
    same = all([np.array_equal(b.read(np.uint8)[0], _bits(a)) for b, a in inputs])
    score = None if sout is None else sout.read(np.float32)[0].reshape(N, C, H, W)
    p = None if pred is None else pred.read(np.uint8)[0].reshape(N, H, W)
    cm = None if conf is None else conf.read(np.int64)[0].reshape(C, C)
    return rc, score, p, cm, intact, same


# ---------------------------------------------------------------------------------------------------------------------
# the checks every case makes
# ---------------------------------------------------------------------------------------------------------------------
def rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def rand_logits(N, geo, C, hw, flip, seed):
    return rand((N, len(geo[2]) * (2 if flip else 1), C, hw[0], hw[1]), seed, 3.0)


def grid(Hs, Ws, tile):
    return Hs, Ws, M.tile_grid(Hs, Ws, tile), tile


def padding(N, Cin, H, W, Hs, Ws, origins, tile, flip):
    """where a tile leaves the scaled frame (pad_image's zeros), as a mask over (N, T + T_flip, Cin, th, tw)"""
    return M.zoom_tiles(np.ones((N, Cin, H, W)), Hs, Ws, origins, tile, flip) == 0


def tiles_ok(lib, mem, image, Hs, Ws, origins, tile, flip, first=0, count=None, offset=0):
    """run_tiles plus what holds for every call: rc, the guard bands, the padding exactly +0.0"""
    rc, got, intact = run_tiles(lib, mem, image, Hs, Ws, origins, tile, flip, first, count, offset)
    assert rc == 0, lib.last_error()
    assert intact, "a guard band of tiles_out or the image was written"
    pad = padding(*image.shape, Hs, Ws, origins, tile, flip)[:, first:first + got.shape[1]]
    assert np.all(got.view(np.uint32)[pad] == 0), "the padding is not +0.0"
    return got


def check_tiles(name, lib, mem, image, Hs, Ws, origins, tile, flip, offset=0):
    got = tiles_ok(lib, mem, image, Hs, Ws, origins, tile, flip, offset=offset)
    ref = M.zoom_tiles(image, Hs, Ws, origins, tile, flip)
    assert got.shape == ref.shape and not np.isnan(got).any(), "an element of tiles_out was not written"
    bar = 1e-6 * float(np.abs(image).max())
    err = float(np.abs(got - ref).max())
    _note("tiles", name, err, bar)
    assert err <= bar
    return got


def oracle_score(logits, geo, H, W, flip, score_in=None, divide_by=0):
    ref = M.multiscale_scores([logits], [geo], H, W, flip)
    if score_in is not None:
        ref = ref + np.asarray(score_in, np.float64)
    return ref / divide_by if divide_by > 0 else ref


def accumulate_ok(lib, mem, logits, geo, H, W, flip, **kw):
    """run_accumulate plus what holds for every call: rc, the guard bands, the inputs, every prediction written"""
    rc, score, pred, conf, intact, same = run_accumulate(lib, mem, logits, geo, H, W, flip, **kw)
    assert rc == 0, lib.last_error()
    assert intact, "a guard band was written"
    assert same, "an input was written"
    if pred is not None and logits.shape[2] <= PRED_FILL:
        assert not (pred == PRED_FILL).any(), "an element of pred_out was not written"
    return score, pred, conf


def check_accumulate(name, lib, mem, logits, geo, H, W, flip, labels=None, ignore_label=255, score_in=None, divide_by=0,
                     offsets=None, exact_pred=None, want=None):
    """One call against the float64 oracle at the project's bars; ``exact_pred`` replaces the near-tie rule (deliberate ties).
    Returns (score, pred, counts)."""
    C = logits.shape[2]
    want = (("score", "pred") + (("conf",) if labels is not None else ())) if want is None else want
    score, pred, conf = accumulate_ok(lib, mem, logits, geo, H, W, flip, score_in=score_in, divide_by=divide_by, labels=labels,
                                      ignore_label=ignore_label, want=want, offsets=offsets)
    ref = oracle_score(logits, geo, H, W, flip, score_in, divide_by)
    bar = 1e-5 * float(np.abs(logits).max())
    if score is not None:
        assert not np.isnan(score).any(), "an element of score_out was not written"
        err = float(np.abs(score - ref).max())
    if pred is not None:
        if exact_pred is not None:
            assert np.all(pred == exact_pred), f"{int((pred != exact_pred).sum())} predictions are not {exact_pred}"
            extra = ""
        else:
            gap, diff = O.top2_gap(ref), pred != O.argmax(ref)
            extra = (f", predictions differing {int(diff.sum())} of {diff.size}, the oracle's own gap below the bar at "
                     f"{int((gap < bar).sum())}")
            assert np.all(gap[diff] < bar), "a prediction differs where the oracle's top-2 gap is above the bar"
            assert diff.sum() <= NEAR_TIE_SHARE * diff.size
    if score is not None:
        _note("accumulate", name, err, bar, extra if pred is not None else "")
        assert err <= bar
    counts = None
    if conf is not None:
        counts = conf - confusion_seed(C)
        np.testing.assert_array_equal(counts, O.confusion(labels, pred, C, ignore_label))
    return score, pred, counts


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# A. the gather kernel.  N = 2, Cin = 3 throughout, the images independent draws: a wrong image or entry stride is a value error
# ---------------------------------------------------------------------------------------------------------------------
def _image(H, W, seed):
    return rand((2, 3, H, W), seed)


def _tiles_degenerate(H, W, Hs, Ws, flip):
    def case(lib, mem):            # an axis of one position: n_in == 1 (H or W is 1), n_out == 1 (Hs or Ws is 1); the tile pads
        check_tiles(f"tiles {H}x{W}->{Hs}x{Ws} flip={flip}", lib, mem, _image(H, W, 100 + H + W), *grid(Hs, Ws, (8, 8)), flip)
    return case


def tiles_tile_larger_than_the_frame(lib, mem):
    # 7 x 19 = 133 positions: one partial thread block; 5 x 6 of them inside the scaled frame
    check_tiles("tiles 9x12->5x6 tile 7x19", lib, mem, _image(9, 12, 111), 5, 6, [(0, 0)], (7, 19), True)


STRONG = {"up4": (6, 8, 24, 32), "down4": (40, 56, 10, 14)}


def _tiles_strong(key):
    def case(lib, mem):
        H, W, Hs, Ws = STRONG[key]
        check_tiles(f"tiles {H}x{W}->{Hs}x{Ws} tile 9x13", lib, mem, _image(H, W, 120 + H), *grid(Hs, Ws, (9, 13)), True)
    return case


def tiles_misplaced_output(lib, mem):
    H, W, Hs, Ws = STRONG["up4"]
    image, geo = _image(H, W, 120 + H), grid(Hs, Ws, (9, 13))
    base = tiles_ok(lib, mem, image, *geo, True)
    for offset in (1, 2, 3):
        assert same_bits(check_tiles(f"tiles_out + {offset}", lib, mem, image, *geo, True, offset=offset), base)


def tiles_boundary_chunk(lib, mem):
    image, geo = _image(40, 56, 130), grid(60, 84, (33, 33))
    T = len(geo[2])
    assert T == 12
    full = check_tiles("tiles 40x56->60x84 tile 33x33", lib, mem, image, *geo, True)
    for first, count in ((T - 1, 2), (T, 1), (2 * T - 1, 1)):       # the last plain and the first flipped entry in one call
        part = tiles_ok(lib, mem, image, *geo, True, first, count)
        assert same_bits(part, full[:, first:first + count]), (first, count)


def tiles_zero_weight_taps_are_not_read(lib, mem):
    """(5, 6) -> (9, 11): output o reads source o / 2; an odd o has weight 1/2 on both neighbours, an even o weight 0 on the
    second one, which must not be read: a non-finite source pixel (y, x) reaches exactly |oy - 2y| <= 1 and |ox - 2x| <= 1."""
    H, W, Hs, Ws = 5, 6, 9, 11
    clean = _image(H, W, 140)
    image = clean.copy()
    poison = [(0, 1, 2, 3, np.inf), (1, 2, 1, 2, np.nan), (1, 2, 3, 4, np.inf)]           # (n, channel, y, x, value)
    want = np.zeros((2, 2, 3, Hs, Ws), bool)
    oy, ox = np.arange(Hs)[:, None], np.arange(Ws)[None, :]
    for n, c, y, x, v in poison:
        assert 0 < y < H - 1 and 0 < x < W - 1
        image[n, c, y, x] = v
        hit = (np.abs(oy - 2 * y) <= 1) & (np.abs(ox - 2 * x) <= 1)
        want[n, 0, c] |= hit
        want[n, 1, c] |= hit[:, ::-1]                                                       # the flipped entry
    rc, got, intact = run_tiles(lib, mem, image, Hs, Ws, [(0, 0)], (Hs, Ws), True)
    assert rc == 0 and intact
    assert np.array_equal(~np.isfinite(got), want), "the non-finite outputs are not those with a non-zero weight on the poison"
    assert np.all(got[0, :, 1][want[0, :, 1]] == np.inf)
    assert np.all(np.isnan(got[1, :, 2, 1:4][want[1, :, 2, 1:4]])) and np.all(got[1, :, 2, 5:8][want[1, :, 2, 5:8]] == np.inf)
    ref = M.zoom_tiles(clean, Hs, Ws, [(0, 0)], (Hs, Ws), True)
    bar = 1e-6 * float(np.abs(clean).max())
    err = float(np.abs(got - ref)[~want].max())
    _note("tiles", "tiles 5x6->9x11 beside the poison", err, bar)
    assert err <= bar


# ---------------------------------------------------------------------------------------------------------------------
# B. the accumulate kernel
# ---------------------------------------------------------------------------------------------------------------------
def _labels(N, H, W, C, seed):
    return O.make_case_inputs(N, H, W, C, seed)[1]


def _acc_one_position_axis(Hs, Ws, H, W, hw):
    def case(lib, mem):            # n_in == 1: every output row (column) reads the frame's only row (column), lambda = 0
        geo = grid(Hs, Ws, (8, 8))
        assert len(geo[2]) == 3
        check_accumulate(f"accumulate {Hs}x{Ws}->{H}x{W} logits {hw}", lib, mem, rand_logits(2, geo, 3, hw, True, Hs + hw[0]),
                         geo, H, W, True, _labels(2, H, W, 3, 7))
    return case


def _spread(S, H, W):
    """the outputs of (H, W) that have a tap of non-zero weight on a position of the scaled-frame mask S"""
    out = np.zeros((H, W), bool)
    y0, y1, ly = M.axis(S.shape[0], H)
    x0, x1, lx = M.axis(S.shape[1], W)
    for ys, my in ((y0, np.ones(H, bool)), (y1, ly != 0)):
        for xs, mx in ((x0, np.ones(W, bool)), (x1, lx != 0)):
            out |= S[ys][:, xs] & my[:, None] & mx[None, :]
    return out


def acc_exact_ratio_zero_weight_taps(lib, mem):
    """(9, 11) -> (17, 21): output o sits on scaled position o / 2.  One +inf logit in one plain tile.  Inside a tile (header
    step 4) the bilinear sample is PyTorch's unconditional four-term sum, so the logit makes every position of its tile whose
    four neighbours include it non-finite, those with weight 0 on it as 0 * inf = NaN; the resample of step 5 then carries a
    position to exactly the outputs with a non-zero tap weight on it, and to no other."""
    N, C, H, W, flip = 2, 5, 17, 21, True
    geo = grid(9, 11, (8, 8))
    Hs, Ws, origins, tile = geo
    assert len(origins) == 4
    clean = rand_logits(N, geo, C, (3, 3), flip, 150)
    n0, t0, c0, py, px = 1, 1, 2, 1, 1
    logits = clean.copy()
    logits[n0, t0, c0, py, px] = np.inf
    y1, x1 = origins[t0]
    read, weighted = np.zeros((Hs, Ws), bool), np.zeros((Hs, Ws), bool)
    ya = O._axis(3, tile[0], np.arange(min(tile[0], Hs - y1)))
    xa = O._axis(3, tile[1], np.arange(min(tile[1], Ws - x1)))
    on = lambda a, p: ((a[0] == p) | (a[1] == p), ((a[0] == p) & (a[2] != 0)) | ((a[1] == p) & (a[3] != 0)))   # noqa: E731
    (ry, wy), (rx, wx) = on(ya, py), on(xa, px)
    read[y1:y1 + len(ry), x1:x1 + len(rx)] = ry[:, None] & rx[None, :]
    weighted[y1:y1 + len(wy), x1:x1 + len(wx)] = wy[:, None] & wx[None, :]
    want, narrow = _spread(read, H, W), _spread(weighted, H, W)
    assert narrow.any() and not (narrow & ~want).any() and not want.all()
    labels = _labels(N, H, W, C, 151)
    score, pred, conf = accumulate_ok(lib, mem, logits, geo, H, W, flip, labels=labels)
    bad = ~np.isfinite(score)
    print(f"accumulate exact ratio: {int(want.sum())} outputs reach the logit through non-zero taps on a position that "
          f"reads it, {int(narrow.sum())} of them with non-zero weights inside the tile too; non-finite {int(bad.sum())}")
    expect = np.zeros_like(bad)
    expect[n0, c0] = want
    assert np.array_equal(bad, expect), "the non-finite scores are not those the header's steps 4 and 5 give"
    ref = oracle_score(clean, geo, H, W, flip)
    bar = 1e-5 * float(np.abs(clean).max())
    err = float(np.abs(score - ref)[~expect].max())
    _note("accumulate", "accumulate 9x11->17x21 beside the +inf logit", err, bar)
    assert err <= bar
    assert np.all(pred[n0][want] == c0), "+inf or NaN is np.argmax's maximum"
    diff = (pred != O.argmax(ref)) & ~expect.any(1)
    assert np.all(O.top2_gap(ref)[diff] < bar) and diff.sum() <= NEAR_TIE_SHARE * diff.size
    np.testing.assert_array_equal(conf - confusion_seed(C), O.confusion(labels, pred, C))


TIES = ("all_equal", "two_at_plus_inf", "all_minus_inf")


def _acc_ties(kind):
    def case(lib, mem):
        N, C, H, W, flip = 2, 4, 15, 21, True
        geo = grid(10, 14, (8, 8))
        labels = _labels(N, H, W, C, 160)
        logits = np.full((N, 2 * len(geo[2]), C, 2, 2), 1.5, np.float32)
        if kind == "all_equal":                                   # every class the same score: the first one
            score, _, _ = check_accumulate("accumulate all logits equal", lib, mem, logits, geo, H, W, flip, labels, exact_pred=0)
            assert np.all(score == score[:, :1])
            return
        if kind == "two_at_plus_inf":                             # +inf, or NaN where a tile's sample has a weight of 0
            logits[:, :, (1, 3)] = np.inf
        else:                                                     # the first scale's `c == 0 ||`: no score is > -inf
            logits[:] = -np.inf
        score, pred, conf = accumulate_ok(lib, mem, logits, geo, H, W, flip, labels=labels)
        if kind == "two_at_plus_inf":
            assert np.abs(score[:, (0, 2)] - 1.5).max() <= 1e-5 * 1.5
            assert np.all((score[:, (1, 3)] == np.inf) | np.isnan(score[:, (1, 3)]))
            assert np.all(np.isnan(score[:, 1]) == np.isnan(score[:, 3]))
        else:
            assert np.all((score == -np.inf) | np.isnan(score))
        first = 1 if kind == "two_at_plus_inf" else 0
        assert np.all(pred == first), f"{int((pred != first).sum())} predictions are not {first}"
        np.testing.assert_array_equal(conf - confusion_seed(C), O.confusion(labels, pred, C))
    return case


LABEL_SHAPE = (2, 19, 30, 41)                                    # N, C, H, W; scaled frame (20, 28), six 13 x 13 tiles, flip


def _label_inputs():
    N, C, H, W = LABEL_SHAPE
    geo = grid(20, 28, (13, 13))
    assert len(geo[2]) == 6
    return geo, rand_logits(N, geo, C, (3, 3), True, 170)


def acc_ignore_label_inside_the_classes(lib, mem):
    N, C, H, W = LABEL_SHAPE
    geo, logits = _label_inputs()
    rng = np.random.default_rng(171)
    labels = rng.integers(-300, 300, (N, H, W)).astype(np.int64)                # rows 2::3: mostly out of range
    labels[:, ::3] = 7                                                          # the ignore label, inside [0, C)
    labels[:, 1::3] = rng.integers(0, C, (N, len(range(1, H, 3)), W))
    counted = (labels != 7) & (labels >= 0) & (labels < C)
    assert (labels < 0).any() and (labels >= C).any() and counted.any()
    _, _, counts = check_accumulate("accumulate ignore label 7", lib, mem, logits, geo, H, W, True, labels, ignore_label=7)
    assert int(counts.sum()) == int(counted.sum()) and not counts[7].any()


def acc_ignore_label_minus_one(lib, mem):
    N, C, H, W = LABEL_SHAPE
    geo, logits = _label_inputs()
    rng = np.random.default_rng(172)
    labels = rng.integers(0, C, (N, H, W)).astype(np.int64)
    labels[rng.random((N, H, W)) < 0.1] = -1
    labels[rng.random((N, H, W)) < 0.1] = 255                                   # not the ignore label here, but >= C
    counted = (labels >= 0) & (labels < C)
    _, _, counts = check_accumulate("accumulate ignore label -1", lib, mem, logits, geo, H, W, True, labels, ignore_label=-1)
    assert (labels == -1).any() and (labels == 255).any() and int(counts.sum()) == int(counted.sum())


def acc_all_labels_ignored(lib, mem):
    N, C, H, W = LABEL_SHAPE
    geo, logits = _label_inputs()
    labels = np.full((N, H, W), 255, np.int64)
    rc, _, _, conf, intact, same = run_accumulate(lib, mem, logits, geo, H, W, True, labels=labels)
    assert rc == 0 and intact and same
    assert same_bits(conf, confusion_seed(C)), "the confusion buffer is not its seed"


def acc_labels_without_confusion(lib, mem):
    N, C, H, W = LABEL_SHAPE
    geo, logits = _label_inputs()
    plain = accumulate_ok(lib, mem, logits, geo, H, W, True, want=("score", "pred"))
    with_labels = accumulate_ok(lib, mem, logits, geo, H, W, True, labels=_labels(N, H, W, C, 173), want=("score", "pred"))
    assert same_bits(plain[0], with_labels[0]) and same_bits(plain[1], with_labels[1]) and with_labels[2] is None


def acc_optional_outputs_divide_by_and_in_place(lib, mem):
    N, C, H, W, flip = 2, 4, 15, 21, True
    geo = [grid(10, 14, (8, 8)), grid(20, 28, (13, 13))]
    logits = [rand_logits(N, g, C, (2, 2), flip, 180 + i) for i, g in enumerate(geo)]
    odd = {"score_in": 1, "score_out": 3, "pred": 1}
    # the first scale, score_in NULL: each output alone and both, then divided
    both = check_accumulate("accumulate first scale", lib, mem, logits[0], geo[0], H, W, flip, offsets=odd)
    only_pred = accumulate_ok(lib, mem, logits[0], geo[0], H, W, flip, want=("pred",), offsets=odd)
    only_score = accumulate_ok(lib, mem, logits[0], geo[0], H, W, flip, want=("score",))
    assert only_pred[0] is None and only_score[1] is None
    assert same_bits(only_pred[1], both[1]) and same_bits(only_score[0], both[0])
    third = check_accumulate("accumulate first scale / 3", lib, mem, logits[0], geo[0], H, W, flip, divide_by=3)
    assert same_bits(third[0], both[0] / np.float32(3)) and not same_bits(third[0], both[0])
    # the second scale on top of the first: out of place, then in place 1 to 3 elements off a 16-byte boundary
    labels = _labels(N, H, W, C, 182)
    out = check_accumulate("accumulate second scale", lib, mem, logits[1], geo[1], H, W, flip, labels, score_in=both[0],
                           divide_by=2, offsets=odd)
    for k in (1, 2, 3):
        inp = accumulate_ok(lib, mem, logits[1], geo[1], H, W, flip, score_in=both[0], divide_by=2, labels=labels,
                            in_place=True, offsets={"score_in": k, "pred": k})
        assert same_bits(inp[0], out[0]) and same_bits(inp[1], out[1]) and same_bits(inp[2] - confusion_seed(C), out[2])


def _acc_one_past(H, W, Hs, Ws, flip):
    def case(lib, mem):            # the last workgroup counts H * W - 4096 pixels: 1 (one thread) and 16 (part of a thread row)
        geo = grid(Hs, Ws, (8, 8))
        labels = np.random.default_rng(H).integers(0, 2, (2, H, W)).astype(np.int64)
        _, _, counts = check_accumulate(f"accumulate {Hs}x{Ws}->{H}x{W}", lib, mem, rand_logits(2, geo, 2, (2, 2), flip, 190 + H),
                                        geo, H, W, flip, labels)
        assert int(counts.sum()) == 2 * H * W
    return case


def acc_c256(lib, mem):
    """C = 256 at a scale != 1: the 128 KiB histogram, which needs the kernel's dynamic LDS grant"""
    N, C, H, W = 1, 256, 60, 80
    geo = grid(30, 40, (33, 33))
    assert len(geo[2]) == 2
    logits = rand_logits(N, geo, C, (5, 5), False, 200)
    logits[:, :, 255] += 4.0                                                    # pred 255 is common
    labels = np.random.default_rng(201).integers(0, C, (N, H, W)).astype(np.int64)
    labels[:, :, :40] = 255
    labels[0, 0, :10] = -1                                                      # the ignore label
    _, _, counts = check_accumulate("accumulate C=256", lib, mem, logits, geo, H, W, False, labels, ignore_label=-1)
    assert counts[255, 255] > 0 and int(counts.sum()) == H * W - 10


def acc_64_tiles_with_flip(lib, mem):
    """T = T_flip = 64 at a scale != 1: cover counts up to 9 in each byte of the packed tap counts"""
    N, C, H, W = 1, 5, 138, 138
    geo = grid(552, 552, (97, 97))
    assert len(geo[2]) == 64
    check_accumulate("accumulate 64 tiles + flip", lib, mem, rand_logits(N, geo, C, (13, 13), True, 210), geo, H, W, True,
                     _labels(N, H, W, C, 211))


def _acc_saturation(low_half):
    def case(lib, mem):            # every counted pixel of a workgroup, 4096, in one 16-bit counter, at a scale != 1
        C, H, W = 19, 111, 111
        l, a = (2, 4) if low_half else (2, 5)
        assert ((l * C + a) % 2 == 0) == low_half
        logits = np.zeros((1, 1, C, 7, 7), np.float32)
        logits[:, :, a] = 10.0
        labels = np.full((1, H, W), l, np.int64)
        labels[0, 5, 7:11] = 255
        labels[0, 90, 3] = C
        n = int((labels == l).sum())
        assert n >= 3 * 4096 + 17
        _, _, counts = check_accumulate(f"accumulate saturation cell ({l}, {a})", lib, mem, logits, (56, 56, [(0, 0)], (56, 56)),
                                        H, W, False, labels, exact_pred=a)
        assert int(counts[l, a]) == n and int(counts.sum()) == n
    return case


# ---------------------------------------------------------------------------------------------------------------------
# the table: name -> case(lib, mem).  The shapes are the smallest that reach each path.  Every case runs on both back ends: the
# three large ones (C = 256, 64 tiles + flip, counter saturation) take 0.03 to 0.35 s each in the SIMT emulator, measured, so
# none is left to the device alone.
# Near ties, from the float64 oracle alone (every case prints them): pixels whose top-2 gap is below the score bar, of all --
#   one-row and one-column frames 0 / 480 (both logit shapes), exact ratio 0 / 714, labels 4 / 2460, optional outputs 0 / 630
#   (first scale) and 1 / 630 (second), one past a workgroup 0 / 8194, one past a thread row 0 / 8224, C = 256: 0 / 4800,
#   64 tiles: 0 / 19044 -- far below the 1 % that NEAR_TIE_SHARE allows.
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}
for _H, _W, _Hs, _Ws in ((1, 9, 1, 18), (2, 9, 1, 5), (7, 1, 14, 1), (7, 2, 4, 1)):
    for _flip in (False, True):
        CASES[f"tiles_{_H}x{_W}_to_{_Hs}x{_Ws}_{'flip' if _flip else 'plain'}"] = _tiles_degenerate(_H, _W, _Hs, _Ws, _flip)
CASES.update({
    "tiles_tile_larger_than_the_frame": tiles_tile_larger_than_the_frame,
    "tiles_up4": _tiles_strong("up4"),
    "tiles_down4": _tiles_strong("down4"),
    "tiles_boundary_chunk": tiles_boundary_chunk,
    "tiles_zero_weight_taps_are_not_read": tiles_zero_weight_taps_are_not_read,
    "tiles_misplaced_output": tiles_misplaced_output,
    "acc_one_row_frame_logits_1x1": _acc_one_position_axis(1, 20, 12, 20, (1, 1)),
    "acc_one_row_frame_logits_2x2": _acc_one_position_axis(1, 20, 12, 20, (2, 2)),
    "acc_one_column_frame_logits_1x1": _acc_one_position_axis(20, 1, 20, 12, (1, 1)),
    "acc_one_column_frame_logits_2x2": _acc_one_position_axis(20, 1, 20, 12, (2, 2)),
    "acc_exact_ratio_zero_weight_taps": acc_exact_ratio_zero_weight_taps,
})
CASES.update({f"acc_ties_{_k}": _acc_ties(_k) for _k in TIES})
CASES.update({
    "acc_ignore_label_inside_the_classes": acc_ignore_label_inside_the_classes,
    "acc_ignore_label_minus_one": acc_ignore_label_minus_one,
    "acc_all_labels_ignored": acc_all_labels_ignored,
    "acc_labels_without_confusion": acc_labels_without_confusion,
    "acc_optional_outputs_divide_by_and_in_place": acc_optional_outputs_divide_by_and_in_place,
    "acc_one_past_a_workgroup": _acc_one_past(1, 4097, 1, 33, True),
    "acc_one_past_a_thread_row": _acc_one_past(257, 16, 17, 4, False),
    "acc_c256": acc_c256,
    "acc_64_tiles_with_flip": acc_64_tiles_with_flip,
    "acc_saturation_low_half": _acc_saturation(True),
    "acc_saturation_high_half": _acc_saturation(False),
})
ALL = list(CASES)


def run_case(name, lib, mem):
    CASES[name](lib, mem)
