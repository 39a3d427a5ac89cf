"""The driver and the case table of the single-scale evaluation library (include/ccnet_eval.h, ccnet_eval_sliding_f32) at its
limits, shared by the SIMT-emulator tests (tests/test_eval_host.py) and the device tests (tests/test_gpu_eval.py).  A plain
module, test infrastructure only; what it shares with the multi-scale table it imports from tests/mseval_cases.py.

``run_sliding`` calls the C ABI directly on buffers of tests/guarded_memory.py: every tensor lies between two bands of GUARD
elements of a fixed bit pattern inside an allocation of its own, on ``HostMemory`` for the emulator build or ``DeviceMemory`` for
the shipped library.  What the bands can show: a stray WRITE within 64 elements in front of or behind a tensor -- one element
past pred_out, the padding half of the last histogram word at odd C, an element in front of probs_out.  What they cannot: a read
outside a tensor (it goes unseen; that the kernel reads none follows from its clamped indices, by reading them), a write further
away than the bands reach, and a read-modify-write that leaves the bits as they were (an atomic add of 0).

The reference is the float64 oracle (eval_oracle.sliding_scores / argmax / top2_gap / confusion) at the project's bars: a score
within 1e-5 max|logit|; a prediction may differ from the oracle's only where the oracle's top-2 gap is below that bar, and on at
most 1 % of the pixels; the confusion counts equal confusion(label, the library's own prediction) exactly.  Every check prints
its error against its bar; ``WORST`` keeps the largest ratio.  Every call is also made through ccnet_mseval_accumulate_f32 at
Hs = H, Ws = W with no score_in and divide_by = 0, which mseval_kernels.hpp promises to be the same score bit for bit, the same
prediction and the same counts -- scores that are not finite included."""
import numpy as np

import eval_oracle as O
import mseval_oracle as M
from guarded_memory import Buf, DeviceMemory, HostMemory  # noqa: F401  (the tests reach them through here)
from mseval_cases import NEAR_TIE_SHARE, PRED_FILL, _bits, confusion_seed, pred_guard, rand, run_accumulate, same_bits

WORST = {"sliding": 0.0}                       # the largest error / bar seen in this process


def _note(name, err, bar, extra=""):
    WORST["sliding"] = max(WORST["sliding"], err / bar)
    print(f"{name}: max err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.3f}{extra}")


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def run_sliding(lib, mem, logits, origins, tile, H, W, flip, labels=None, ignore_label=255, want=("probs", "pred", "conf"),
                offsets=None, conf_init=None):
    """One ccnet_eval_sliding_f32 call on guarded buffers for ``logits`` (N, T + T_flip, C, h, w):
    (rc, probs, pred, conf, guards_intact, inputs_unchanged).

    ``want`` names the outputs that are passed; the others are NULL and come back as None.  They start as NaN (probs_out),
    PRED_FILL (pred_out) and ``confusion_seed(C)`` (confusion; ``conf_init`` replaces the seed, for a second call into the same
    counts; returned as the buffer holds it: the counts are conf - what it started as), so an element that is not written and a
    ``=`` in place of ``+=`` both show.  ``labels`` without "conf" passes labels with a NULL confusion.  ``offsets`` =
    {"probs", "pred"} places those tensors that many elements past a 16-byte boundary (pred_out: at that byte); the kernel uses
    element-wide accesses only, so nothing may depend on the alignment.  ``guards_intact``: every band of every buffer, inputs
    included, holds its pattern -- stray writes only, within GUARD = 64 elements of a tensor; a read outside a tensor is not
    seen.  ``inputs_unchanged``: the bytes of the logits and the labels after the call are those uploaded."""
    from ccnet_amd._eval_lib import origins_array
    logits = np.ascontiguousarray(logits, np.float32)
    N, entries, C, h, w = logits.shape
    T = len(origins)
    assert entries == T * (2 if flip else 1) and set(want) <= {"probs", "pred", "conf"}
    assert "conf" not in want or labels is not None
    off = dict({"probs": 0, "pred": 0}, **(offsets or {}))
    bufs = [Buf(mem, "logits", "f32", logits.size, 0, logits)]
    inputs = [(bufs[0], logits)]
    lab = probs = pred = conf = None
    if labels is not None:
        labels = np.ascontiguousarray(labels, np.int64)
        assert labels.shape == (N, H, W)
        lab = Buf(mem, "labels", "i64", labels.size, 0, labels)
        bufs.append(lab)
        inputs.append((lab, labels))
    if "probs" in want:
        n = N * C * H * W
        probs = Buf(mem, "probs_out", "f32", n, off["probs"], np.full(n, np.nan, np.float32))
        bufs.append(probs)
    if "pred" in want:
        pred = Buf(mem, "pred_out", "u8", N * H * W, off["pred"], np.full(N * H * W, PRED_FILL, np.uint8), pattern=pred_guard(C))
        bufs.append(pred)
    if "conf" in want:
        conf = Buf(mem, "confusion", "i64", C * C, 0, confusion_seed(C) if conf_init is None else conf_init)
        bufs.append(conf)
    ptr = lambda b: None if b is None else b.ptr                                # noqa: E731
    rc = lib.ccnet_eval_sliding_f32(bufs[0].ptr, T, T if flip else 0, origins_array(origins), N, C, h, w, tile[0], tile[1], H, W,
                                    ptr(lab), int(ignore_label), ptr(probs), ptr(pred), ptr(conf), mem.stream)
    intact = all([b.read(np.uint8)[1] for b in bufs])
    same = all([np.array_equal(b.read(np.uint8)[0], _bits(a)) for b, a in inputs])
    p = None if probs is None else probs.read(np.float32)[0].reshape(N, C, H, W)
    q = None if pred is None else pred.read(np.uint8)[0].reshape(N, H, W)
    cm = None if conf is None else conf.read(np.int64)[0].reshape(C, C)
    return rc, p, q, cm, intact, same


# ---------------------------------------------------------------------------------------------------------------------
# the checks every case makes
# ---------------------------------------------------------------------------------------------------------------------
def sliding_ok(lib, ms, mem, logits, origins, tile, H, W, flip, labels=None, ignore_label=255, want=("probs", "pred", "conf"),
               offsets=None, conf_init=None):
    """run_sliding plus what holds for every call: rc, the guard bands, the inputs, every prediction written, and the same call
    through the multi-scale library ``ms`` (its outputs at offset 0): the same bits, predictions and counts."""
    C = logits.shape[2]
    want = tuple(k for k in want if k != "conf" or labels is not None)
    rc, probs, pred, conf, intact, same = run_sliding(lib, mem, logits, origins, tile, H, W, flip, labels, ignore_label, want,
                                                      offsets, conf_init)
    assert rc == 0, lib.last_error()
    assert intact, "a guard band was written"
    assert same, "an input was written"
    if pred is not None and C <= PRED_FILL:
        assert not (pred == PRED_FILL).any(), "an element of pred_out was not written"
    names = {"probs": "score", "pred": "pred", "conf": "conf"}
    rc, score2, pred2, conf2, intact, same = run_accumulate(ms, mem, logits, (H, W, origins, tile), H, W, flip, labels=labels,
                                                            ignore_label=ignore_label, want=tuple(names[k] for k in want))
    assert rc == 0 and intact and same, ms.last_error()
    if probs is not None:
        assert same_bits(probs, score2), "the multi-scale library's score at Hs = H, Ws = W has other bits"
    if pred is not None:
        assert np.array_equal(pred, pred2), f"the two libraries' predictions differ at {int((pred != pred2).sum())} pixels"
    if conf is not None:
        start = confusion_seed(C) if conf_init is None else conf_init
        np.testing.assert_array_equal(conf - start, conf2 - confusion_seed(C))
    return probs, pred, conf


def oracle(logits, origins, tile, H, W, flip):
    with np.errstate(invalid="ignore", divide="ignore"):                        # 0 / 0 where no tile covers a pixel
        return O.sliding_scores(logits, origins, tile, H, W, flip)


def compare(name, probs, pred, ref, bar, held=None):
    """``probs`` and ``pred`` against the float64 ``ref`` on the pixels ``held`` (N, H, W; default all): the score within ``bar``;
    a prediction other than np.argmax's only where the oracle's top-2 gap is below it, and on at most NEAR_TIE_SHARE of them.
    First, on the oracle alone: no more than NEAR_TIE_SHARE of the pixels are such near ties."""
    N, C = ref.shape[:2]
    held = np.ones(ref[:, 0].shape, bool) if held is None else held
    extra = ""
    if C > 1:
        gap = O.top2_gap(np.where(held[:, None], ref, 0.0))
        near = (gap < bar) & held
        assert near.sum() <= NEAR_TIE_SHARE * held.sum(), f"{name}: the oracle has {int(near.sum())} near ties, re-seed the case"
    if pred is not None:
        if C == 1:
            assert np.all(pred == 0)
        else:
            diff = (pred != O.argmax(ref)) & held
            extra = (f", predictions differing {int(diff.sum())} of {int(held.sum())}, the oracle's own gap below the bar at "
                     f"{int(near.sum())}")
            assert np.all(gap[diff] < bar), "a prediction differs where the oracle's top-2 gap is above the bar"
            assert diff.sum() <= NEAR_TIE_SHARE * held.sum()
    if probs is not None:
        at = np.broadcast_to(held[:, None], ref.shape)
        assert not np.isnan(probs[at]).any(), "an element of probs_out was not written"
        err = float(np.abs(probs - ref)[at].max())
        _note(name, err, bar, extra)
        assert err <= bar


def check_sliding(name, lib, ms, mem, logits, origins, tile, H, W, flip, labels=None, ignore_label=255, offsets=None,
                  exact_pred=None, want=("probs", "pred", "conf"), conf_init=None):
    """One call against the float64 oracle at the project's bars; ``exact_pred`` replaces the near-tie rule (deliberate ties).
    Returns (probs, pred, counts)."""
    C = logits.shape[2]
    probs, pred, conf = sliding_ok(lib, ms, mem, logits, origins, tile, H, W, flip, labels, ignore_label, want, offsets, conf_init)
    ref = oracle(logits, origins, tile, H, W, flip)
    bar = 1e-5 * float(np.abs(logits).max())
    if exact_pred is not None:
        if pred is not None:
            assert np.all(pred == exact_pred), f"{int((pred != exact_pred).sum())} predictions are not {exact_pred}"
        if probs is not None:
            err = float(np.abs(probs - ref).max())
            _note(name, err, bar)
            assert err <= bar
    else:
        compare(name, probs, pred, ref, bar)
    counts = None
    if conf is not None:
        counts = conf - (confusion_seed(C) if conf_init is None else conf_init)
        np.testing.assert_array_equal(counts, O.confusion(labels, pred, C, ignore_label))
    return probs, pred, counts


# ---------------------------------------------------------------------------------------------------------------------
# the cases.  N = 2 unless noted, the two images independent draws: a wrong image stride is a value error
# ---------------------------------------------------------------------------------------------------------------------
def rand_logits(N, T, C, hw, flip, seed):
    return rand((N, T * (2 if flip else 1), C, hw[0], hw[1]), seed, 3.0)


def _labels(N, H, W, C, seed):
    return O.make_case_inputs(N, H, W, C, seed)[1]


def _plain(name, H, W, tile, hw, flip, C=3, origins=None, seed=0, N=2):
    """a random case on the tile grid of (H, W) (or the given origins) with the usual labels"""
    def case(lib, ms, mem):
        org = M.tile_grid(H, W, tile) if origins is None else origins
        check_sliding(name, lib, ms, mem, rand_logits(N, len(org), C, hw, flip, 300 + seed), org, tile, H, W, flip,
                      _labels(N, H, W, C, 400 + seed))
    return case


def asymmetric_two_tiles_under_flip(lib, ms, mem):
    """tiles of 15 columns at 0 and 9 on 20 columns, the second cut at the edge: columns 9..14 have two tiles in the plain pass,
    their mirror images 5..10 in the flipped one, so the two cover counts of a pixel differ on 5..8 and 11..14"""
    H, W, tile, origins = 6, 20, (6, 15), [(0, 0), (0, 9)]
    cover = np.zeros(W, int)
    for _, x1 in origins:
        cover[x1:x1 + tile[1]] += 1
    assert (cover != cover[::-1]).sum() == 8 and cover.min() == 1
    check_sliding("two tiles at 0 and 9 of 20 columns + flip", lib, ms, mem, rand_logits(2, 2, 5, (2, 3), True, 310), origins,
                  tile, H, W, True, _labels(2, H, W, 5, 311))


def uncovered_pixel(lib, ms, mem):
    """tiles of 4 columns at 0 and 4 on 9 columns leave column 8 without a tile in the plain pass and column 0 (its mirror image)
    in the flipped pass.  ccnet_eval.h: 0 / 0 = NaN for every class there, whichever pass it is, pred = 0, counted at [label][0];
    nothing is written outside the outputs.  Every other pixel is held to the oracle."""
    N, C, H, W, tile, origins = 2, 5, 6, 9, (6, 4), [(0, 0), (0, 4)]
    logits = rand_logits(N, 2, C, (2, 2), True, 320)
    labels = np.random.default_rng(321).integers(0, C, (N, H, W)).astype(np.int64)
    probs, pred, conf = sliding_ok(lib, ms, mem, logits, origins, tile, H, W, True, labels)
    ref = oracle(logits, origins, tile, H, W, True)
    bare = np.zeros((N, H, W), bool)
    bare[:, :, (0, 8)] = True
    assert np.array_equal(np.isnan(ref), np.broadcast_to(bare[:, None], ref.shape))          # the oracle says the same
    assert np.array_equal(np.isnan(probs), np.isnan(ref)), "the NaN scores are not those of the two uncovered columns"
    assert np.all(pred[bare] == 0) and np.all(O.argmax(ref)[bare] == 0)
    compare("uncovered pixel: the covered ones", probs, pred, ref, 1e-5 * float(np.abs(logits).max()), ~bare)
    counts = conf - confusion_seed(C)
    np.testing.assert_array_equal(counts, O.confusion(labels, pred, C))
    assert int(counts[:, 0].sum()) >= int(bare.sum()) and int(counts.sum()) == N * H * W


def _one_past(H, W, tile, origins, flip):
    def case(lib, ms, mem):            # the last workgroup counts H * W - 4096 pixels: 1 (one thread) and 16 (part of a thread row)
        labels = np.random.default_rng(H).integers(0, 2, (2, H, W)).astype(np.int64)
        _, _, counts = check_sliding(f"{H}x{W} = 4096 + {H * W - 4096} pixels", lib, ms, mem,
                                     rand_logits(2, len(origins), 2, (3, 5), flip, 330 + H), origins, tile, H, W, flip, labels)
        assert int(counts.sum()) == 2 * H * W
    return case


def one_class(lib, ms, mem):
    H, W, tile = 12, 20, (8, 8)
    origins = M.tile_grid(H, W, tile)
    labels = np.zeros((2, H, W), np.int64)
    labels[:, ::5] = 255
    labels[:, 1::5] = 1                                                         # >= C
    _, pred, counts = check_sliding("C = 1", lib, ms, mem, rand_logits(2, len(origins), 1, (2, 2), True, 340), origins, tile, H, W,
                                    True, labels, exact_pred=0)
    assert counts.shape == (1, 1) and int(counts[0, 0]) == int((labels == 0).sum())


def c256_ignore_minus_one(lib, ms, mem):
    """C = 256 at a small map: the 128 KiB histogram (the kernel's dynamic LDS grant), labels 255 counted, the ignore label -1"""
    N, C, H, W, tile = 2, 256, 12, 20, (8, 8)
    origins = M.tile_grid(H, W, tile)
    assert len(origins) == 6
    logits = rand_logits(N, 6, C, (2, 2), False, 350)
    logits[:, :, 255] += 4.0                                                    # pred 255 is common
    labels = np.random.default_rng(351).integers(0, C, (N, H, W)).astype(np.int64)
    labels[:, :, :8] = 255
    labels[0, 0, :10] = -1
    _, _, counts = check_sliding("C = 256", lib, ms, mem, logits, origins, tile, H, W, False, labels, ignore_label=-1)
    assert counts[255, 255] > 0 and int(counts.sum()) == N * H * W - 10


def tiles_64_with_flip(lib, ms, mem):
    """T = T_flip = 64 (the most the origins' kernel argument holds) at tiles of 3 x 3: cover counts up to 4"""
    N, C, H, W, tile = 2, 5, 17, 17, (3, 3)
    origins = M.tile_grid(H, W, tile)
    assert len(origins) == 64
    check_sliding("64 tiles + flip", lib, ms, mem, rand_logits(N, 64, C, (2, 2), True, 360), origins, tile, H, W, True,
                  _labels(N, H, W, C, 361))


LABEL_SHAPE = (2, 9, 14, 20)                                    # N, C, H, W; six 8 x 8 tiles, flip


def _label_inputs():
    N, C, H, W = LABEL_SHAPE
    origins = M.tile_grid(H, W, (8, 8))
    assert len(origins) == 6
    return origins, rand_logits(N, 6, C, (2, 3), True, 370)


def ignore_label_inside_the_classes(lib, ms, mem):
    N, C, H, W = LABEL_SHAPE
    origins, logits = _label_inputs()
    rng = np.random.default_rng(371)
    labels = rng.integers(-300, 300, (N, H, W)).astype(np.int64)                # rows 2::3: mostly out of range
    labels[:, ::3] = 7                                                          # the ignore label, inside [0, C)
    labels[:, 1::3] = rng.integers(0, C, (N, len(range(1, H, 3)), W))
    counted = (labels != 7) & (labels >= 0) & (labels < C)
    assert (labels < 0).any() and (labels >= C).any() and counted.any()
    _, _, counts = check_sliding("ignore label 7", lib, ms, mem, logits, origins, (8, 8), H, W, True, labels, ignore_label=7)
    assert int(counts.sum()) == int(counted.sum()) and not counts[7].any()


def all_labels_ignored(lib, ms, mem):
    N, C, H, W = LABEL_SHAPE
    origins, logits = _label_inputs()
    _, _, conf = sliding_ok(lib, ms, mem, logits, origins, (8, 8), H, W, True, np.full((N, H, W), 255, np.int64))
    assert same_bits(conf, confusion_seed(C)), "the confusion buffer is not its seed"


def labels_without_confusion(lib, ms, mem):
    N, C, H, W = LABEL_SHAPE
    origins, logits = _label_inputs()
    plain = sliding_ok(lib, ms, mem, logits, origins, (8, 8), H, W, True, want=("probs", "pred"))
    with_labels = sliding_ok(lib, ms, mem, logits, origins, (8, 8), H, W, True, _labels(N, H, W, C, 372), want=("probs", "pred"))
    assert same_bits(plain[0], with_labels[0]) and same_bits(plain[1], with_labels[1]) and with_labels[2] is None


def optional_outputs_and_misplaced_buffers(lib, ms, mem):
    N, C, H, W = LABEL_SHAPE
    origins, logits = _label_inputs()
    labels = _labels(N, H, W, C, 373)
    args = (lib, ms, mem, logits, origins, (8, 8), H, W, True, labels)
    both = check_sliding("every output", *args)
    only_probs = sliding_ok(*args[:-1], want=("probs",))
    only_pred = sliding_ok(*args[:-1], want=("pred",))
    only_conf = sliding_ok(*args, want=("conf",))
    assert only_probs[1] is None and only_probs[2] is None and same_bits(only_probs[0], both[0])
    assert only_pred[0] is None and only_pred[2] is None and same_bits(only_pred[1], both[1])
    assert only_conf[0] is None and only_conf[1] is None and same_bits(only_conf[2] - confusion_seed(C), both[2])
    for k in (1, 2, 3):
        off = check_sliding(f"probs_out + {k}, pred_out at an odd byte", *args, offsets={"probs": k, "pred": 2 * k - 1})
        assert same_bits(off[0], both[0]) and same_bits(off[1], both[1]) and same_bits(off[2], both[2])


def two_calls_into_one_confusion(lib, ms, mem):
    N, C, H, W = LABEL_SHAPE
    origins, logits = _label_inputs()
    labels = _labels(N, H, W, C, 374)
    _, pred, one = check_sliding("first call", lib, ms, mem, logits, origins, (8, 8), H, W, True, labels)
    first = confusion_seed(C) + one
    other = rand_logits(N, 6, C, (2, 3), True, 375)
    _, pred2, two = check_sliding("second call", lib, ms, mem, other, origins, (8, 8), H, W, True, labels, conf_init=first)
    assert (pred != pred2).any() and int(two.sum()) == int(one.sum()) > 0      # (check_sliding: conf == first + the call's counts)


def _saturation(low_half):
    def case(lib, ms, mem):            # N = 1: every counted pixel of a workgroup, 4096, in one 16-bit counter
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
        _, _, counts = check_sliding(f"saturation cell ({l}, {a})", lib, ms, mem, logits, [(0, 0)], (H, W), H, W, False, labels,
                                     exact_pred=a)
        assert int(counts[l, a]) == n and int(counts.sum()) == n
    return case


TIES = ("all_equal", "two_at_plus_inf", "all_minus_inf")


def _ties(kind):
    def case(lib, ms, mem):
        N, C, H, W, flip, tile = 2, 4, 12, 20, True, (8, 8)
        origins = M.tile_grid(H, W, tile)
        labels = _labels(N, H, W, C, 380)
        logits = np.full((N, 2 * len(origins), C, 2, 2), 1.5, np.float32)
        if kind == "all_equal":                                   # every class the same score: the first one
            probs, _, _ = check_sliding("all logits equal", lib, ms, mem, logits, origins, tile, H, W, flip, labels, exact_pred=0)
            assert np.all(probs == probs[:, :1])
            return
        if kind == "two_at_plus_inf":                             # +inf, or NaN where a tile's sample has a weight of 0
            logits[:, :, (1, 3)] = np.inf
        else:                                                     # `c == 0 ||`: no score is > -inf
            logits[:] = -np.inf
        probs, pred, conf = sliding_ok(lib, ms, mem, logits, origins, tile, H, W, flip, labels)
        if kind == "two_at_plus_inf":
            assert np.abs(probs[:, (0, 2)] - 1.5).max() <= 1e-5 * 1.5
            assert np.all((probs[:, (1, 3)] == np.inf) | np.isnan(probs[:, (1, 3)]))
            assert np.all(np.isnan(probs[:, 1]) == np.isnan(probs[:, 3]))
            print(f"two classes at +inf: {int(np.isnan(probs[:, 1]).sum())} of {N * H * W} pixels have NaN scores")
        else:
            assert np.all((probs == -np.inf) | np.isnan(probs))
        first = 1 if kind == "two_at_plus_inf" else 0
        assert np.all(pred == first), f"{int((pred != first).sum())} of {pred.size} predictions are not {first}"
        np.testing.assert_array_equal(conf - confusion_seed(C), O.confusion(labels, pred, C))
    return case


def one_plus_inf_logit(lib, ms, mem):
    """One +inf logit in one plain tile of one image (3 x 3 logits under 9 x 9 tiles: the source index is ly / 4, exact).  Inside a
    tile the bilinear sample is PyTorch's unconditional four-term sum (ccnet_mseval.h, step 4), so the logit makes the plain
    pass non-finite at every position of its tile whose four neighbours include it -- +inf where its weight is not 0, NaN
    (0 * inf) where it is -- and at no other; the mean over the covering tiles and the other pass's half keep it non-finite.
    np.argmax takes +inf and NaN alike for the maximum: pred is that class on all of them."""
    N, C, H, W, flip, tile = 2, 5, 12, 15, True, (9, 9)
    origins = M.tile_grid(H, W, tile)
    assert origins == [(0, 0), (0, 6), (3, 0), (3, 6)]
    clean = rand_logits(N, 4, C, (3, 3), flip, 390)
    n0, t0, c0, py, px = 1, 1, 2, 1, 1
    logits = clean.copy()
    logits[n0, t0, c0, py, px] = np.inf
    y1, x1 = origins[t0]
    ya = O._axis(3, tile[0], np.arange(min(tile[0], H - y1)))
    xa = O._axis(3, tile[1], np.arange(min(tile[1], W - x1)))
    on = lambda a, p: ((a[0] == p) | (a[1] == p), ((a[0] == p) & (a[2] != 0)) | ((a[1] == p) & (a[3] != 0)))   # noqa: E731
    (ry, wy), (rx, wx) = on(ya, py), on(xa, px)
    read, weighted = np.zeros((H, W), bool), np.zeros((H, W), bool)
    read[y1:y1 + len(ry), x1:x1 + len(rx)] = ry[:, None] & rx[None, :]
    weighted[y1:y1 + len(wy), x1:x1 + len(wx)] = wy[:, None] & wx[None, :]
    assert weighted.any() and (read & ~weighted).any() and not read.all()
    labels = _labels(N, H, W, C, 391)
    probs, pred, conf = sliding_ok(lib, ms, mem, logits, origins, tile, H, W, flip, labels)
    bad = ~np.isfinite(probs)
    expect = np.zeros_like(bad)
    expect[n0, c0] = read
    print(f"one +inf logit: {int(read.sum())} positions of its tile read it, {int(weighted.sum())} with a non-zero weight; "
          f"non-finite scores {int(bad.sum())}, NaN {int(np.isnan(probs).sum())}")
    assert np.array_equal(bad, expect), "the non-finite scores are not those the header predicts"
    assert np.all(probs[n0, c0][weighted] == np.inf) and np.all(np.isnan(probs[n0, c0][read & ~weighted]))
    wrong = pred[n0][read] != c0
    assert not wrong.any(), f"{int(wrong.sum())} of {int(read.sum())} predictions on the non-finite scores are not class {c0}"
    with np.errstate(invalid="ignore"):
        assert np.array_equal(pred, O.argmax(probs)), "pred is not np.argmax of the library's own score"
    ref, bar = oracle(clean, origins, tile, H, W, flip), 1e-5 * float(np.abs(clean).max())
    compare("beside the +inf logit", probs, pred, ref, bar, ~expect.any(1))
    err = float(np.abs(probs - ref)[~expect].max())                             # and the other classes of the poisoned pixels
    _note("every finite score of the +inf case", err, bar)
    assert err <= bar
    np.testing.assert_array_equal(conf - confusion_seed(C), O.confusion(labels, pred, C))


# ---------------------------------------------------------------------------------------------------------------------
# the table: name -> case(lib, ms, mem).  The shapes are the smallest that reach each path; every case runs on both back ends.
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    # degenerate axes
    "one_row_image": _plain("H = 1", 1, 20, (8, 8), (2, 2), True, seed=1),
    "one_column_image_flip": _plain("W = 1 + flip (xf = 0)", 20, 1, (8, 8), (2, 2), True, seed=2),
    "tile_of_one_row": _plain("tile 1x8, logits 2x3 (scale 0 along H)", 3, 12, (1, 8), (2, 3), True, seed=3,
                              origins=[(0, 0), (1, 0), (2, 0), (0, 4), (1, 4), (2, 4)]),
    "tile_of_one_column": _plain("tile 8x1, logits 3x2 (scale 0 along W)", 12, 3, (8, 1), (3, 2), True, seed=4,
                                 origins=[(0, 0), (0, 1), (0, 2), (4, 0), (4, 1), (4, 2)]),
    "logits_1x1": _plain("logits 1x1", 12, 20, (8, 8), (1, 1), True, seed=5),
    "tile_larger_than_the_image": _plain("tile 7x19 on 5x6", 5, 6, (7, 19), (2, 3), True, seed=6, origins=[(0, 0)]),
    "whole_image": _plain("T = 1, tile == image", 9, 13, (9, 13), (2, 2), True, seed=7, origins=[(0, 0)]),
    # coverage
    "asymmetric_two_tiles_under_flip": asymmetric_two_tiles_under_flip,
    "uncovered_pixel": uncovered_pixel,
    # workgroup edges
    "one_past_a_workgroup": _one_past(17, 241, (17, 160), [(0, 0), (0, 81)], True),
    "one_past_a_thread_row": _one_past(257, 16, (160, 16), [(0, 0), (97, 0)], False),
    "fewer_pixels_than_threads": _plain("7x11 < 256 pixels", 7, 11, (5, 8), (2, 2), False, seed=8,
                                        origins=[(0, 0), (0, 3), (2, 0), (2, 3)]),
    # classes
    "one_class": one_class,
    "odd_class_count": _plain("C = 7", 12, 20, (8, 8), (2, 2), True, C=7, seed=9),
    "c256_ignore_minus_one": c256_ignore_minus_one,
    # tiles
    "tiles_64_with_flip": tiles_64_with_flip,
    # labels
    "ignore_label_inside_the_classes": ignore_label_inside_the_classes,
    "all_labels_ignored": all_labels_ignored,
    "labels_without_confusion": labels_without_confusion,
    # outputs, accumulation, saturation
    "optional_outputs_and_misplaced_buffers": optional_outputs_and_misplaced_buffers,
    "two_calls_into_one_confusion": two_calls_into_one_confusion,
    "saturation_low_half": _saturation(True),
    "saturation_high_half": _saturation(False),
}
CASES.update({f"ties_{_k}": _ties(_k) for _k in TIES})
CASES["one_plus_inf_logit"] = one_plus_inf_logit
ALL = list(CASES)
NAN_CASES = ("ties_two_at_plus_inf", "one_plus_inf_logit")       # what `s > best` alone gets wrong: it skips a NaN score


def run_case(name, lib, ms, mem):
    CASES[name](lib, ms, mem)
