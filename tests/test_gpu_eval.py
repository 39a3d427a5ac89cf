"""Sliding-window evaluation on the MI355X (libccnet_eval.so through ccnet_amd.evaluate) against the reference fixtures and
the numpy oracle: score map, prediction, confusion counts; flip, batches, bf16 net output, small images; a real Seg_Model
against stock torch; repeatability; no host sync; the eval_synthetic driver on one and two ranks."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_cases as EC
import eval_oracle as O
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz")))
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def device_call(tiles, origins, tile, H, W, flip=False, label=None, probs=True):
    from ccnet_amd.evaluate import sliding_call
    t = torch.from_numpy(np.ascontiguousarray(tiles)).to(DEV).flatten(0, 1) if isinstance(tiles, np.ndarray) else tiles
    N = t.shape[0] // (len(origins) * (2 if flip else 1))
    C = t.shape[1]
    p = torch.full((N, C, H, W), float("nan"), device=DEV) if probs else None
    pred = torch.full((N, H, W), 0xEE, dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    lab = None if label is None else torch.from_numpy(label).to(DEV)
    sliding_call(t, origins, flip, N, tile, H, W, labels=lab, probs=p, pred=pred, confusion=conf if lab is not None else None)
    torch.cuda.synchronize()
    return (None if p is None else p.cpu().numpy()), pred.cpu().numpy(), conf.cpu().numpy()


def _origins(fx):
    return [(0, 0)] if fx["whole"] else O.reference_tile_grid(int(fx["H"]), int(fx["W"]), fx["tile"])


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_parity(path):
    fx = O.load_fixture(path)
    origins = _origins(fx)
    probs, pred, conf = device_call(O.fixture_tiles(fx, origins), origins, fx["tile"], int(fx["H"]), int(fx["W"]),
                                    label=fx["label"])
    n = O.check_against_fixture(fx, probs, pred, conf)
    print(f"{os.path.basename(path)}: near-tie pixels with a different prediction: {n}")


def _check_vs_oracle(tiles, origins, tile, H, W, flip, label, probs, pred, conf, ignore_label=255):
    ref = O.sliding_scores(tiles, origins, tile, H, W, flip)
    tol = 1e-5 * float(np.abs(tiles).max())
    assert np.abs(probs - ref).max() <= tol
    diff = pred != O.argmax(ref)
    assert np.all(O.top2_gap(ref)[diff] < tol)
    np.testing.assert_array_equal(conf, O.confusion(label, pred, tiles.shape[2], ignore_label))
    return int(diff.sum())


@pytest.mark.parametrize("N,H,W,tile,C,flip", [
    (1, 300, 500, 97, 19, True),         # flip
    (3, 200, 330, 97, 19, False),        # every image its own tiles
    (2, 40, 50, 97, 19, True),           # image smaller than the tile
    (1, 257, 513, 129, 150, False),      # ADE20K's class count
    (1, 120, 160, 97, 256, False),       # the largest C: 128 KiB histogram
])
def test_against_oracle(N, H, W, tile, C, flip):
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(H, W, (tile, tile))
    rng = np.random.default_rng(N * H + W + C)
    h = (tile + 7) // 8
    tiles = (rng.standard_normal((N, len(origins) * (2 if flip else 1), C, h, h)) * 3).astype(np.float32)
    _, label = O.make_case_inputs(N, H, W, C, seed=H + W)
    probs, pred, conf = device_call(tiles, origins, (tile, tile), H, W, flip, label)
    _check_vs_oracle(tiles, origins, (tile, tile), H, W, flip, label, probs, pred, conf)


def _random_tiles(N, T, C, h, w, seed):
    return (np.random.default_rng(seed).standard_normal((N, T, C, h, w)) * 3).astype(np.float32)


def test_exactly_64_tiles_with_flip():
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(552, 552, (97, 97))
    assert len(origins) == 64                                                   # kMaxTiles
    tiles = _random_tiles(1, 128, 19, 13, 13, seed=81)
    _, label = O.make_case_inputs(1, 552, 552, 19, seed=81)
    out = device_call(tiles, origins, (97, 97), 552, 552, True, label)
    n = _check_vs_oracle(tiles, origins, (97, 97), 552, 552, True, label, *out)
    print(f"64 tiles + flip: near-tie prediction differences {n}")


def _saturation_case(low_half, C=19):
    """111 x 111 = 12 321 >= 3 x 4096 + 17 pixels, all predicted `a` and labelled `l` (cell l * C + a even: the low 16 bits
    of its LDS word; odd: the high 16 bits), plus a few ignored and out-of-range labels that are not counted."""
    l, a = (2, 4) if low_half else (2, 5)
    assert ((l * C + a) % 2 == 0) == low_half
    tiles = np.zeros((1, 1, C, 14, 14), np.float32)
    tiles[:, :, a] = 10.0
    label = np.full((1, 111, 111), l, np.int64)
    label[0, 5, 7:11] = 255
    label[0, 90, 3] = C
    return tiles, label, l, a, int((label == l).sum())


@pytest.mark.parametrize("low_half", [True, False], ids=["low_half", "high_half"])
def test_single_cell_counter_saturation(low_half):
    tiles, label, l, a, n = _saturation_case(low_half)
    _, pred, conf = device_call(tiles, [(0, 0)], (111, 111), 111, 111, label=label)
    assert np.all(pred == a) and n >= 3 * 4096 + 17
    assert int(conf[l, a]) == n and int(conf.sum()) == n


def test_c256_with_ignore_label_outside_the_classes():
    from ccnet_amd.evaluate import sliding_call, tile_grid
    H, W, C = 120, 150, 256
    origins = tile_grid(H, W, (97, 97))
    tiles = _random_tiles(1, len(origins), C, 13, 13, seed=83)
    tiles[:, :, 255] += 4.0                                                     # pred 255 is common
    label = np.random.default_rng(84).integers(0, C, (1, H, W)).astype(np.int64)
    label[:, :, :40] = 255
    label[0, 0, :10] = -1                                                       # the ignore label
    t = torch.from_numpy(tiles).to(DEV).flatten(0, 1)
    pred = torch.empty((1, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    probs = torch.empty((1, C, H, W), device=DEV)
    sliding_call(t, origins, False, 1, (97, 97), H, W, labels=torch.from_numpy(label).to(DEV), ignore_label=-1,
                 probs=probs, pred=pred, confusion=conf)
    torch.cuda.synchronize()
    pred, conf = pred.cpu().numpy(), conf.cpu().numpy()
    _check_vs_oracle(tiles, origins, (97, 97), H, W, False, label, probs.cpu().numpy(), pred, conf, ignore_label=-1)
    assert conf[255, 255] > 0 and conf[255].sum() >= 40 * H - 10 and int(conf.sum()) == H * W - 10


def test_ignore_label_inside_the_classes_and_out_of_range_labels():
    from ccnet_amd.evaluate import sliding_call, tile_grid
    H, W, C = 130, 170, 19
    origins = tile_grid(H, W, (97, 97))
    tiles = _random_tiles(2, len(origins), C, 13, 13, seed=85)
    rng = np.random.default_rng(86)
    label = rng.integers(-300, 300, (2, H, W)).astype(np.int64)                 # rows 2::3: mostly out of range
    label[:, ::3] = 7                                                           # the ignore label, inside [0, C)
    label[:, 1::3] = rng.integers(0, C, (2, len(range(1, H, 3)), W))
    t = torch.from_numpy(tiles).to(DEV).flatten(0, 1)
    pred = torch.empty((2, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    sliding_call(t, origins, False, 2, (97, 97), H, W, labels=torch.from_numpy(label).to(DEV), ignore_label=7, pred=pred,
                 confusion=conf)
    torch.cuda.synchronize()
    pred, conf = pred.cpu().numpy(), conf.cpu().numpy()
    counted = (label != 7) & (label >= 0) & (label < C)
    assert (label < 0).any() and (label >= C).any() and counted.any()
    np.testing.assert_array_equal(conf, O.confusion(label, pred, C, ignore_label=7))
    assert int(conf.sum()) == int(counted.sum()) and not conf[7].any()


def test_confusion_accumulates_over_two_device_calls():
    from ccnet_amd.evaluate import sliding_call, tile_grid
    H, W, C = 200, 260, 19
    origins = tile_grid(H, W, (97, 97))
    tiles = _random_tiles(1, 2 * len(origins), C, 13, 13, seed=87)
    _, label = O.make_case_inputs(1, H, W, C, seed=87)
    t = torch.from_numpy(tiles).to(DEV).flatten(0, 1)
    lab = torch.from_numpy(label).to(DEV)
    pred = torch.empty((1, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    sliding_call(t, origins, True, 1, (97, 97), H, W, labels=lab, pred=pred, confusion=conf)
    one = conf.clone()
    sliding_call(t, origins, True, 1, (97, 97), H, W, labels=lab, pred=pred, confusion=conf)
    torch.cuda.synchronize()
    ref = O.confusion(label, pred.cpu().numpy(), C)
    np.testing.assert_array_equal(one.cpu().numpy(), ref)
    np.testing.assert_array_equal(conf.cpu().numpy(), 2 * ref)


@pytest.mark.parametrize("H,W,tile,hw,flip", [
    (40, 56, (8, 8), (1, 1), True),             # 1 x 1 logits: up-sampling scale 0, every tile a constant
    (300, 420, (97, 129), (13, 17), True),      # non-square tile
    (300, 60, (97, 97), (13, 13), True),        # narrower than the tile along W only
    (50, 400, (97, 97), (13, 13), False),       # shorter than the tile along H only
], ids=["logits_1x1", "nonsquare_tile", "narrow_w", "short_h"])
def test_degenerate_geometry(H, W, tile, hw, flip):
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(H, W, tile)
    tiles = _random_tiles(2, len(origins) * (2 if flip else 1), 19, hw[0], hw[1], seed=H + W)
    _, label = O.make_case_inputs(2, H, W, 19, seed=H * W)
    out = device_call(tiles, origins, tile, H, W, flip, label)
    _check_vs_oracle(tiles, origins, tile, H, W, flip, label, *out)


def test_evaluator_bf16_net_output_and_predict_apis():
    from ccnet_amd import SegEvaluator, predict_sliding, predict_whole
    from ccnet_amd.evaluate import tile_grid
    net = O.make_toy_net(19, 3).to(DEV)
    bf = lambda x: [y.to(torch.bfloat16) for y in net(x)]                     # noqa: E731
    _, label = O.make_case_inputs(1, 150, 260, 19, seed=3)
    image = torch.from_numpy(O.make_case_inputs(1, 150, 260, 19, seed=3)[0]).to(DEV)
    lab = torch.from_numpy(label).to(DEV)
    for flip in (False, True):
        ev = SegEvaluator(19, tile_size=(97, 97), flip=flip)
        logits = ev.net_logits(bf, image)
        assert logits.dtype == torch.float32
        pred = ev.update(bf, image, lab)
        origins = tile_grid(150, 260, (97, 97))
        tiles = logits.cpu().numpy().reshape(1, -1, 19, 13, 13)
        ref = O.sliding_scores(tiles, origins, (97, 97), 150, 260, flip)
        diff = pred.cpu().numpy() != O.argmax(ref)
        assert np.all(O.top2_gap(ref)[diff] < 1e-5 * np.abs(tiles).max())
        np.testing.assert_array_equal(ev.confusion.cpu().numpy(), O.confusion(label, pred.cpu().numpy(), 19))
        r = ev.result()
        assert 0.0 <= r["meanIU"] <= 1.0 and r["IU_array"].shape == (19,)
        probs = predict_sliding(net, image, (97, 97), 19, flip=flip)
        assert probs.shape == (1, 19, 150, 260) and torch.equal(probs.argmax(1).to(torch.uint8).cpu(),
                                                                torch.from_numpy(O.argmax(probs.cpu().numpy())))
    whole = predict_whole(net, image)
    ref = F.interpolate(net(image)[0], size=(150, 260), mode="bilinear", align_corners=True)
    assert (whole - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_seg_model_evaluator_against_stock_torch():
    from ccnet_amd import SegEvaluator
    from ccnet_amd.evaluate import tile_grid
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    image = torch.randn(1, 3, 1024, 2048, device=DEV, generator=g)
    label = torch.randint(0, 19, (1, 1024, 2048), device=DEV, generator=g)
    label[torch.rand(1, 1024, 2048, device=DEV, generator=g) < 0.05] = 255
    ev = SegEvaluator(19)
    logits = ev.net_logits(model, image)
    assert logits.shape == (8, 19, 97, 97)
    pred = ev.accumulate(logits, label, 1024, 2048)
    # stock torch on the device: F.interpolate per tile, crop, accumulate, divide, argmax, bincount
    full = torch.zeros(1, 19, 1024, 2048, device=DEV)
    count = torch.zeros(1, 1, 1024, 2048, device=DEV)
    for t, (y1, x1) in enumerate(tile_grid(1024, 2048, (769, 769))):
        up = F.interpolate(logits[t:t + 1], size=(769, 769), mode="bilinear", align_corners=True)
        y2, x2 = min(y1 + 769, 1024), min(x1 + 769, 2048)
        full[:, :, y1:y2, x1:x2] += up[:, :, :y2 - y1, :x2 - x1]
        count[:, :, y1:y2, x1:x2] += 1
    full /= count
    stock = full.argmax(1).to(torch.uint8)
    top2 = full.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 1e-5 * logits.abs().max()
    diff = pred != stock
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    keep = (label != 255)
    ref_cm = torch.bincount((label[keep] * 19 + stock[keep].long()), minlength=361).reshape(19, 19)
    n = int(diff.sum())
    d = (ev.confusion - ref_cm).abs()
    assert int(d.sum()) <= 2 * n and int(d.max()) <= n, (int(d.sum()), n)
    print(f"Seg_Model 1024x2048: pixels whose prediction differs at a near tie: {n}")


def test_bitwise_repeatable():
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(700, 900, (257, 257))
    rng = np.random.default_rng(5)
    tiles = (rng.standard_normal((1, 2 * len(origins), 19, 33, 33)) * 3).astype(np.float32)
    _, label = O.make_case_inputs(1, 700, 900, 19, seed=5)
    a = device_call(tiles, origins, (257, 257), 700, 900, True, label)
    b = device_call(tiles, origins, (257, 257), 700, 900, True, label)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_no_host_sync_in_the_post_processing():
    from ccnet_amd import SegEvaluator
    net = O.make_toy_net(19, 4).to(DEV)
    image = torch.randn(1, 3, 300, 400, device=DEV)
    label = torch.randint(0, 19, (1, 300, 400), device=DEV)
    ev = SegEvaluator(19, tile_size=(97, 97), flip=True)
    logits = ev.net_logits(net, image)
    ev.accumulate(logits, label, 300, 400)                      # warm: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred = ev.accumulate(logits, label, 300, 400)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert pred.shape == (1, 300, 400) and int(ev.confusion.sum()) == 2 * 300 * 400


# ---------------------------------------------------------------------------------------------------------------------
# the library at its limits, over the C ABI on guarded device buffers (tests/eval_cases.py; the emulator runs the same table).
# Every call is repeated through libccnet_mseval.so at Hs = H, Ws = W: the same bits, predictions and counts.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guarded():
    from ccnet_amd import _eval_lib, _mseval_lib
    yield _eval_lib.get_lib(), _mseval_lib.get_lib(), EC.DeviceMemory()
    print("largest error / bar on the device:", {k: round(v, 4) for k, v in EC.WORST.items()})


@pytest.mark.parametrize("name", EC.ALL)
def test_limits_on_guarded_buffers(guarded, name):
    EC.run_case(name, *guarded)


# ---------------------------------------------------------------------------------------------------------------------
# sliding_call hands raw pointers to a kernel that indexes them by the shapes it is told: it refuses every other tensor
# ---------------------------------------------------------------------------------------------------------------------
def _validation_inputs():
    from ccnet_amd.evaluate import tile_grid
    N, C, H, W, tile = 2, 5, 12, 20, (8, 8)
    origins = tile_grid(H, W, tile)
    logits = torch.from_numpy(EC.rand_logits(N, len(origins), C, (2, 2), False, 500)).to(DEV).flatten(0, 1)
    labels = torch.from_numpy(O.make_case_inputs(N, H, W, C, seed=501)[1]).to(DEV)
    return N, C, H, W, tile, origins, logits, labels


def test_sliding_call_refuses_tensors_the_kernel_would_misread():
    from ccnet_amd.evaluate import sliding_call
    N, C, H, W, tile, origins, logits, labels = _validation_inputs()
    probs = torch.full((N, C, H, W), float("nan"), device=DEV)
    pred = torch.full((N, H, W), 0xEE, dtype=torch.uint8, device=DEV)
    conf = torch.full((C, C), 7, dtype=torch.int64, device=DEV)
    wide = torch.full((N, H, W + 4), 0xEE, dtype=torch.uint8, device=DEV)
    last = torch.full((N, C, H, W), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    flat = torch.full((C * C,), 7, dtype=torch.int64, device=DEV)
    assert not last.is_contiguous() and not wide[:, :, :W].is_contiguous() and logits[:-1].is_contiguous()
    call = lambda lg=logits, **kw: sliding_call(lg, origins, False, N, tile, H, W, **kw)           # noqa: E731
    for match, kw in (
            ("probs must be a contiguous", dict(probs=last)),                                      # channels_last
            ("pred must be a contiguous", dict(pred=wide[:, :, :W])),                              # a column slice
            ("labels must be a contiguous torch.int64", dict(labels=labels.to(torch.int32), pred=pred, confusion=conf)),
            ("logits must be a contiguous", dict(lg=logits[:-1], probs=probs, pred=pred)),         # one tile short
            ("logits must be a contiguous", dict(lg=logits.to(torch.float64), probs=probs)),
            ("confusion must be a contiguous", dict(labels=labels, pred=pred, confusion=flat)),    # C * C, but not (C, C)
            ("pred must be a contiguous", dict(pred=pred.to(torch.int64))),
            ("probs must be a contiguous", dict(probs=probs[:1])),
            ("confusion needs labels", dict(pred=pred, confusion=conf))):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its prefill
    assert torch.isnan(probs).all() and torch.isnan(last).all()
    assert (pred == 0xEE).all() and (wide == 0xEE).all() and (conf == 7).all() and (flat == 7).all()
    call(labels=labels, probs=probs, pred=pred, confusion=conf)                                    # the well-formed call passes
    torch.cuda.synchronize()
    assert not torch.isnan(probs).any() and (pred < C).all()
    assert int((conf - 7).sum()) == int(((labels >= 0) & (labels < C)).sum())


def test_evaluator_accumulate_refuses_strided_logits():
    """SegEvaluator.accumulate is public and reaches the kernel with the caller's logits: channels_last or sliced ones raise (as
    in MultiScaleEvaluator) instead of being read through the wrong strides, and the counts stay as they were"""
    from ccnet_amd import SegEvaluator
    N, C, H, W, tile, origins, logits, labels = _validation_inputs()
    ev = SegEvaluator(C, tile_size=tile)
    want = ev.accumulate(logits, labels, H, W)
    counts = ev.confusion.clone()
    padded = torch.zeros((logits.shape[0], C, 2, 3), device=DEV)
    padded[..., :2] = logits
    for strided in (logits.contiguous(memory_format=torch.channels_last), padded[..., :2]):
        assert torch.equal(strided, logits) and not strided.is_contiguous()
        with pytest.raises(RuntimeError, match="logits must be a contiguous"):
            ev.accumulate(strided, labels, H, W)
    with pytest.raises(RuntimeError, match="labels must be a contiguous"):
        ev.accumulate(logits, labels[:, :, :W - 1], H, W)
    torch.cuda.synchronize()
    assert torch.equal(ev.confusion, counts)
    assert torch.equal(ev.accumulate(logits.clone(), labels.to(torch.int32), H, W), want)         # labels are converted, as before
    assert torch.equal(ev.confusion, 2 * counts)


DRIVER = ["-m", "ccnet_amd.eval_synthetic", "--images", "4", "--height", "256", "--width", "512", "--tile", "193",
          "--flip"]


def _driver(prefix, tmp_path, name):
    dump = str(tmp_path / f"{name}.pt")
    r = subprocess.run([sys.executable] + prefix + DRIVER + ["--dump-confusion", dump], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return res, torch.load(dump)


def test_eval_synthetic_one_and_two_ranks(tmp_path):
    one, cm1 = _driver([], tmp_path, "one")
    assert one["n_gpus"] == 1 and one["counted_pixels"] == int(cm1.sum()) > 0 and one["route"], one
    from ccnet_amd.evaluate import tile_grid
    assert one["config"]["tiles"] == len(tile_grid(256, 512, (193, 193))) and 0.0 <= one["meanIU"] <= 1.0
    two, cm2 = _driver(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29517"], tmp_path, "two")
    assert two["n_gpus"] == 2, two
    assert torch.equal(cm1, cm2) and two["meanIU"] == one["meanIU"]
