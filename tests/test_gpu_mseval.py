"""Multi-scale evaluation on the MI355X (libccnet_mseval.so through ccnet_amd.evaluate) against the numpy oracle, the reference +
scipy fixtures, the single-scale kernel (bit for bit at scales = (1.0,)) and a stock-torch chain on the device: the gather
kernel (zoom + flip + cut + pad), the per-scale accumulate kernel, in-place accumulation, MultiScaleEvaluator, a real net."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_oracle as O
import mseval_cases as MC
import mseval_oracle as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mseval_*.npz")))
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_tiles(image, geo, flip, first=0, count=None):
    """(N, count, Cin, th, tw) numpy from one gather launch into a NaN-filled buffer."""
    from ccnet_amd.evaluate import scaled_tiles_call
    Hs, Ws, origins, tile = geo
    count = len(origins) * (2 if flip else 1) - first if count is None else count
    out = torch.full((image.shape[0], count, image.shape[1], tile[0], tile[1]), float("nan"), device=DEV)
    scaled_tiles_call(image, Hs, Ws, origins, tile, flip, first, count, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_multiscale(logits, geo, H, W, flip, label=None, confusion=None, ignore_label=255):
    """The chain of accumulate launches over the scales, out of place: (score, pred, confusion) as numpy."""
    from ccnet_amd.evaluate import accumulate_call
    N, C = logits[0].shape[0], logits[0].shape[2]
    lab = None if label is None else dev(label)
    pred = torch.full((N, H, W), 0xEE, dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV) if confusion is None else confusion
    score = None
    for i, (lg, (Hs, Ws, origins, tile)) in enumerate(zip(logits, geo)):
        last = i == len(geo) - 1
        out = torch.full((N, C, H, W), float("nan"), device=DEV)
        accumulate_call(dev(lg).flatten(0, 1), origins, flip, N, tile, Hs, Ws, H, W, score_in=score, score_out=out,
                        divide_by=len(geo) if last else 0, labels=lab if last else None, ignore_label=ignore_label,
                        pred=pred if last else None, confusion=conf if last and lab is not None else None)
        score = out
    torch.cuda.synchronize()
    return score.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy()


def random_logits(geo, N, C, flip, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((N, len(g[2]) * (2 if flip else 1), C, (g[3][0] + 7) // 8, (g[3][1] + 7) // 8)) * 3)
            .astype(np.float32) for g in geo]


# ---------------------------------------------------------------------------------------------------------------------
# the gather kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,tile,flip", [(s, tile, flip) for s in (0.5, 0.75, 1.5, 2.0) for tile in (33, None)
                                         for flip in (False, True)])
def test_tiles_kernel_against_oracle_and_in_chunks(s, tile, flip):
    image, _ = O.make_case_inputs(2, 60, 80, 19, seed=21)
    geo = M.geometry(60, 80, s, (tile, tile), tile is None)
    img = dev(image)
    got = device_tiles(img, geo, flip)
    ref = M.zoom_tiles(image, *geo, flip)
    err = float(np.abs(got - ref).max())                                      # (NaN where an element was not written)
    print(f"tiles s={s} tile={geo[3]} flip={flip}: max err {err:.3e}, bar {1e-6 * np.abs(image).max():.3e}")
    assert got.shape == ref.shape and err <= 1e-6 * np.abs(image).max()
    parts = [device_tiles(img, geo, flip, first, min(3, got.shape[1] - first)) for first in range(0, got.shape[1], 3)]
    assert np.array_equal(np.concatenate(parts, 1), got)


def test_tiles_at_scale_one_are_cut_tiles_bit_for_bit():
    from ccnet_amd.evaluate import cut_tiles
    image, _ = O.make_case_inputs(2, 60, 80, 19, seed=22)
    img = dev(image)
    for tile, whole in (((33, 33), False), (None, True)):
        geo = M.geometry(60, 80, 1.0, tile, whole)
        got = device_tiles(img, geo, True)
        want = cut_tiles(img, geo[2], geo[3], True).cpu().numpy().reshape(got.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the accumulate kernel
# ---------------------------------------------------------------------------------------------------------------------
def _check_vs_oracle(logits, geo, H, W, flip, label, score, pred, conf):
    ref = M.multiscale_scores(logits, geo, H, W, flip)
    tol = 1e-5 * max(float(np.abs(lg).max()) for lg in logits)
    err = float(np.abs(score - ref).max())
    diff = pred != O.argmax(ref)
    print(f"score err {err:.3e} (bar {tol:.3e}), near-tie prediction differences {int(diff.sum())}")
    assert err <= tol
    assert np.all(O.top2_gap(ref)[diff] < tol)
    np.testing.assert_array_equal(conf, O.confusion(label, pred, logits[0].shape[2]))


@pytest.mark.parametrize("N,H,W,tile,C,scales,flip", [
    (1, 60, 80, 33, 19, (0.5,), False),
    (1, 60, 80, 33, 19, (0.75,), True),
    (1, 60, 80, 33, 19, (1.5,), False),
    (2, 60, 80, 33, 19, (2.0,), True),                   # every image its own tiles
    (1, 97, 131, 65, 7, (0.5, 1.0, 2.0), True),          # 24 tiles at scale 2, odd C
    (1, 200, 300, 97, 150, (0.75, 1.25), False),         # ADE20K's class count: the 45 000 B histogram
])
def test_accumulate_against_oracle(N, H, W, tile, C, scales, flip):
    geo = [M.geometry(H, W, s, (tile, tile), False) for s in scales]
    if (H, W) == (97, 131):
        assert len(geo[2][2]) == 24
    logits = random_logits(geo, N, C, flip, seed=H * W + C + len(scales))
    _, label = O.make_case_inputs(N, H, W, C, seed=H + W)
    _check_vs_oracle(logits, geo, H, W, flip, label, *device_multiscale(logits, geo, H, W, flip, label))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_parity(path):
    from ccnet_amd import MultiScaleEvaluator, predict_multiscale
    fx = M.load_fixture(path)
    net = fx["net"].to(DEV)
    image, label = dev(fx["image"]), dev(fx["label"])
    score = predict_multiscale(net, image, fx["tile"], fx["scales"], fx["C"], flip_evaluation=fx["flip"], whole=fx["whole"])
    ev = MultiScaleEvaluator(fx["C"], scales=fx["scales"], tile_size=fx["tile"], whole=fx["whole"], flip=fx["flip"])
    pred = ev.update(net, image, label)
    torch.cuda.synchronize()
    n = M.check_against_fixture(fx, score.cpu().numpy(), pred.cpu().numpy(), ev.confusion.cpu().numpy())
    print(f"{os.path.basename(path)}: near-tie pixels with a different prediction: {n}")


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_scale_one_is_the_single_scale_kernel_bit_for_bit(flip):
    from ccnet_amd.evaluate import sliding_call
    N, H, W, C, tile = 2, 150, 260, 19, (97, 97)
    geo = M.geometry(H, W, 1.0, tile, False)
    logits = random_logits([geo], N, C, flip, seed=31)
    _, label = O.make_case_inputs(N, H, W, C, seed=31)
    score, pred, conf = device_multiscale(logits, [geo], H, W, flip, label)
    probs = torch.full((N, C, H, W), float("nan"), device=DEV)
    pred1 = torch.empty((N, H, W), dtype=torch.uint8, device=DEV)
    conf1 = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    sliding_call(dev(logits[0]).flatten(0, 1), geo[2], flip, N, tile, H, W, labels=dev(label), probs=probs, pred=pred1,
                 confusion=conf1)
    torch.cuda.synchronize()
    assert np.array_equal(score.view(np.uint32), probs.cpu().numpy().view(np.uint32))
    assert np.array_equal(pred, pred1.cpu().numpy()) and np.array_equal(conf, conf1.cpu().numpy())


def test_in_place_accumulation_divide_by_and_repeatability():
    from ccnet_amd.evaluate import accumulate_call
    N, H, W, C, flip = 1, 150, 200, 19, True
    geo = [M.geometry(H, W, s, (97, 97), False) for s in (0.75, 1.25)]
    logits = [dev(lg).flatten(0, 1) for lg in random_logits(geo, N, C, flip, seed=41)]
    _, label = O.make_case_inputs(N, H, W, C, seed=41)
    lab = dev(label)

    def chain(in_place, divide_by, conf):
        buf = torch.full((N, C, H, W), float("nan"), device=DEV)
        accumulate_call(logits[0], geo[0][2], flip, N, geo[0][3], geo[0][0], geo[0][1], H, W, score_out=buf)
        out = buf if in_place else torch.full((N, C, H, W), float("nan"), device=DEV)
        pred = torch.empty((N, H, W), dtype=torch.uint8, device=DEV)
        accumulate_call(logits[1], geo[1][2], flip, N, geo[1][3], geo[1][0], geo[1][1], H, W, score_in=buf, score_out=out,
                        divide_by=divide_by, labels=lab, pred=pred, confusion=conf)
        torch.cuda.synchronize()
        return out.cpu().numpy(), pred.cpu().numpy()

    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    out, pred = chain(False, 2, conf)
    one = conf.clone()
    inp, pred_inp = chain(True, 2, conf)                                        # score_out == score_in
    assert np.array_equal(out.view(np.uint32), inp.view(np.uint32)) and np.array_equal(pred, pred_inp)
    np.testing.assert_array_equal(one.cpu().numpy(), O.confusion(label, pred, C))
    np.testing.assert_array_equal(conf.cpu().numpy(), 2 * one.cpu().numpy())    # accumulated over the two calls
    undivided, _ = chain(True, 0, None)
    assert np.array_equal(out, undivided / np.float32(2)) and not np.array_equal(out, undivided)
    again, pred_again = chain(False, 2, None)                                   # two runs are bit-identical
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)) and np.array_equal(pred, pred_again)


# ---------------------------------------------------------------------------------------------------------------------
# the public layer
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluator_is_the_chain_of_the_two_entry_points_and_tile_batch_does_not_matter():
    from ccnet_amd import MultiScaleEvaluator
    from ccnet_amd.evaluate import accumulate_call
    H, W, C, scales = 128, 256, 19, (0.75, 1.0, 1.5)
    net = O.make_toy_net(C, 7).to(DEV)
    image_np, label_np = O.make_case_inputs(1, H, W, C, seed=7)
    image, label = dev(image_np), dev(label_np)
    ev = MultiScaleEvaluator(C, scales=scales, tile_size=(97, 97), flip=True, tile_batch=8)
    logits = ev.net_logits(net, image)
    pred = ev.accumulate(logits, label, H, W)
    # the manual chain on the evaluator's own logits
    score = torch.empty((1, C, H, W), device=DEV)
    pred2 = torch.empty((1, H, W), dtype=torch.uint8, device=DEV)
    conf2 = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    geo = ev.geometry(H, W)
    assert geo == [M.geometry(H, W, s, (97, 97), False) for s in scales]
    for i, (lg, (Hs, Ws, origins, tile)) in enumerate(zip(logits, geo)):
        last = i == len(geo) - 1
        accumulate_call(lg, origins, True, 1, tile, Hs, Ws, H, W, score_in=score if i else None, score_out=score,
                        divide_by=3 if last else 0, labels=label if last else None, pred=pred2 if last else None,
                        confusion=conf2 if last else None)
    torch.cuda.synchronize()
    assert torch.equal(pred, pred2) and torch.equal(ev.confusion, conf2)
    assert torch.equal(score.argmax(1).to(torch.uint8), pred)
    r = ev.result()
    assert 0.0 <= r["meanIU"] <= 1.0 and r["IU_array"].shape == (C,)
    # the logits are the net over the gather kernel's tiles, and the whole thing is the oracle's multi-scale score
    np_logits = [lg.cpu().numpy().reshape(1, -1, C, lg.shape[2], lg.shape[3]) for lg in logits]
    ref = M.multiscale_scores(np_logits, geo, H, W, True)
    tol = 1e-5 * max(float(np.abs(lg).max()) for lg in np_logits)
    assert np.abs(score.cpu().numpy() - ref).max() <= tol
    # one tile per net call
    ev1 = MultiScaleEvaluator(C, scales=scales, tile_size=(97, 97), flip=True, tile_batch=1)
    logits1 = ev1.net_logits(net, image)
    pred1 = ev1.accumulate(logits1, label, H, W)
    np_logits1 = [lg.cpu().numpy().reshape(1, -1, C, lg.shape[2], lg.shape[3]) for lg in logits1]
    ref1 = M.multiscale_scores(np_logits1, geo, H, W, True)
    assert np.abs(ref1 - ref).max() <= tol
    diff = (pred1 != pred).cpu().numpy()
    assert np.all(O.top2_gap(ref)[diff] < tol)
    ev.reset()
    assert int(ev.confusion.sum()) == 0


def test_tile_batch_that_cuts_a_chunk_across_the_plain_and_flipped_tiles():
    """scale 0.75 of 128 x 256 has T + T_flip = 2 * 3 entries: tile_batch = 5 asks for [0, 5), which starts in the plain tiles and
    ends in the flipped ones, and leaves [5, 6)"""
    from ccnet_amd import MultiScaleEvaluator
    H, W, C, scales = 128, 256, 19, (0.75, 1.0, 1.5)
    net = O.make_toy_net(C, 7).to(DEV)
    image_np, label_np = O.make_case_inputs(1, H, W, C, seed=7)
    image, label = dev(image_np), dev(label_np)
    out = {}
    for tile_batch in (8, 5):
        ev = MultiScaleEvaluator(C, scales=scales, tile_size=(97, 97), flip=True, tile_batch=tile_batch)
        geo = ev.geometry(H, W)
        assert 2 * len(geo[0][2]) == 6
        logits = ev.net_logits(net, image)
        pred = ev.accumulate(logits, label, H, W)
        torch.cuda.synchronize()
        np_logits = [lg.cpu().numpy().reshape(1, -1, C, lg.shape[2], lg.shape[3]) for lg in logits]
        out[tile_batch] = np_logits, M.multiscale_scores(np_logits, geo, H, W, True), pred.cpu().numpy()
    tol = 1e-5 * max(float(np.abs(lg).max()) for lg in out[8][0])
    err = max(float(np.abs(a - b).max()) for a, b in zip(out[5][0], out[8][0]))
    diff = out[5][2] != out[8][2]
    print(f"tile_batch 5 against 8: logits differ by {err:.3e} (bar {tol:.3e}), predictions at {int(diff.sum())} pixels")
    assert err <= tol and np.abs(out[5][1] - out[8][1]).max() <= tol
    assert np.all(O.top2_gap(out[8][1])[diff] < tol)


def test_argument_validation_of_the_two_calls_raises():
    from ccnet_amd.evaluate import accumulate_call, scaled_tiles_call
    N, C, H, W = 1, 5, 30, 40
    Hs, Ws, origins, tile = M.geometry(H, W, 0.5, (33, 33), False)
    logits = torch.zeros((N * len(origins), C, 5, 5), device=DEV)
    call = lambda **kw: accumulate_call(logits, origins, False, N, tile, Hs, Ws, H, W, **kw)       # noqa: E731
    call(score_out=torch.empty((N, C, H, W), device=DEV))                                          # the well-formed call passes
    with pytest.raises(RuntimeError, match="score_out must be a contiguous"):
        call(score_out=torch.empty((N, C, W, H), device=DEV).transpose(2, 3))                      # the right shape, strided
    with pytest.raises(RuntimeError, match="labels must be a contiguous torch.int64"):
        call(labels=torch.zeros((N, H, W), dtype=torch.int32, device=DEV), pred=torch.empty((N, H, W), dtype=torch.uint8,
                                                                                             device=DEV))
    with pytest.raises(RuntimeError, match="score_out must be a contiguous"):
        call(score_out=torch.empty((N, C, H, W + 1), device=DEV))
    with pytest.raises(RuntimeError, match="pred must be a contiguous"):
        call(pred=torch.empty((N, H, W), dtype=torch.int64, device=DEV))
    image = torch.zeros((N, 3, H, W), device=DEV)
    scaled_tiles_call(image, Hs, Ws, origins, tile, False, out=torch.empty((N, len(origins), 3) + tile, device=DEV))
    with pytest.raises(RuntimeError, match="out must be a contiguous fp32 tensor of shape"):
        scaled_tiles_call(image, Hs, Ws, origins, tile, False, out=torch.empty((N, len(origins) + 1, 3) + tile, device=DEV))
    with pytest.raises(RuntimeError, match="out must be a contiguous fp32 tensor of shape"):
        scaled_tiles_call(image, Hs, Ws, origins, tile, False,
                          out=torch.empty((N, len(origins), 3, tile[1], tile[0]), device=DEV).transpose(3, 4))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the library at its limits, over the C ABI on guarded device buffers (tests/mseval_cases.py; the emulator runs the same table)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guarded():
    from ccnet_amd import _mseval_lib
    yield _mseval_lib.get_lib(), MC.DeviceMemory()
    print("largest error / bar on the device:", {k: round(v, 4) for k, v in MC.WORST.items()})


@pytest.mark.parametrize("name", MC.ALL)
def test_limits_on_guarded_buffers(guarded, name):
    MC.run_case(name, *guarded)


def stock_chain(logits, geo, N, H, W, flip):
    """Stock torch on the device: per scale F.interpolate(align_corners=True) of every tile, crop, accumulate, divide, the
    flipped pass mirrored back, then F.interpolate back to (H, W) (in float64, so that the reference's own coordinate
    rounding stays out of the comparison), and the mean: (N, C, H, W) float64."""
    total = None
    for lg, (Hs, Ws, origins, tile) in zip(logits, geo):
        T = len(origins)
        lg = lg.unflatten(0, (N, -1))
        passes = []
        for p in range(2 if flip else 1):
            full = torch.zeros(N, lg.shape[2], Hs, Ws, device=DEV)
            count = torch.zeros(1, 1, Hs, Ws, device=DEV)
            for t, (y1, x1) in enumerate(origins):
                up = F.interpolate(lg[:, p * T + t], size=tile, mode="bilinear", align_corners=True)
                y2, x2 = min(y1 + tile[0], Hs), min(x1 + tile[1], Ws)
                full[:, :, y1:y2, x1:x2] += up[:, :, :y2 - y1, :x2 - x1]
                count[:, :, y1:y2, x1:x2] += 1
            passes.append(full / count)
        s = 0.5 * (passes[0] + passes[1].flip(-1)) if flip else passes[0]
        back = F.interpolate(s.double(), size=(H, W), mode="bilinear", align_corners=True)
        total = back if total is None else total + back
    return total / len(geo)


def _check_vs_stock(stock, pred, conf, label, tol, ignore_label=255):
    C = stock.shape[1]
    want = stock.argmax(1).to(torch.uint8)
    top2 = stock.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < tol
    diff = pred != want
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    n = int(diff.sum())
    if conf is not None:
        keep = label != ignore_label
        ref_cm = torch.bincount(label[keep] * C + want[keep].long(), minlength=C * C).reshape(C, C)
        d = (conf - ref_cm).abs()
        assert int(d.sum()) <= 2 * n and int(d.max()) <= n, (int(d.sum()), n)
    return n


def test_at_scale_against_stock_torch():
    from ccnet_amd.evaluate import accumulate_call, scale_geometry
    H, W, C, scales = 1024, 2048, 19, (0.75, 1.0, 1.25)
    geo = [scale_geometry(H, W, s, (769, 769), False) for s in scales]
    assert [len(g[2]) for g in geo] == [3, 8, 10]
    g = torch.Generator(device=DEV).manual_seed(3)
    logits = [torch.randn(2 * len(gs[2]), C, 97, 97, device=DEV, generator=g) * 3 for gs in geo]
    label = torch.randint(0, C, (1, H, W), device=DEV, generator=g)
    label[torch.rand(1, H, W, device=DEV, generator=g) < 0.05] = 255
    score = torch.empty((1, C, H, W), device=DEV)
    pred = torch.empty((1, H, W), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    for i, (lg, (Hs, Ws, origins, tile)) in enumerate(zip(logits, geo)):
        last = i == 2
        accumulate_call(lg, origins, True, 1, tile, Hs, Ws, H, W, score_in=score if i else None, score_out=score,
                        divide_by=3 if last else 0, labels=label if last else None, pred=pred if last else None,
                        confusion=conf if last else None)
    stock = stock_chain(logits, geo, 1, H, W, True)
    tol = 1e-5 * max(float(lg.abs().max()) for lg in logits)
    err = float((score.double() - stock).abs().max())
    n = _check_vs_stock(stock, pred, conf, label, tol)
    print(f"1024x2048, 3 scales + flip: score err {err:.3e} (bar {tol:.3e}), near-tie prediction differences {n}")
    assert err <= tol


def test_seg_model_whole_image_two_scales_against_stock_torch():
    from ccnet_amd import MultiScaleEvaluator
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    model = Seg_Model(19, recurrence=2).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    image = torch.randn(1, 3, 257, 513, device=DEV, generator=g)
    label = torch.randint(0, 19, (1, 257, 513), device=DEV, generator=g)
    ev = MultiScaleEvaluator(19, scales=(0.5, 1.0), whole=True)
    geo = ev.geometry(257, 513)
    assert [(gs[0], gs[1]) for gs in geo] == [(128, 256), (257, 513)] and all(gs[3] == (gs[0], gs[1]) for gs in geo)
    logits = ev.net_logits(model, image)
    pred = ev.accumulate(logits, label, 257, 513)
    torch.cuda.synchronize()
    stock = stock_chain(logits, geo, 1, 257, 513, False)
    n = _check_vs_stock(stock, pred, ev.confusion, label, 1e-5 * max(float(lg.abs().max()) for lg in logits))
    assert int(ev.confusion.sum()) == 257 * 513
    print(f"Seg_Model whole image, scales (0.5, 1.0): pixels whose prediction differs at a near tie: {n}")
