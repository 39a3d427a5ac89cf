"""CPU checks of the sliding-window evaluation (include/ccnet_eval.h, ccnet_amd/csrc_eval/, ccnet_amd/evaluate.py): the
numpy oracle against the reference fixtures, the tile grid against the reference's loop, the shipped gfx950 library's
surface, the kernel sources run in the SIMT emulator (tests/emu/ + the primitives of tests/emu_eval/) against the oracle,
the rank sharding and the confusion reduction over gloo."""
import ctypes
import glob
import os
import socket

import numpy as np
import pytest
import torch

import lib_checks as L
import eval_cases as EC
import eval_oracle as O
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz")))
SMALL = [f for f in FIXTURES if "recipe" not in f]
EVAL_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_eval")


def _id(path):
    return os.path.basename(path)[:-4]


def test_fixtures_cover_the_issue_cases():
    names = {_id(f) for f in FIXTURES}
    assert {"eval_1024x2048_t769_c19_recipe", "eval_128x256_t97_c19_multi", "eval_60x80_t97_c19_padded",
            "eval_300x160_t97_c19_portrait", "eval_128x256_c19_whole", "eval_200x300_t97_c150"} <= names
    for f in FIXTURES:
        fx = O.load_fixture(f)
        assert (fx["label"] == 255).any() and fx["pred"].shape == (1, fx["H"], fx["W"])


def _origins(fx):
    return [(0, 0)] if fx["whole"] else O.reference_tile_grid(int(fx["H"]), int(fx["W"]), fx["tile"])


@pytest.mark.parametrize("path", FIXTURES, ids=_id)
def test_oracle_reproduces_reference_fixture(path):
    fx = O.load_fixture(path)
    origins = _origins(fx)
    probs = O.sliding_scores(O.fixture_tiles(fx, origins), origins, fx["tile"], int(fx["H"]), int(fx["W"]))
    pred = O.argmax(probs)
    n_diff = O.check_against_fixture(fx, probs, pred, O.confusion(fx["label"], pred, int(fx["C"])), rel=1e-6)
    assert n_diff == 0


def test_tile_grid_equals_the_reference_loop():
    from ccnet_amd.evaluate import tile_grid
    for f in FIXTURES:
        fx = O.load_fixture(f)
        if not fx["whole"]:
            assert tile_grid(fx["H"], fx["W"], fx["tile"]) == O.reference_tile_grid(fx["H"], fx["W"], fx["tile"])
    assert len(tile_grid(1024, 2048, (769, 769))) == 8
    n = 0
    for tile in (33, 97, 129, 385, 513, 769):
        stride = -(-tile * 2 // 3)
        for H in (1, 7, tile - stride + 1, tile - 1, tile, tile + 1, 2 * tile + 5, 1024):
            for W in (1, 13, tile - stride + 1, tile, 3 * tile - 2, 2048):
                ref = O.reference_tile_grid(H, W, (tile, tile))
                got = tile_grid(H, W, (tile, tile))
                if H - tile > -stride and W - tile > -stride:
                    assert got == ref, (H, W, tile)
                    n += 1
                assert len(got) >= 1 and all(0 <= y < H and 0 <= x < W for y, x in got)
    assert n > 100


def test_tile_grid_keeps_one_tile_for_tiny_images():
    from ccnet_amd.evaluate import tile_grid
    assert O.reference_tile_grid(10, 10, (769, 769)) == []           # the reference: no tile, a 0/0 score map
    assert tile_grid(10, 10, (769, 769)) == [(0, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _eval_lib
    return _eval_lib.LIB_PATH


def test_library_exports_exactly_the_header(eval_lib_path):
    from ccnet_amd import _eval_lib
    names = _eval_lib.declared_symbols()
    assert set(names) == set(_eval_lib._PROTOTYPES) and len(names) == 4
    assert L.exported_symbols(eval_lib_path) == names


def test_library_contains_gfx950_code(eval_lib_path):
    blob = open(eval_lib_path, "rb").read()
    assert b"gfx950" in blob and b"sliding_kernel" in blob


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch(eval_lib_path, tmp_path):
    kernels = L.code_object_kernels(eval_lib_path, tmp_path, "_ZN7segeval")
    assert len(kernels) == 1, sorted(kernels)
    bad = L.kernels_using_scratch(kernels)
    assert not bad, bad


def test_version_and_argument_validation_without_a_gpu(eval_lib_path):
    from ccnet_amd import _eval_lib
    lib = _eval_lib.EvalLibrary(eval_lib_path)
    assert lib.ccnet_eval_version() == 100 and lib.ccnet_eval_arch() == b"gfx950"
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    org = _eval_lib.origins_array([(0, 0)] * 65)
    call = lib.ccnet_eval_sliding_f32
    args = dict(T=1, Tf=0, N=1, C=19, h=97, w=97, th=769, tw=769, H=1024, W=2048)

    def run(logits=p, y1x1=org, labels=p, conf=p, **kw):
        a = dict(args, **kw)
        return call(logits, a["T"], a["Tf"], y1x1, a["N"], a["C"], a["h"], a["w"], a["th"], a["tw"], a["H"], a["W"], labels,
                    255, None, None, conf, None)

    assert run(C=257) == -1 and "C=257" in lib.last_error()
    assert run(C=0) == -1
    assert run(T=65) == -1 and "T=65" in lib.last_error()
    assert run(T=0) == -1
    assert run(T=2, Tf=1) == -1
    assert run(H=0) == -1 and run(h=0) == -1 and run(N=0) == -1
    assert run(y1x1=_eval_lib.origins_array([(1024, 0)])) == -1 and "outside" in lib.last_error()
    assert run(logits=None) == -2
    assert run(y1x1=None) == -2
    assert run(labels=None) == -2 and "labels" in lib.last_error()
    assert lib.last_error().startswith("ccnet_eval:")


def test_sources_carry_no_env_knobs_and_no_emulator_code():
    files = L.product_sources(EVAL_CSRC, L.COMMON_CSRC)
    assert "eval_api.hip" in files and "eval_kernels.hpp" in files and "ccnet_host.hpp" in files
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f


def test_cpu_input_raises_instead_of_falling_back():
    from ccnet_amd import SegEvaluator, predict_sliding, predict_whole
    net = O.make_toy_net(19, 0)
    img = torch.zeros(1, 3, 40, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_sliding(net, img, (33, 33), 19)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_whole(net, img)
    ev = SegEvaluator(19, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(net, img, torch.zeros(1, 40, 40, dtype=torch.long))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._eval_lib import EvalLibrary
    return EvalLibrary(L.build_shared_scaffold_emu("eval"))


def emu_eval(lib, tiles, origins, tile, H, W, flip=False, label=None, C=None, conf=None, ignore_label=255):
    """One call of the emulated C ABI with numpy buffers standing in for device memory: (probs, pred, confusion)."""
    from ccnet_amd._eval_lib import origins_array
    tiles = np.ascontiguousarray(tiles, np.float32)
    N, _, C, h, w = tiles.shape
    probs = np.full((N, C, H, W), np.nan, np.float32)
    pred = np.full((N, H, W), 0xEE, np.uint8)
    conf = np.zeros((C, C), np.int64) if conf is None else conf
    lab = None if label is None else np.ascontiguousarray(label, np.int64)
    lib.check(lib.ccnet_eval_sliding_f32(tiles.ctypes.data, len(origins), len(origins) if flip else 0, origins_array(origins),
                                         N, C, h, w, tile[0], tile[1], H, W, None if lab is None else lab.ctypes.data, ignore_label,
                                         probs.ctypes.data, pred.ctypes.data, None if lab is None else conf.ctypes.data,
                                         None), "sliding")
    return probs, pred, conf


@pytest.mark.parametrize("path", SMALL, ids=_id)
def test_emulated_kernel_matches_reference_fixture(emu, path):
    fx = O.load_fixture(path)
    origins = _origins(fx)
    probs, pred, conf = emu_eval(emu, O.fixture_tiles(fx, origins), origins, fx["tile"], int(fx["H"]), int(fx["W"]),
                                 label=fx["label"])
    O.check_against_fixture(fx, probs, pred, conf)


@pytest.mark.parametrize("case", [
    dict(N=2, H=70, W=90, tile=33, C=19, flip=False),      # every image its own tiles
    dict(N=1, H=70, W=90, tile=33, C=19, flip=True),       # flipped pass mirrored back along W
    dict(N=2, H=20, W=25, tile=33, C=7, flip=True),        # image smaller than the tile, odd C (padded histogram word)
])
def test_emulated_kernel_matches_oracle(emu, case):
    N, H, W, tile, C, flip = (case[k] for k in ("N", "H", "W", "tile", "C", "flip"))
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(H, W, (tile, tile))
    rng = np.random.default_rng(H * W + N)
    h = (tile + 7) // 8
    tiles = (rng.standard_normal((N, len(origins) * (2 if flip else 1), C, h, h)) * 3).astype(np.float32)
    _, label = O.make_case_inputs(N, H, W, C, seed=7)
    ref = O.sliding_scores(tiles, origins, (tile, tile), H, W, flip)
    probs, pred, conf = emu_eval(emu, tiles, origins, (tile, tile), H, W, flip, label)
    assert np.abs(probs - ref).max() <= 1e-5 * np.abs(tiles).max()
    gap = O.top2_gap(ref)
    diff = pred != O.argmax(ref)
    assert np.all(gap[diff] < 1e-5 * np.abs(tiles).max())
    np.testing.assert_array_equal(conf, O.confusion(label, pred, C))       # the counts of its own prediction, exactly


def test_emulated_confusion_accumulates_across_calls(emu):
    fx = O.load_fixture(os.path.join(GOLDEN, "eval_60x80_t97_c19_padded.npz"))
    origins = _origins(fx)
    tiles = O.fixture_tiles(fx, origins)
    _, _, conf = emu_eval(emu, tiles, origins, fx["tile"], 60, 80, label=fx["label"])
    _, _, conf2 = emu_eval(emu, tiles, origins, fx["tile"], 60, 80, label=fx["label"], conf=conf.copy())
    np.testing.assert_array_equal(conf2, 2 * conf)


@pytest.mark.parametrize("low_half", [True, False], ids=["low_half", "high_half"])
def test_emulated_single_cell_counter_saturation(emu, low_half):
    """111 x 111 pixels, every counted one in the same cell: four workgroups of up to 4096 counts each, in the low or the
    high 16 bits of the LDS word."""
    l, a = (2, 4) if low_half else (2, 5)
    tiles = np.zeros((1, 1, 19, 14, 14), np.float32)
    tiles[:, :, a] = 10.0
    label = np.full((1, 111, 111), l, np.int64)
    label[0, 5, 7:11] = 255
    label[0, 90, 3] = 19
    n = int((label == l).sum())
    assert n >= 3 * 4096 + 17 and ((l * 19 + a) % 2 == 0) == low_half
    _, pred, conf = emu_eval(emu, tiles, [(0, 0)], (111, 111), 111, 111, label=label)
    assert np.all(pred == a) and int(conf[l, a]) == n and int(conf.sum()) == n


def test_emulated_c256_ignore_outside_and_out_of_range_labels(emu):
    """C = 256 with ignore -1 counts label 255 and pred 255; with ignore 7 inside [0, C), 7, negative labels and labels
    >= C are not counted."""
    from ccnet_amd.evaluate import tile_grid
    H, W = 40, 50
    origins = tile_grid(H, W, (33, 33))
    rng = np.random.default_rng(9)
    tiles = (rng.standard_normal((1, len(origins), 256, 5, 5)) * 3).astype(np.float32)
    tiles[:, :, 255] += 4.0
    label = rng.integers(0, 256, (1, H, W)).astype(np.int64)
    label[:, :, :10] = 255
    label[0, 0, :4] = -1
    _, pred, conf = emu_eval(emu, tiles, origins, (33, 33), H, W, label=label, ignore_label=-1)
    np.testing.assert_array_equal(conf, O.confusion(label, pred, 256, ignore_label=-1))
    assert conf[255, 255] > 0 and int(conf.sum()) == H * W - 4
    label = rng.integers(-300, 300, (1, H, W)).astype(np.int64)
    label[:, ::3] = 7
    label[:, 1::3] = rng.integers(0, 19, (1, len(range(1, H, 3)), W))
    _, pred, conf = emu_eval(emu, tiles[:, :, :19], origins, (33, 33), H, W, label=label, ignore_label=7)
    np.testing.assert_array_equal(conf, O.confusion(label, pred, 19, ignore_label=7))
    assert int(conf.sum()) == int(((label != 7) & (label >= 0) & (label < 19)).sum()) and not conf[7].any()


@pytest.mark.parametrize("H,W,tile,hw,flip", [
    (20, 28, (8, 8), (1, 1), True),             # 1 x 1 logits: up-sampling scale 0
    (40, 60, (33, 41), (5, 6), True),           # non-square tile
    (60, 20, (33, 33), (5, 5), True),           # narrower than the tile along W only
], ids=["logits_1x1", "nonsquare_tile", "narrow_w"])
def test_emulated_degenerate_geometry(emu, H, W, tile, hw, flip):
    from ccnet_amd.evaluate import tile_grid
    origins = tile_grid(H, W, tile)
    rng = np.random.default_rng(H + W)
    tiles = (rng.standard_normal((1, len(origins) * (2 if flip else 1), 7, hw[0], hw[1])) * 3).astype(np.float32)
    _, label = O.make_case_inputs(1, H, W, 7, seed=H * W)
    ref = O.sliding_scores(tiles, origins, tile, H, W, flip)
    probs, pred, conf = emu_eval(emu, tiles, origins, tile, H, W, flip, label)
    assert np.abs(probs - ref).max() <= 1e-5 * np.abs(tiles).max()
    diff = pred != O.argmax(ref)
    assert np.all(O.top2_gap(ref)[diff] < 1e-5 * np.abs(tiles).max())
    np.testing.assert_array_equal(conf, O.confusion(label, pred, 7))


# ---------------------------------------------------------------------------------------------------------------------
# the library at its limits, over the C ABI on guarded host buffers (tests/eval_cases.py; the device runs the same table).
# Every call is repeated through the multi-scale library at Hs = H, Ws = W, hence its emulator build.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_multi():
    from ccnet_amd._mseval_lib import MsEvalLibrary
    emu_dir = os.path.join(ROOT, "tests", "emu_eval")
    out = L.build_emu_library(os.path.join(emu_dir, "libmseval_emu.so"), os.path.join(EVAL_CSRC, "mseval_api.hip"),
                              [emu_dir, L.EMU_DIR, EVAL_CSRC, L.INCLUDE], reads=(L.EMU_COMMON_DIR, L.COMMON_CSRC))
    return MsEvalLibrary(out)


@pytest.mark.parametrize("name", EC.ALL)
def test_emulated_limits(emu, emu_multi, name):
    EC.run_case(name, emu, emu_multi, EC.HostMemory())


# ---------------------------------------------------------------------------------------------------------------------
# mIoU, sharding and the distributed reduction
# ---------------------------------------------------------------------------------------------------------------------
def test_mean_iou_is_the_reference_formula():
    from ccnet_amd.evaluate import mean_iou
    cm = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    r = mean_iou(torch.from_numpy(cm))
    iu = np.array([5 / (6 + 7 - 5), 3 / (5 + 4 - 3), 0.0])
    np.testing.assert_allclose(r["IU_array"], iu)
    assert r["meanIU"] == pytest.approx(iu.mean())                 # averaged over all C classes, the empty one included


def test_rank_sharding_takes_every_image_once():
    from ccnet_amd.evaluate import shard_indices
    for n in (0, 1, 7, 8, 500):
        for world in (1, 2, 3, 4, 8):
            got = sorted(i for r in range(world) for i in shard_indices(n, r, world))
            assert got == list(range(n))
    assert list(shard_indices(8, 1, 2)) == [1, 3, 5, 7]


def test_eval_driver_flags():
    from ccnet_amd.eval_synthetic import build_parser
    a = build_parser().parse_args([])
    assert (a.images, a.height, a.width, a.tile, a.whole, a.flip, a.recurrence, a.num_classes, a.bf16, a.seed) == \
        (8, 1024, 2048, 769, False, False, 2, 19, False, 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, out):
    import sys
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from ccnet_amd.evaluate import SegEvaluator
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ev = SegEvaluator(4, device="cpu")
        ev.confusion += torch.arange(16, dtype=torch.int64).reshape(4, 4) * (rank + 1)
        r = ev.result()
        out.put((rank, r["meanIU"], r["IU_array"].tolist(), ev.confusion.tolist()))
    finally:
        dist.destroy_process_group()


def test_confusion_all_reduce_over_gloo_world_2():
    import torch.multiprocessing as mp
    from ccnet_amd.evaluate import mean_iou
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = mean_iou(torch.arange(16, dtype=torch.int64).reshape(4, 4) * 3)
    for rank, miou, iu, local in res:
        assert miou == pytest.approx(want["meanIU"]) and np.allclose(iu, want["IU_array"])
        assert local == (torch.arange(16).reshape(4, 4) * (rank + 1)).tolist()     # the local counts stay the rank's own
