"""CPU checks of multi-scale evaluation (include/ccnet_mseval.h, ccnet_amd/csrc_eval/mseval_*, ccnet_amd/evaluate.py): the
shipped gfx950 library's surface and argument checks, the numpy oracle against the reference + scipy fixtures, and both kernels'
sources run in the SIMT emulator (tests/emu/ + the primitives of tests/emu_eval/) against the oracle and the fixtures."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import eval_oracle as O
import lib_checks as L
import mseval_cases as MC
import mseval_oracle as M
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mseval_*.npz")))
EVAL_CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_eval")
EMU_EVAL = os.path.join(ROOT, "tests", "emu_eval")


def _id(path):
    return os.path.basename(path)[:-4]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, the scaled size and the fixtures
# ---------------------------------------------------------------------------------------------------------------------
def test_fixtures_cover_the_issue_cases():
    assert {_id(f) for f in FIXTURES} == {
        "mseval_128x256_t97_c19_seven_flip", "mseval_60x80_t97_c19_small", "mseval_300x160_t97_c19_portrait_flip",
        "mseval_128x256_c19_whole", "mseval_128x256_t97_c19_reference_1x"}
    fx = M.load_fixture(os.path.join(GOLDEN, "mseval_128x256_t97_c19_seven_flip.npz"))
    assert fx["scales"] == [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0] and fx["flip"]
    assert [len(g[2]) for g in M.fixture_geometry(fx)] == [2, 3, 8, 10, 18, 21, 32]
    for f in FIXTURES:
        fx = M.load_fixture(f)
        assert fx["pred"].shape == (1, fx["H"], fx["W"]) and fx["probs_sample"].shape == (8192,)


def test_scaled_size_is_round_half_to_even_and_equals_the_fixtures():
    from ccnet_amd import scaled_size
    assert scaled_size(97, 97, 0.5) == (48, 48) and scaled_size(97, 97, 1.5) == (146, 146) and scaled_size(33, 33, 0.5) == (16, 16)
    assert scaled_size(1024, 2048, 0.75) == (768, 1536) and scaled_size(1024, 2048, 1.0) == (1024, 2048)
    assert scaled_size(1, 3, 0.1) == (1, 1)                                   # never empty
    for f in FIXTURES:
        fx = M.load_fixture(f)
        for s, size in zip(fx["scales"], fx["sizes"].tolist()):
            assert scaled_size(fx["H"], fx["W"], s) == tuple(size) == M.scaled_size(fx["H"], fx["W"], s)


@pytest.mark.parametrize("path", FIXTURES, ids=_id)
def test_oracle_reproduces_reference_fixture(path):
    fx = M.load_fixture(path)
    probs = M.fixture_scores(fx)
    pred = O.argmax(probs)
    assert M.check_against_fixture(fx, probs, pred, O.confusion(fx["label"], pred, fx["C"]), rel=1e-6) == 0


def test_oracle_geometry_is_the_host_layer_geometry():
    from ccnet_amd.evaluate import scale_geometry
    for H, W, tile in ((128, 256, 97), (60, 80, 97), (300, 160, 97), (1024, 2048, 769), (97, 131, 65)):
        for s in (0.5, 0.75, 1.0, 1.25, 1.5, 2.0):
            for whole in (False, True):
                assert scale_geometry(H, W, s, (tile, tile), whole) == M.geometry(H, W, s, (tile, tile), whole)


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _mseval_lib
    return _mseval_lib.LIB_PATH


def test_build_table_names_the_unit_in_the_evaluation_row(lib_path):
    import __graft_entry__ as g
    row = [e for e in g.EXTENSIONS if e.name == "eval"][0]
    assert [u.name for u in row.libraries()] == ["eval", "mseval"] and row.units[0].csrc == row.csrc
    assert g.MSEVAL_LIB == lib_path and lib_path.endswith(os.path.join("csrc_eval", "libccnet_mseval.so"))
    rest = lambda flags: [f for f in flags if "--version-script" not in f]    # noqa: E731  (the same flags but its own map)
    assert rest(g.MSEVAL_HIPCC_FLAGS) == rest(g.EVAL_HIPCC_FLAGS) and len(g.MSEVAL_HIPCC_FLAGS) == len(g.EVAL_HIPCC_FLAGS)
    assert row.units[0].exports.endswith("mseval_exports.map") and row.units[0].sources()[:-2] == row.sources()[:-2]


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _mseval_lib
    names = _mseval_lib.declared_symbols()
    assert set(names) == set(_mseval_lib._PROTOTYPES) and len(names) == 5
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"tiles_kernel" in blob and b"accumulate_kernel" in blob and b"sliding_kernel" not in blob


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_no_kernel_uses_scratch_and_the_single_scale_library_keeps_one_kernel(lib_path, tmp_path):
    from ccnet_amd import _eval_lib
    (tmp_path / "ms").mkdir()
    (tmp_path / "ev").mkdir()
    kernels = L.code_object_kernels(lib_path, tmp_path / "ms", "_ZN6mseval")
    assert len(kernels) == 2, sorted(kernels)
    assert not L.kernels_using_scratch(kernels)
    assert not L.code_object_kernels(lib_path, tmp_path / "ms", "_ZN7segeval")
    assert len(L.code_object_kernels(_eval_lib.LIB_PATH, tmp_path / "ev", "_ZN7segeval")) == 1
    assert not L.code_object_kernels(_eval_lib.LIB_PATH, tmp_path / "ev", "_ZN6mseval")


def test_sources_use_only_the_platform_primitives():
    files = L.product_sources(EVAL_CSRC)
    assert {"mseval_api.hip", "mseval_kernels.hpp", "eval_sample.hpp", "eval_kernels.hpp", "eval_api.hip"} <= set(files)
    for f in ("mseval_api.hip", "mseval_kernels.hpp", "eval_sample.hpp"):
        text = files[f]
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomicAdd" not in text and "<<<" not in text and "hipMemcpy" not in text and "Synchronize" not in text, f


def test_version_and_argument_validation_without_a_gpu(lib_path):
    from ccnet_amd import _mseval_lib
    lib = _mseval_lib.MsEvalLibrary(lib_path)
    assert lib.ccnet_mseval_version() == 100 and lib.ccnet_mseval_arch() == b"gfx950"
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first
    org = _mseval_lib.origins_array([(0, 0)] * 65)
    base = dict(T=1, Tf=0, N=1, C=19, h=97, w=97, th=769, tw=769, Hs=768, Ws=1536, H=1024, W=2048, div=0, Cin=3, first=0, count=1)

    def acc(logits=p, y1x1=org, labels=p, conf=p, **kw):
        a = dict(base, **kw)
        return lib.ccnet_mseval_accumulate_f32(logits, a["T"], a["Tf"], y1x1, a["N"], a["C"], a["h"], a["w"], a["th"], a["tw"],
                                               a["Hs"], a["Ws"], a["H"], a["W"], None, None, a["div"], labels, 255, None, conf, None)

    def til(image=p, y1x1=org, out=p, **kw):
        a = dict(base, **kw)
        return lib.ccnet_mseval_tiles_f32(image, a["N"], a["Cin"], a["H"], a["W"], a["Hs"], a["Ws"], a["T"], a["Tf"], y1x1,
                                          a["th"], a["tw"], a["first"], a["count"], out, None)

    assert acc(C=257) == -1 and "C=257" in lib.last_error()
    assert acc(C=0) == -1
    for call in (acc, til):
        assert call(T=65) == -1 and "T=65" in lib.last_error()
        assert call(T=0) == -1
        assert call(T=2, Tf=1) == -1
        assert call(H=0) == -1 and call(Hs=0) == -1 and call(N=0) == -1 and call(th=0) == -1
        assert call(Hs=65536, Ws=32768) == -1 and "too large" in lib.last_error()        # Hs * Ws = 2^31
        assert call(H=65536, W=32768) == -1 and "too large" in lib.last_error()
        # the origin must lie in the SCALED image: row 768 is inside the 1024 x 2048 image but not inside 768 x 1536
        assert call(y1x1=_mseval_lib.origins_array([(768, 0)])) == -1 and "outside the 768x1536 scaled" in lib.last_error()
        assert call(y1x1=_mseval_lib.origins_array([(0, 1536)])) == -1 and call(y1x1=_mseval_lib.origins_array([(-1, 0)])) == -1
        assert call(y1x1=None) == -2
    assert acc(h=0) == -1 and acc(div=-1) == -1 and "divide_by" in lib.last_error()
    assert acc(logits=None) == -2
    assert acc(labels=None) == -2 and "labels" in lib.last_error()
    assert til(Cin=0) == -1
    assert til(first=1) == -1 and til(count=0) == -1 and til(first=-1) == -1 and til(T=2, Tf=2, first=3, count=2) == -1
    assert "outside the 4 tiles" in lib.last_error()
    assert til(image=None) == -2 and til(out=None) == -2
    assert lib.last_error().startswith("ccnet_mseval:")


def test_cpu_input_raises_instead_of_falling_back():
    from ccnet_amd import MultiScaleEvaluator, predict_multiscale
    net = O.make_toy_net(19, 0)
    img = torch.zeros(1, 3, 40, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_multiscale(net, img, (33, 33), (0.5, 1.0), 19)
    ev = MultiScaleEvaluator(19, scales=(0.75, 1.0), tile_size=(33, 33), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(net, img, torch.zeros(1, 40, 40, dtype=torch.long))
    with pytest.raises(ValueError):
        MultiScaleEvaluator(19, scales=(), device="cpu")
    with pytest.raises(ValueError):
        MultiScaleEvaluator(257, device="cpu")


def test_eval_driver_flags():
    from ccnet_amd.eval_synthetic import build_parser, parse_scales
    a = build_parser().parse_args([])
    assert (a.scales, a.tile_batch) == ("1.0", 8) and parse_scales(a.scales) == (1.0,)
    a = build_parser().parse_args(["--scales", "0.75,1.0,1.25", "--tile-batch", "4"])
    assert parse_scales(a.scales) == (0.75, 1.0, 1.25) and a.tile_batch == 4


# ---------------------------------------------------------------------------------------------------------------------
# the kernel sources in the SIMT emulator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._mseval_lib import MsEvalLibrary
    out = L.build_emu_library(os.path.join(EMU_EVAL, "libmseval_emu.so"), os.path.join(EVAL_CSRC, "mseval_api.hip"),
                              [EMU_EVAL, L.EMU_DIR, EVAL_CSRC, L.INCLUDE], reads=(L.EMU_COMMON_DIR, L.COMMON_CSRC))
    return MsEvalLibrary(out)


@pytest.fixture(scope="module")
def emu_single():
    from ccnet_amd._eval_lib import EvalLibrary
    return EvalLibrary(L.build_shared_scaffold_emu("eval"))


def emu_tiles(lib, image, Hs, Ws, origins, tile, flip, first=0, count=None):
    from ccnet_amd._mseval_lib import origins_array
    image = np.ascontiguousarray(image, np.float32)
    N, Cin, H, W = image.shape
    T = len(origins)
    count = T * (2 if flip else 1) - first if count is None else count
    out = np.full((N, count, Cin, tile[0], tile[1]), np.nan, np.float32)
    lib.check(lib.ccnet_mseval_tiles_f32(image.ctypes.data, N, Cin, H, W, Hs, Ws, T, T if flip else 0, origins_array(origins),
                                         tile[0], tile[1], first, count, out.ctypes.data, None), "tiles")
    return out


def emu_accumulate(lib, logits, geo, H, W, flip, score_in=None, divide_by=0, label=None, conf=None, want_score=True,
                   ignore_label=255):
    """One emulated ccnet_mseval_accumulate_f32 call for geo = (Hs, Ws, origins, tile): (score, pred, confusion)."""
    from ccnet_amd._mseval_lib import origins_array
    Hs, Ws, origins, tile = geo
    logits = np.ascontiguousarray(logits, np.float32)
    N, _, C, h, w = logits.shape
    score = np.full((N, C, H, W), np.nan, np.float32) if want_score else None
    pred = np.full((N, H, W), 0xEE, np.uint8)
    conf = np.zeros((C, C), np.int64) if conf is None else conf
    lab = None if label is None else np.ascontiguousarray(label, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                          # noqa: E731
    lib.check(lib.ccnet_mseval_accumulate_f32(logits.ctypes.data, len(origins), len(origins) if flip else 0,
                                              origins_array(origins), N, C, h, w, tile[0], tile[1], Hs, Ws, H, W, ptr(score_in),
                                              ptr(score), divide_by, ptr(lab), ignore_label, pred.ctypes.data,
                                              None if lab is None else conf.ctypes.data, None), "accumulate")
    return score, pred, conf


def emu_multiscale(lib, logits, geo, H, W, flip, label):
    score = None
    for i, (lg, g) in enumerate(zip(logits, geo)):
        last = i == len(geo) - 1
        score, pred, conf = emu_accumulate(lib, lg, g, H, W, flip, score_in=score, divide_by=len(geo) if last else 0,
                                           label=label if last else None)
    return score, pred, conf


def random_logits(geo, N, C, flip, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((N, len(g[2]) * (2 if flip else 1), C, (g[3][0] + 7) // 8, (g[3][1] + 7) // 8)) * 3)
            .astype(np.float32) for g in geo]


TILE_CASES = [(s, tile, flip) for s in (0.5, 0.75, 1.5, 2.0) for tile in (33, None) for flip in (False, True)]


@pytest.mark.parametrize("s,tile,flip", TILE_CASES)
def test_emulated_tiles_kernel_matches_oracle(emu, s, tile, flip):
    image, _ = O.make_case_inputs(2, 60, 80, 19, seed=21)
    Hs, Ws, origins, tile = M.geometry(60, 80, s, (tile, tile), tile is None)
    got = emu_tiles(emu, image, Hs, Ws, origins, tile, flip)
    ref = M.zoom_tiles(image, Hs, Ws, origins, tile, flip)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6 * np.abs(image).max()
    parts = [emu_tiles(emu, image, Hs, Ws, origins, tile, flip, first, min(3, got.shape[1] - first))
             for first in range(0, got.shape[1], 3)]
    assert np.array_equal(np.concatenate(parts, 1), got)


def test_emulated_tiles_at_scale_one_are_cut_tiles(emu):
    from ccnet_amd.evaluate import cut_tiles, tile_grid
    image, _ = O.make_case_inputs(2, 60, 80, 19, seed=22)
    image[0, 0, 3, 5] = np.inf                                                 # a copy: no arithmetic touches the values
    origins = tile_grid(60, 80, (33, 33))
    got = emu_tiles(emu, image, 60, 80, origins, (33, 33), True)
    want = cut_tiles(torch.from_numpy(image), origins, (33, 33), True).numpy().reshape(got.shape)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("N,H,W,tile,C,scales,flip", [
    (2, 40, 56, 33, 7, (0.5, 1.0, 2.0), True),          # odd C, every image its own tiles
    (1, 33, 47, 33, 19, (0.75, 1.25), False),
    (1, 30, 44, None, 5, (0.5, 1.5), True),             # whole
    (1, 1, 9, 8, 3, (1.0, 2.0), False),                 # one output row: n_out == 1 on an axis
])
def test_emulated_accumulate_matches_oracle(emu, N, H, W, tile, C, scales, flip):
    geo = [M.geometry(H, W, s, (tile, tile), tile is None) for s in scales]
    logits = random_logits(geo, N, C, flip, seed=H * W + C)
    _, label = O.make_case_inputs(N, H, W, C, seed=5)
    ref = M.multiscale_scores(logits, geo, H, W, flip)
    score, pred, conf = emu_multiscale(emu, logits, geo, H, W, flip, label)
    tol = 1e-5 * max(float(np.abs(lg).max()) for lg in logits)
    assert np.abs(score - ref).max() <= tol
    diff = pred != O.argmax(ref)
    assert np.all(O.top2_gap(ref)[diff] < tol)
    np.testing.assert_array_equal(conf, O.confusion(label, pred, C))


@pytest.mark.parametrize("path", FIXTURES, ids=_id)
def test_emulated_kernels_match_reference_fixture(emu, path):
    fx = M.load_fixture(path)
    geo = M.fixture_geometry(fx)
    logits = []
    for Hs, Ws, origins, tile in geo:                                          # the emulated gather feeds the toy net
        tiles = emu_tiles(emu, fx["image"], Hs, Ws, origins, tile, fx["flip"])
        with torch.no_grad():
            logits.append(fx["net"](torch.from_numpy(tiles[0]))[0].numpy()[None])
    score, pred, conf = emu_multiscale(emu, logits, geo, fx["H"], fx["W"], fx["flip"], fx["label"])
    M.check_against_fixture(fx, score, pred, conf)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_emulated_scale_one_is_the_single_scale_kernel_bit_for_bit(emu, emu_single, flip):
    from ccnet_amd._eval_lib import origins_array
    N, H, W, C, tile = 2, 70, 90, 19, (33, 33)
    geo = M.geometry(H, W, 1.0, tile, False)
    logits = random_logits([geo], N, C, flip, seed=31)[0]
    _, label = O.make_case_inputs(N, H, W, C, seed=31)
    score, pred, conf = emu_accumulate(emu, logits, geo, H, W, flip, divide_by=1, label=label)
    probs = np.full((N, C, H, W), np.nan, np.float32)
    pred1 = np.full((N, H, W), 0xEE, np.uint8)
    conf1 = np.zeros((C, C), np.int64)
    T = len(geo[2])
    emu_single.check(emu_single.ccnet_eval_sliding_f32(logits.ctypes.data, T, T if flip else 0, origins_array(geo[2]), N, C,
                                                       logits.shape[3], logits.shape[4], tile[0], tile[1], H, W,
                                                       label.ctypes.data, 255, probs.ctypes.data, pred1.ctypes.data,
                                                       conf1.ctypes.data, None), "sliding")
    assert np.array_equal(score.view(np.uint32), probs.view(np.uint32))
    assert np.array_equal(pred, pred1) and np.array_equal(conf, conf1)


def test_emulated_in_place_accumulation_and_divide_by(emu):
    H, W, C = 33, 47, 7
    geo = [M.geometry(H, W, s, (33, 33), False) for s in (0.75, 1.25)]
    logits = random_logits(geo, 1, C, True, seed=41)
    _, label = O.make_case_inputs(1, H, W, C, seed=41)
    first, _, _ = emu_accumulate(emu, logits[0], geo[0], H, W, True)
    out, pred, conf = emu_accumulate(emu, logits[1], geo[1], H, W, True, score_in=first, divide_by=2, label=label)
    # in place: score_out == score_in
    from ccnet_amd._mseval_lib import origins_array
    buf = first.copy()
    pred2 = np.zeros((1, H, W), np.uint8)
    lab = np.ascontiguousarray(label, np.int64)
    Hs, Ws, origins, tile = geo[1]
    emu.check(emu.ccnet_mseval_accumulate_f32(logits[1].ctypes.data, len(origins), len(origins), origins_array(origins), 1, C,
                                              logits[1].shape[3], logits[1].shape[4], tile[0], tile[1], Hs, Ws, H, W,
                                              buf.ctypes.data, buf.ctypes.data, 2, lab.ctypes.data, 255, pred2.ctypes.data,
                                              conf.ctypes.data, None), "accumulate")
    assert np.array_equal(buf, out) and np.array_equal(pred2, pred)
    np.testing.assert_array_equal(conf, 2 * O.confusion(label, pred, C))        # accumulated over the two calls
    undivided, _, _ = emu_accumulate(emu, logits[1], geo[1], H, W, True, score_in=first)
    assert np.array_equal(out, undivided / np.float32(2)) and not np.array_equal(out, undivided)


# ---------------------------------------------------------------------------------------------------------------------
# the library at its limits, over the C ABI on guarded host buffers (tests/mseval_cases.py; the device runs the same table)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL)
def test_emulated_limits(emu, name):
    MC.run_case(name, emu, MC.HostMemory())
