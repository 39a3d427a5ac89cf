"""CPU checks of the input-pipeline library (include/ccnet_augment.h, ccnet_amd/csrc_augment/, ccnet_amd/augment.py): the
shipped gfx950 library's surface and its place in the build table, the size and parameter arithmetic against hand values and a
literal restatement of the reference's draws, the datasets on tiny PNG files, every argument check without a device, and the
oracle's image against torch's CPU F.interpolate away from exact ties."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import augment_oracle as D
import lib_checks as L
from conftest import ROOT
from guarded_memory import HostMemory

CSRC = os.path.join(ROOT, "ccnet_amd", "csrc_augment")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _augment_lib
    return _augment_lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    from ccnet_amd import _augment_lib
    return _augment_lib.AugmentLibrary(lib_path)


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._augment_lib import AugmentLibrary
    return AugmentLibrary(L.build_shared_scaffold_emu("augment"))


def test_build_table_keeps_its_rows_and_the_library_is_a_second_unit():
    import __graft_entry__ as g
    rows = [u for e in g.EXTENSIONS for u in e.libraries()]
    assert len(g.EXTENSIONS) == 7 and len(rows) == 9 and "augment" not in [u.name for u in rows]
    unit = [e for e in g.SECOND_UNITS if e.name == "augment"][0]
    assert g.all_libraries() == rows + g.SECOND_UNITS and [e.name for e in g.SECOND_UNITS] == ["celovasz", "augment"]
    assert unit.csrc == CSRC and unit.binding == "_augment_lib" and unit.exports == os.path.join(CSRC, "exports.map")
    assert unit.unit == os.path.join(CSRC, "augment_api.hip") and unit.header.endswith("ccnet_augment.h")
    assert g.AUGMENT_LIB == os.path.join(CSRC, "libccnet_augment.so")
    assert g.AUGMENT_HIPCC_FLAGS == g._BASE_FLAGS + ["-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-I" + CSRC,
                                                     "-I" + os.path.join(ROOT, "include")]
    assert os.path.join(ROOT, "ccnet_amd", "csrc_common", "ccnet_host.hpp") in unit.sources()


def test_library_exports_exactly_the_header(lib_path):
    from ccnet_amd import _augment_lib
    names = _augment_lib.declared_symbols()
    assert names == sorted(["ccnet_augment_version", "ccnet_augment_arch", "ccnet_augment_last_error_string",
                            "ccnet_augment_scaled_size", "ccnet_augment_crop_u8"])
    assert set(names) == set(_augment_lib._PROTOTYPES)
    assert L.exported_symbols(lib_path) == names


def test_library_contains_gfx950_code_and_the_binding_mirrors_the_header(lib_path, lib):
    from ccnet_amd import _augment_lib as m
    blob = open(lib_path, "rb").read()
    assert b"gfx950" in blob and b"_ZN7augment11crop_kernel" in blob
    assert lib.ccnet_augment_version() == 100 == m.CCNET_AUGMENT_VERSION and lib.ccnet_augment_arch() == b"gfx950"
    header = open(m.HEADER_PATH).read()
    fields = ("FRAME_OFF", "LABEL_OFF", "HS", "WS", "PITCH", "NUM", "DEN", "HZ", "WZ", "H_OFF", "W_OFF", "MIRROR")
    for k, field in enumerate(fields):
        assert re.search(rf"#define CCNET_AUGMENT_{field}\s+{k}\b", header), field
        assert getattr(m, field) == k
    assert f"#define CCNET_AUGMENT_DESC_INTS {m.DESC_INTS}\n" in header and m.DESC_INTS == D.DESC_INTS
    assert f"#define CCNET_AUGMENT_MAX_RATIO {m.MAX_RATIO}\n" in header and f"#define CCNET_AUGMENT_MAX_SIDE {m.MAX_SIDE}\n" in header


@pytest.mark.skipif(not L.HAVE_LLVM_BINUTILS, reason="no LLVM binutils")
def test_the_kernel_uses_no_scratch(lib_path, tmp_path):
    kernels = L.code_object_kernels(lib_path, tmp_path, "_ZN7augment")
    assert len(kernels) == 1, sorted(kernels)
    assert not L.kernels_using_scratch(kernels)


def test_sources_carry_no_env_knobs_no_emulator_code_and_no_atomics():
    files = L.product_sources(CSRC)
    assert set(files) == {"augment_api.hip", "augment_kernels.hpp", "augment_platform.hpp"}
    for f, text in files.items():
        assert "getenv" not in text and "CCNET_EMU" not in text and "hip_emu" not in text and "emu::" not in text, f
        assert "atomicAdd" not in text and "__shared__" not in text and "asm volatile" not in text, f
        assert "hipMemcpy" not in text and "Synchronize" not in text and "hipMalloc" not in text, f       # nothing is read back


def test_binding_refuses_a_missing_library_and_another_abi_version(lib_path, tmp_path, monkeypatch):
    from ccnet_amd import _augment_lib as m
    assert issubclass(m.AugmentError, RuntimeError)
    with pytest.raises(m.AugmentError, match="not found"):
        m.AugmentLibrary(str(tmp_path / "libccnet_missing.so"))
    monkeypatch.setattr(m, "CCNET_AUGMENT_VERSION", m.CCNET_AUGMENT_VERSION + 1)
    with pytest.raises(m.AugmentError, match="rebuild"):
        m.AugmentLibrary(m.LIB_PATH)


HAND_SIZES = [((5, 7, 1, 2), (2, 4)),            # 2.5 -> 2 and 3.5 -> 4: ties go to the even neighbour
              ((1, 3, 1, 2), (1, 2)),            # 0.5 -> 0 -> at least 1; 1.5 -> 2
              ((20, 30, 7, 10), (14, 21)), ((20, 30, 21, 10), (42, 63)), ((20, 30, 1, 1), (20, 30)),
              ((1024, 2048, 7, 10), (717, 1434)),          # 716.8, 1433.6
              ((1024, 2048, 21, 10), (2150, 4301)),        # 2150.4, 4300.8
              ((1024, 2048, 15, 10), (1536, 3072)), ((5, 6, 1023, 1024), (5, 6)), ((5, 6, 1024, 1), (5120, 6144)),
              ((15, 25, 13, 10), (20, 32)),                # 19.5 -> 20 (odd quotient rounds up), 32.5 -> 32
              ((20, 30, 1, 1024), (1, 1))]


@pytest.mark.parametrize("args,want", HAND_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_scaled_size_against_hand_values(lib, args, want):
    from ccnet_amd import augment
    assert augment.scaled_size(*args) == want
    assert lib.scaled_size(*args) == want
    assert D.scaled_size(*args) == want


def test_scaled_size_of_the_library_agrees_with_python_and_refuses_its_limits(lib):
    from ccnet_amd import augment
    rng = random.Random(5)
    for _ in range(2000):
        h, w, num, den = rng.randint(1, 3000), rng.randint(1, 3000), rng.randint(1, 1024), rng.randint(1, 1024)
        want = augment.scaled_size(h, w, num, den)
        hz, wz = ctypes.c_int(-7), ctypes.c_int(-7)
        code = lib.ccnet_augment_scaled_size(h, w, num, den, hz, wz)
        if max(want) <= 65535:
            assert code == 0 and (hz.value, wz.value) == want, (h, w, num, den)
        else:
            assert code == -1 and (hz.value, wz.value) == (-7, -7)
    hz = ctypes.c_int(0)
    for bad in ((10, 10, 0, 1), (10, 10, 1, 0), (10, 10, 1025, 1), (10, 10, 1, 1025), (0, 10, 1, 1), (10, 0, 1, 1), (64, 64, 1024, 1)):
        assert lib.ccnet_augment_scaled_size(*bad, hz, hz) == -1, bad
        assert lib.last_error().startswith("ccnet_augment: scaled_size")
    assert lib.ccnet_augment_scaled_size(10, 10, 1, 1, None, None) == -2


def reference_draws(seed, height, width, crop, first, steps, scale=True, mirror=True):
    """dataset/datasets.py's three draws, restated literally: generate_scale_label's randint (157-158 / 39-40), the two offset
    randints on the padded scaled size (197-199), np.random.choice(2) * 2 - 1 (205-206)."""
    random.seed(seed)
    np.random.seed(seed)
    k = random.randint(0, steps) if scale else None
    num, den = (first + k, 10) if scale else (1, 1)
    img_h, img_w = D.scaled_size(height, width, num, den)
    img_h, img_w = img_h + max(crop[0] - img_h, 0), img_w + max(crop[1] - img_w, 0)
    h_off = random.randint(0, img_h - crop[0])
    w_off = random.randint(0, img_w - crop[1])
    flip = np.random.choice(2) * 2 - 1 if mirror else 1
    return num, den, h_off, w_off, flip == -1


@pytest.mark.parametrize("seed", [0, 1, 2, 7, 1234, 99991])
def test_draw_params_makes_the_references_draws_in_its_order(seed):
    from ccnet_amd import augment
    for size, crop, scales, kw in (((1024, 2048), (769, 769), augment.CITYSCAPES_SCALES, {}),
                                   ((375, 500), (321, 321), augment.VOC_SCALES, {}),
                                   ((200, 300), (321, 321), augment.VOC_SCALES, {}),
                                   ((1024, 2048), (769, 769), augment.CITYSCAPES_SCALES, {"scale": False}),
                                   ((1024, 2048), (769, 769), augment.CITYSCAPES_SCALES, {"mirror": False})):
        want = reference_draws(seed, *size, crop, scales[0], scales[1], **kw)
        random.seed(seed)
        np.random.seed(seed)
        p = augment.draw_params(*size, crop, scales=scales, **kw)
        assert (p.num, p.den, p.h_off, p.w_off, p.mirror) == want
        assert (p.hz, p.wz) == D.scaled_size(*size, p.num, p.den)
        # and the generators stand where the reference's would: the next draws agree too
        after = (random.random(), np.random.random())
        reference_draws(seed, *size, crop, scales[0], scales[1], **kw)
        assert after == (random.random(), np.random.random())
    assert augment.CITYSCAPES_SCALES == (7, 14, 10) and augment.VOC_SCALES == (5, 11, 10)


def test_both_mirror_draws_and_every_scale_step_occur():
    from ccnet_amd import augment
    random.seed(3)
    np.random.seed(3)
    drawn = [augment.draw_params(1024, 2048, (769, 769)) for _ in range(400)]
    assert {p.num for p in drawn} == set(range(7, 22)) and {p.den for p in drawn} == {10}
    assert {p.mirror for p in drawn} == {False, True}


def test_cityscapes_table_is_the_references_map():
    from ccnet_amd import augment
    table = augment.CITYSCAPES_ID_TO_TRAINID
    assert table.dtype == np.uint8 and table.shape == (256,) and np.array_equal(table, D.cityscapes_table())
    assert sorted(set(table[:34]) - {255}) == list(range(19)) and table[7] == 0 and table[33] == 18 and table[0] == 255
    assert np.array_equal(table[34:], np.arange(34, 256))
    assert augment.cityscapes_table(250)[0] == 250 and augment.cityscapes_table(250)[7] == 0


def test_csdataset_decodes_draws_and_collates_and_the_kernel_finishes_the_batch(tmp_path, emu):
    from ccnet_amd import augment
    root = str(tmp_path)
    list_path, arrays = D.write_tiny_cityscapes(root, [(20, 30), (9, 11), (19, 29)])
    ds = augment.CSDataSet(root, list_path, crop_size=(16, 16), mean=D.MEAN)
    assert len(ds) == 3 and len(augment.CSDataSet(root, list_path, max_iters=7, crop_size=(16, 16))) == 9
    random.seed(11)
    np.random.seed(11)
    samples = [ds[k] for k in range(3)]
    random.seed(11)
    np.random.seed(11)
    for k, (frame, label, params, size, name) in enumerate(samples):
        assert frame.dtype == label.dtype == np.uint8
        assert np.array_equal(frame, arrays[k][0]) and np.array_equal(label, arrays[k][1])          # R, G, B as written
        assert params == augment.draw_params(*label.shape, (16, 16)) and isinstance(params, augment.AugmentParams)
        assert tuple(size) == frame.shape and name == f"f{k}_gtFine_labelIds"
    batch = augment.collate(samples, pin=False)
    frames, labels = [a[0] for a in arrays], [a[1] for a in arrays]
    mine = [(p.num, p.den, p.h_off, p.w_off, int(p.mirror)) for p in batch["params"]]
    assert np.array_equal(batch["desc"].numpy(), D.descriptors(frames, mine))
    assert np.array_equal(batch["frames"].numpy(), np.concatenate([f.reshape(-1) for f in frames]))
    assert np.array_equal(batch["labels"].numpy(), np.concatenate([l.reshape(-1) for l in labels]))
    assert batch["name"] == [s[4] for s in samples] and batch["size"].shape == (3, 3)
    aug = ds.device_augment()
    assert (aug.crop_h, aug.crop_w, aug.source_order, aug.ignore_label) == (16, 16, "rgb", 255) and aug.mean == D.MEAN
    assert np.array_equal(aug.label_table.numpy(), D.cityscapes_table())
    # the kernel (its sources in the emulator), told that the frames are R, G, B, finishes what the dataset started
    code, images, out, intact = D.run_raw(emu, HostMemory(), frames, labels, mine, (16, 16),
                                          aug.label_table.numpy(), mean=aug.mean, source_rgb=aug.source_order == "rgb",
                                          desc=batch["desc"].numpy())
    assert code == 0 and intact
    D.assert_bit_exact(images, out, *D.augment_batch(frames, labels, mine, (16, 16), table=D.cityscapes_table()))


def test_vocdataset_reads_the_references_layout(tmp_path):
    from PIL import Image
    from ccnet_amd import augment
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    frame, label = D.make_frame(12, 17, 3), D.make_label(12, 17, 3, ids=tuple(range(21)) + (255,))
    Image.fromarray(frame, "RGB").save(os.path.join(root, "JPEGImages", "2007_000032.jpg"), quality=95)
    Image.fromarray(label, "L").save(os.path.join(root, "SegmentationClassAug", "2007_000032.png"))
    with open(os.path.join(root, "train_aug.txt"), "w") as f:
        f.write("2007_000032\n")
    ds = augment.VOCDataSet(root, os.path.join(root, "train_aug.txt"), crop_size=(8, 8), mean=D.MEAN, mirror=False)
    random.seed(2)
    got_frame, got_label, params, size, name = ds[0]
    assert got_frame.shape == (12, 17, 3) and got_frame.dtype == np.uint8 and np.array_equal(got_label, label)
    assert name == "2007_000032" and tuple(size) == (12, 17, 3)
    assert params.den == 10 and 5 <= params.num <= 16 and params.mirror is False
    assert ds.device_augment().label_table is None


def test_public_layer_refuses_cpu_tensors_and_bad_arguments():
    from ccnet_amd import augment
    frames, labels, samples, crop, table = D.build_case("batch_mixed")
    params = [augment.AugmentParams(n, d, *D.scaled_size(*l.shape, n, d), ho, wo, bool(m))
              for l, (n, d, ho, wo, m) in zip(labels, samples)]
    fbuf, lbuf, desc = augment.pack(frames, labels, params)
    assert np.array_equal(desc.numpy(), D.descriptors(frames, samples)) and fbuf.numel() == 2055 and lbuf.numel() == 685
    aug = augment.DeviceAugment(crop, D.MEAN, label_table=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(fbuf, lbuf, desc)
    with pytest.raises(RuntimeError, match="no CPU"):
        augment.DevicePrefetcher([], aug, "cpu")
    with pytest.raises(ValueError, match="source_order"):
        augment.DeviceAugment(crop, D.MEAN, source_order="gbr")
    with pytest.raises(ValueError, match="three means"):
        augment.DeviceAugment(crop, (1.0, 2.0))
    with pytest.raises(ValueError, match="256"):
        augment.DeviceAugment(crop, D.MEAN, label_table=np.arange(19))
    with pytest.raises(ValueError, match="uint8"):
        augment.pack([frames[0].astype(np.float32)], labels[:1], params[:1])
    import ccnet_amd
    assert ccnet_amd.DeviceAugment is augment.DeviceAugment and ccnet_amd.augment is augment
    assert ccnet_amd.scaled_size is ccnet_amd.evaluate.scaled_size            # the evaluator's export stays what it was


def test_entry_point_checks_its_arguments_without_a_device(lib):
    frames, labels, samples, crop, table = D.build_case("s21_far")
    good = D.descriptors(frames, samples)
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)                       # never dereferenced: every call below fails its checks first

    def call(desc, B=1, ch=16, cw=16, fbytes=1800, lbytes=600, ptrs=(p, p, p, p, p)):
        d = np.ascontiguousarray(desc, np.int32)
        f, l, dd, img, out = ptrs
        return lib.ccnet_augment_crop_u8(f, fbytes, l, lbytes, d.ctypes.data, dd, None, img, out, B, ch, cw, 0.0, 0.0, 0.0, 255,
                                         1, None)

    for kw in ({"B": 0}, {"B": 65536}, {"ch": 0}, {"cw": 0}, {"ch": 65536}, {"B": 4, "ch": 20000, "cw": 20000}):
        assert call(good, **kw) == -1 and "unsupported shape" in lib.last_error(), kw
    for k in range(5):
        ptrs = tuple(None if j == k else p for j in range(5))
        assert call(good, ptrs=ptrs) == -2 and "NULL" in lib.last_error()
    for column, value, word in ((5, 1025, "scale"), (5, 0, "scale"), (6, 1025, "scale"), (6, 0, "scale"), (2, 0, "frame"),
                                (4, 29, "frame"), (7, 41, "scaled size"), (8, 64, "scaled size"), (9, 27, "offset"),
                                (9, -1, "offset"), (10, 48, "offset"), (11, 2, "mirror"), (0, -3, "outside"), (1, 1, "outside"),
                                (0, 1, "outside")):
        desc = good.copy()
        desc[0, column] = value
        assert call(desc) == -1 and word in lib.last_error(), (column, value, lib.last_error())
    huge = good.copy()
    huge[0, 2:5] = [64, 64, 64]
    huge[0, 5:9] = [1024, 1, 65536, 65536]
    assert call(huge, fbytes=3 * 4096, lbytes=4096) == -1 and "unsupported frame" in lib.last_error()
    assert call(good, fbytes=1799) == -1 and call(good, lbytes=599) == -1 and "outside its buffer" in lib.last_error()


FIFTEEN = [(7 + k, 10) for k in range(15)]


def test_oracle_image_equals_rounded_float64_interpolate_away_from_ties():
    """20 x 30 frames at the fifteen recipe scales (every Hs * f and Ws * f is an integer): the oracle's grey levels against
    rint(F.interpolate(float64, bilinear, align_corners=False)) wherever the float64 value is not an exact .5 tie."""
    import torch.nn.functional as F
    compared = total = 0
    for k, (num, den) in enumerate(FIFTEEN):
        frame = D.make_frame(20, 30, 300 + k)
        hz, wz = D.scaled_size(20, 30, num, den)
        assert (hz * den, wz * den) == (20 * num, 30 * num)
        q, _ = D.resized_levels(frame, num, den, np.arange(hz), np.arange(wz))
        x = torch.from_numpy(frame.astype(np.float64)).permute(2, 0, 1)[None]
        y = F.interpolate(x, scale_factor=num / den, mode="bilinear", align_corners=False, recompute_scale_factor=False)
        assert tuple(y.shape[2:]) == (hz, wz)
        y = y[0].permute(1, 2, 0).numpy()
        tie = np.abs(y - np.floor(y) - 0.5) < 1e-9
        mismatches = int((np.rint(y)[~tie] != q[~tie]).sum())
        kept = int((~tie).sum())
        print(f"scale {num}/{den}: {hz} x {wz}, {y.size} elements, {int(tie.sum())} ties left out, {mismatches} mismatches")
        assert mismatches == 0
        # at a tie the contract rounds half up
        assert np.array_equal(q[tie], np.floor(y[tie]) + 1)
        compared, total = compared + kept, total + y.size
    print(f"compared {compared} of {total} elements")
    assert total == 57960 and compared >= 0.9 * total            # (a single scale may leave out more: 3/2 has about 10 % ties)


def test_oracle_numerator_stays_inside_32_bits_at_the_largest_ratios():
    top = 0
    for k, (num, den) in enumerate([(1024, 1), (1023, 1024), (1024, 1023), (1021, 7), (1024, 3), (513, 512), (1019, 1024),
                                    (1024, 1024), (1023, 2)]):
        frame = D.make_frame(5, 6, 500 + k)
        frame.reshape(-1)[::7] = 255
        hz, wz = D.scaled_size(5, 6, num, den)
        _, n = D.resized_levels(frame, num, den, np.arange(min(hz, 600)), np.arange(min(wz, 600)))
        top = max(top, n)
    assert top == 2048 * 2048 * 255 + 2048 * 2048 // 2 < 2 ** 32          # reached: a 255 pixel sampled at num = 1024


def test_train_driver_takes_device_augment_with_every_criterion_flag_and_refuses_the_cpu():
    from ccnet_amd.train_synthetic import build_parser, parse_args, run
    assert build_parser().parse_args([]).device_augment is False
    for flags in ([], ["--ohem"], ["--lovasz"], ["--fused-dsn"], ["--fused-ohem"], ["--fused-lovasz"], ["--ohem", "--fused-dsn"],
                  ["--abn", "device"]):
        args = parse_args(["--device-augment"] + flags)
        assert args.device_augment and args.augment_frame == [1024, 2048]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(build_parser().parse_args(["--device-augment", "--cpu", "--steps", "1", "--warmup", "0"]),
            model_factory=lambda: torch.nn.Identity())


LOADER_SIZES = [(20, 30), (9, 11), (19, 29), (7, 5), (12, 17), (20, 30)]


def test_collate_in_dataloader_workers_never_touches_the_device_api(tmp_path, monkeypatch):
    """CSDataSet through DataLoader(num_workers=2, collate_fn=collate), the route a real run takes: the workers' batches are
    those of the same draws in this process, they arrive unpinned, and no worker calls into torch.cuda (the stand-ins below
    are inherited by the forked workers and raise there)."""
    from ccnet_amd import augment
    parent = os.getpid()

    def guard(real):
        def call(*a, **k):
            if os.getpid() != parent:
                raise AssertionError("a DataLoader worker called into torch.cuda")
            return real(*a, **k)
        return call
    for name in ("is_available", "device_count", "_lazy_init", "init"):
        monkeypatch.setattr(torch.cuda, name, guard(getattr(torch.cuda, name)))
    root = str(tmp_path)
    list_path, arrays = D.write_tiny_cityscapes(root, LOADER_SIZES)
    ds = augment.CSDataSet(root, list_path, crop_size=(16, 16), mean=D.MEAN)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=augment.collate, num_workers=2,
                                         worker_init_fn=D.seed_worker, multiprocessing_context="fork")
    got = list(loader)
    assert len(got) == 3
    want = D.replay_worker_draws(LOADER_SIZES, (16, 16), batch_size=2, num_workers=2)
    for k, batch in enumerate(got):
        pairs = arrays[2 * k:2 * k + 2]
        assert not batch["frames"].is_pinned() and not batch["labels"].is_pinned() and not batch["desc"].is_pinned()
        assert batch["params"] == want[k] and batch["name"] == [f"f{2 * k + j}_gtFine_labelIds" for j in range(2)]
        assert np.array_equal(batch["frames"].numpy(), np.concatenate([f.reshape(-1) for f, _ in pairs]))
        assert np.array_equal(batch["labels"].numpy(), np.concatenate([l.reshape(-1) for _, l in pairs]))
        mine = [(p.num, p.den, p.h_off, p.w_off, int(p.mirror)) for p in want[k]]
        assert np.array_equal(batch["desc"].numpy(), D.descriptors([f for f, _ in pairs], mine))


def test_collate_ignores_pin_inside_a_worker(monkeypatch):
    from ccnet_amd import augment
    frames, labels, samples, crop, _ = D.build_case("batch_mixed")
    params = [augment.AugmentParams(n, d, *D.scaled_size(*l.shape, n, d), ho, wo, bool(m))
              for l, (n, d, ho, wo, m) in zip(labels, samples)]
    rows = list(zip(frames, labels, params, [np.array(f.shape) for f in frames], ["a", "b", "c"]))
    asked = []
    monkeypatch.setattr(augment, "pack", lambda f, l, p, pin=False: asked.append(pin) or ("f", "l", "d"))
    augment.collate(rows)
    augment.collate(rows, pin=True)
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    augment.collate(rows, pin=True)
    assert asked == [False, True, False]
