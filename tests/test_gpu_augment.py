"""The input-pipeline kernel on the device (libccnet_augment.so): the case table of tests/augment_oracle.py through the C ABI on
guarded buffers and through ccnet_amd.augment.DeviceAugment, bit-exactly against the integer oracle; refusals that launch
nothing; the prefetcher; the training driver's --device-augment."""
import math

import numpy as np
import pytest
import torch

import augment_oracle as D
from guarded_memory import DeviceMemory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ccnet_amd import _augment_lib
    return _augment_lib.get_lib()


@pytest.fixture(scope="module")
def expected():
    """The oracle's answer per case, computed once and left unchanged"""
    out = {}
    for name in D.CASES:
        frames, labels, samples, crop, table = D.build_case(name)
        out[name] = D.augment_batch(frames, labels, samples, crop, table=table)
    return out


def to_params(labels, samples):
    from ccnet_amd import augment
    return [augment.AugmentParams(n, d, *D.scaled_size(*l.shape, n, d), ho, wo, bool(m)) for l, (n, d, ho, wo, m) in zip(labels, samples)]


def through_module(name, source_order="rgb"):
    from ccnet_amd import augment
    frames, labels, samples, crop, table = D.build_case(name)
    if source_order == "bgr":
        frames = [f[:, :, ::-1].copy() for f in frames]
    fbuf, lbuf, desc = augment.pack(frames, labels, to_params(labels, samples))
    aug = augment.DeviceAugment(crop, D.MEAN, D.IGNORE, table, source_order)
    images, out = aug(fbuf.cuda(), lbuf.cuda(), desc)
    assert images.dtype == torch.float32 and out.dtype == torch.int64 and images.is_cuda and out.is_cuda
    assert tuple(images.shape) == (len(frames), 3) + crop and tuple(out.shape) == (len(frames),) + crop
    return images.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("name", list(D.CASES))
def test_c_abi_matches_the_oracle_bit_exactly_on_guarded_buffers(lib, expected, name):
    frames, labels, samples, crop, table = D.build_case(name)
    code, images, out, intact = D.run_raw(lib, DeviceMemory(), frames, labels, samples, crop, table)
    assert code == 0, lib.last_error()
    assert intact
    assert not np.isnan(images).any() and (out >= 0).all()          # every element of the NaN / -1 outputs written
    D.assert_bit_exact(images, out, *expected[name])


@pytest.mark.parametrize("name", list(D.CASES))
def test_device_augment_matches_the_oracle_bit_exactly(expected, name):
    D.assert_bit_exact(*through_module(name), *expected[name])


def test_rgb_and_bgr_sources_give_the_same_output(expected):
    for name in ("batch_mixed", "s21_far_mirror"):
        D.assert_bit_exact(*through_module(name, "bgr"), *expected[name])


def test_identity_is_frame_minus_mean_and_the_tables_labels():
    frames, labels, samples, crop, table = D.build_case("identity")
    (num, den, h_off, w_off, mirror), (ch, cw) = samples[0], crop
    images, out = through_module("identity")
    window = frames[0][h_off:h_off + ch, w_off:w_off + cw, ::-1].transpose(2, 0, 1).astype(np.float32)
    assert np.array_equal(images[0], window - np.array(D.MEAN, np.float32)[:, None, None])
    assert np.array_equal(out[0], table[labels[0][h_off:h_off + ch, w_off:w_off + cw]].astype(np.int64))


def test_a_second_run_is_bitwise_the_first_and_a_given_device_table_changes_nothing():
    from ccnet_amd import augment
    frames, labels, samples, crop, table = D.build_case("batch_mixed")
    fbuf, lbuf, desc = augment.pack(frames, labels, to_params(labels, samples))
    aug = augment.DeviceAugment(crop, D.MEAN, D.IGNORE, table)
    f, l = fbuf.cuda(), lbuf.cuda()
    a = aug(f, l, desc)
    b = aug(f, l, desc)
    c = aug(f, l, desc, desc_device=desc.cuda())
    for other in (b, c):
        assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1], other[1])


def test_limit_violations_return_an_error_and_launch_nothing(lib):
    frames, labels, samples, crop, table = D.build_case("s21_far")
    good = D.descriptors(frames, samples)
    for column, value, word in ((5, 1025, "scale"), (9, good[0, 9] + 1, "offset"), (10, good[0, 10] + 1, "offset")):
        desc = good.copy()
        desc[0, column] = value
        code, images, out, intact = D.run_raw(lib, DeviceMemory(), frames, labels, samples, crop, table, desc=desc)
        assert code == -1 and word in lib.last_error(), lib.last_error()
        assert intact and np.isnan(images).all() and (out == -1).all()
    from ccnet_amd import _augment_lib, augment
    fbuf, lbuf, desc = augment.pack(frames, labels, to_params(labels, samples))
    desc[0, _augment_lib.NUM] = 1025
    with pytest.raises(_augment_lib.AugmentError, match="scale 1025/10"):
        augment.DeviceAugment(crop, D.MEAN, D.IGNORE, table)(fbuf.cuda(), lbuf.cuda(), desc)


def test_prefetcher_returns_the_batches_of_the_plain_loop():
    from ccnet_amd import augment
    names = ["batch_mixed", "s07_far_mirror", "batch_mixed"]
    batches, plain = [], []
    aug = augment.DeviceAugment((16, 16), D.MEAN, D.IGNORE, D.cityscapes_table())
    for k, name in enumerate(names):
        frames, labels, samples, crop, _ = D.build_case(name, seed=900 + 16 * k)
        assert crop == (16, 16)
        params = to_params(labels, samples)
        sizes = [np.array(f.shape) for f in frames]
        batches.append(augment.collate(list(zip(frames, labels, params, sizes, [f"{name}{j}" for j in range(len(frames))]))))
        assert not batches[-1]["frames"].is_pinned()        # collate leaves pinning to the consumer: here, the prefetcher
        plain.append(aug(batches[-1]["frames"].cuda(), batches[-1]["labels"].cuda(), batches[-1]["desc"]))
        D.assert_bit_exact(plain[-1][0].cpu().numpy(), plain[-1][1].cpu().numpy(),
                           *D.augment_batch(frames, labels, samples, crop, table=D.cityscapes_table()))
    got = list(augment.DevicePrefetcher(batches, aug, "cuda:0"))
    assert len(got) == 3
    for (images, out, batch), (want_images, want_out), given in zip(got, plain, batches):
        assert batch is given
        assert torch.equal(images.view(torch.int32), want_images.view(torch.int32)) and torch.equal(out, want_out)


@pytest.mark.parametrize("pin_memory", [True, False], ids=["loader_pins", "prefetcher_pins"])
def test_prefetcher_over_a_dataloader_with_workers_returns_the_plain_loops_batches(tmp_path, pin_memory):
    """The route a real run takes: CSDataSet -> DataLoader(num_workers=2, collate_fn=collate) -> DevicePrefetcher.  The device
    copies start from pinned memory either way (the loader's pin thread, or the prefetcher's own pinning), and the batches
    are those of a plain loop over the same loader, which are the oracle's."""
    from ccnet_amd import augment
    sizes = [(20, 30), (9, 11), (19, 29), (7, 5), (12, 17), (20, 30)]
    list_path, arrays = D.write_tiny_cityscapes(str(tmp_path), sizes)
    ds = augment.CSDataSet(str(tmp_path), list_path, crop_size=(16, 16), mean=D.MEAN)
    aug = ds.device_augment()

    def loader():
        return torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=augment.collate, num_workers=2, pin_memory=pin_memory,
                                           worker_init_fn=D.seed_worker, multiprocessing_context="fork")
    plain = []
    for k, batch in enumerate(loader()):
        assert batch["frames"].is_pinned() == batch["labels"].is_pinned() == batch["desc"].is_pinned() == pin_memory
        assert augment._pinned(batch["frames"]).is_pinned() and augment._pinned(batch["desc"]).is_pinned()
        assert (augment._pinned(batch["frames"]) is batch["frames"]) == pin_memory
        images, out = aug(batch["frames"].cuda(), batch["labels"].cuda(), batch["desc"])
        mine = [(p.num, p.den, p.h_off, p.w_off, int(p.mirror)) for p in batch["params"]]
        frames, labels = [a[0] for a in arrays[2 * k:2 * k + 2]], [a[1] for a in arrays[2 * k:2 * k + 2]]
        D.assert_bit_exact(images.cpu().numpy(), out.cpu().numpy(),
                           *D.augment_batch(frames, labels, mine, (16, 16), table=D.cityscapes_table()))
        plain.append((images, out, batch["params"], batch["name"]))
    assert [p[2] for p in plain] == D.replay_worker_draws(sizes, (16, 16), batch_size=2, num_workers=2)
    got = list(augment.DevicePrefetcher(loader(), aug, "cuda:0"))
    assert len(got) == len(plain) == 3
    for (images, out, batch), (want_images, want_out, params, names) in zip(got, plain):
        assert batch["params"] == params and batch["name"] == names
        assert torch.equal(images.view(torch.int32), want_images.view(torch.int32)) and torch.equal(out, want_out)


class ToySegmenter(torch.nn.Module):
    """Two 1/8-resolution heads and the stock CriterionDSN: the shape of the real model's output, nothing of its cost"""

    def __init__(self):
        super().__init__()
        from ccnet_amd.segmodel import CriterionDSN
        self.main = torch.nn.Linear(3, 19)
        self.aux = torch.nn.Linear(3, 19)
        self.criterion = CriterionDSN()

    def forward(self, images, labels):
        x = torch.nn.functional.avg_pool2d(images / 64, 8).permute(0, 2, 3, 1)                  # (B, h, w, 3)
        return self.criterion([self.main(x).permute(0, 3, 1, 2), self.aux(x).permute(0, 3, 1, 2)], labels)


def test_train_driver_with_device_augment_runs_two_steps_to_a_finite_loss():
    from ccnet_amd import train_synthetic as T
    args = T.parse_args(["--device-augment", "--augment-frame", "40", "64", "--size", "33", "--steps", "2", "--warmup", "0",
                         "--batch-per-gpu", "2", "--lr", "1e-3"])
    res = T.run(args, model_factory=ToySegmenter, quiet=True)
    assert res["steps"] == 2 and res["value"] > 0 and math.isfinite(res["final_loss"]) and res["final_loss"] > 0
    assert "DeviceAugment" in res["data"]
    source = T.AugmentedSource(2, (40, 64), 33, torch.device("cuda", 0), seed=0)
    images, labels = source.next()
    assert tuple(images.shape) == (2, 3, 33, 33) and set(labels.unique().tolist()) <= set(range(19)) | {255}
    assert torch.isfinite(images).all() and float(images.min()) >= -123.0 and float(images.max()) <= 255.0
