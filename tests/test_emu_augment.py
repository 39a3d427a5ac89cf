"""The input-pipeline kernel sources (ccnet_amd/csrc_augment/) run in the SIMT emulator (tests/emu/ + the twin header of
tests/emu_augment/) through the same C ABI as on the device, bit-exactly against the integer oracle of tests/augment_oracle.py
on guarded host buffers."""
import numpy as np
import pytest

import augment_oracle as D
import lib_checks as L
from guarded_memory import HostMemory


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._augment_lib import AugmentLibrary
    return AugmentLibrary(L.build_shared_scaffold_emu("augment"))


@pytest.mark.parametrize("name", list(D.CASES))
def test_emulated_kernel_matches_the_oracle_bit_exactly(emu, name):
    frames, labels, samples, crop, table = D.build_case(name)
    code, images, out, intact = D.run_raw(emu, HostMemory(), frames, labels, samples, crop, table)
    assert code == 0, emu.last_error()
    assert intact
    assert not np.isnan(images).any() and (out >= 0).all()          # every element written
    D.assert_bit_exact(images, out, *D.augment_batch(frames, labels, samples, crop, table=table))


def test_emulated_rgb_and_bgr_sources_give_the_same_output(emu):
    frames, labels, samples, crop, table = D.build_case("batch_mixed")
    a = D.run_raw(emu, HostMemory(), frames, labels, samples, crop, table, source_rgb=True)
    b = D.run_raw(emu, HostMemory(), [f[:, :, ::-1].copy() for f in frames], labels, samples, crop, table, source_rgb=False)
    assert a[0] == b[0] == 0 and a[3] and b[3]
    D.assert_bit_exact(a[1], a[2], b[1], b[2])


def test_emulated_identity_is_frame_minus_mean_and_the_tables_labels(emu):
    frames, labels, samples, crop, table = D.build_case("identity")
    (num, den, h_off, w_off, mirror), (ch, cw) = samples[0], crop
    assert (num, den, mirror) == (1, 1, 0)
    code, images, out, intact = D.run_raw(emu, HostMemory(), frames, labels, samples, crop, table)
    assert code == 0 and intact
    window = frames[0][h_off:h_off + ch, w_off:w_off + cw, ::-1].transpose(2, 0, 1).astype(np.float32)
    want = window - np.array(D.MEAN, np.float32)[:, None, None]
    assert np.array_equal(images[0], want)
    assert np.array_equal(out[0], table[labels[0][h_off:h_off + ch, w_off:w_off + cw]].astype(np.int64))
    assert set(np.unique(labels[0])) == set(range(34)) | {255} and set(np.unique(out[0])) <= set(range(19)) | {255}


def test_emulated_limit_violations_are_refused_and_nothing_is_written(emu):
    frames, labels, samples, crop, table = D.build_case("s21_far")
    good = D.descriptors(frames, samples)
    for column, value, word in ((5, 1025, "scale"), (6, 0, "scale"), (9, good[0, 9] + 1, "offset"), (10, -1, "offset"),
                                (7, good[0, 7] + 1, "scaled size"), (11, 2, "mirror"), (0, 3, "outside its buffer")):
        desc = good.copy()
        desc[0, column] = value
        code, images, out, intact = D.run_raw(emu, HostMemory(), frames, labels, samples, crop, table, desc=desc)
        assert code == -1 and word in emu.last_error() and emu.last_error().startswith("ccnet_augment:"), emu.last_error()
        assert intact and np.isnan(images).all() and (out == -1).all()
