"""The optimiser kernel sources (ccnet_amd/csrc_sgd/) run in the SIMT emulator (tests/emu/ + the twin header of tests/emu_sgd/)
through the same C ABI as on the device, bit-exactly against the float32 oracle of tests/sgd_oracle.py on guarded host
buffers."""
import numpy as np
import pytest

import lib_checks as L
import sgd_oracle as S
from guarded_memory import HostMemory


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._sgd_lib import SgdLibrary
    return SgdLibrary(L.build_shared_scaffold_emu("sgd"))


@pytest.mark.parametrize("name", list(S.CASES))
def test_emulated_kernel_matches_the_oracle_bit_exactly(emu, name):
    case = S.build_case(name)
    code, got, intact = S.run_raw(emu, HostMemory(), case)
    assert code == 0, emu.last_error()
    assert intact
    S.assert_matches(case, got)


def test_emulated_null_gradient_tensors_and_kept_gradients_are_bitwise_untouched(emu):
    case = S.build_case("null_grad")
    code, got, intact = S.run_raw(emu, HostMemory(), case)
    assert code == 0 and intact
    for t in case["null"]:
        assert S.same_bits(got[0][t], case["p"][t]) and S.same_bits(got[2][t], case["b"][t]) and got[1][t] is None
    assert not S.same_bits(got[0][0], case["p"][0])
    on, off = S.build_case("zero_on"), S.build_case("zero_off")
    g_on, g_off = S.run_raw(emu, HostMemory(), on)[1][1], S.run_raw(emu, HostMemory(), off)[1][1]
    assert all(not g.any() and not np.signbit(g).any() for g in g_on)
    assert all(S.same_bits(g, keep) for g, keep in zip(g_off, off["g"]))


def test_emulated_schedule_picks_its_entry_scales_it_per_group_and_advances_the_counter(emu):
    seen = {}
    for s in (0, 3, 9):
        case = dict(S.build_case("mult_0"), counter=s)              # the same inputs at three counter values
        code, got, intact = S.run_raw(emu, HostMemory(), case)
        assert code == 0 and intact and got[3] == s + 1
        seen[s] = got
        assert float(S.group_lr(case, 0)) == float(np.float32(S.SCHEDULE[min(s, 3)]))          # a multiplier of 1.0 is exact
        assert S.group_lr(case, 1) == np.float32(S.SCHEDULE[min(s, 3)]) * np.float32(10.0)
    # 3 and 9 read the same (last) entry; 0 reads another
    assert all(S.same_bits(a, b) for a, b in zip(seen[3][0], seen[9][0]))
    assert not S.same_bits(seen[0][0][0], seen[3][0][0])
