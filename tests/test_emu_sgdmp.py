"""The mixed-precision optimiser kernel sources (ccnet_amd/csrc_sgdmp/) run in the SIMT emulator (tests/emu/ + the twin header
of tests/emu_sgdmp/) through the same C ABI as on the device, bit-exactly against the oracle of tests/sgdmp_oracle.py on
guarded host buffers; a table of float32 rows against the emulator build of ccnet_sgd_step on the same inputs."""
import numpy as np
import pytest

import lib_checks as L
import sgd_oracle as S
import sgdmp_oracle as M
from guarded_memory import HostMemory


@pytest.fixture(scope="module")
def emu():
    from ccnet_amd._sgdmp_lib import SgdmpLibrary
    return SgdmpLibrary(L.build_shared_scaffold_emu("sgdmp"))


@pytest.fixture(scope="module")
def emu_sgd():
    from ccnet_amd._sgd_lib import SgdLibrary
    return SgdLibrary(L.build_shared_scaffold_emu("sgd"))


@pytest.mark.parametrize("name", list(M.CASES))
def test_emulated_kernel_matches_the_oracle_bit_exactly(emu, name):
    case = M.build_case(name)
    code, got, intact = M.run_raw(emu, HostMemory(), case)
    assert code == 0, emu.last_error()
    assert intact
    M.assert_matches(case, got)


def test_emulated_rounding_case_gives_the_hand_values(emu):
    case = M.build_case("rounding")
    code, got, intact = M.run_raw(emu, HostMemory(), case)
    assert code == 0 and intact
    want = {u: h for u, h in M.ROUNDING if (u & 0x7FFFFFFF) != 0x7F800000}          # (0 * inf: a NaN, see the oracle)
    seen = set()
    for t in range(3):
        for u, h in zip(case["m"][t].view(np.uint32).tolist(), got[0][t].tolist()):
            if u in want:
                assert h == want[u], (t, hex(u), hex(h))
                seen.add((t, u))
        finite = np.isfinite(case["m"][t])
        assert np.array_equal(got[3][t].view(np.uint32)[finite], case["m"][t].view(np.uint32)[finite])      # m' = m, subnormals and -0 kept
    assert len(seen) == 3 * len(want)                                                # every entry on every row


def test_emulated_master_rows_never_read_p_and_skipped_rows_keep_everything(emu):
    case = M.build_case("null_grad")
    code, got, intact = M.run_raw(emu, HostMemory(), case)
    assert code == 0 and intact
    for t in case["null"]:
        assert M.same_bits(got[0][t], case["p"][t]) and M.same_bits(got[2][t], case["b"][t]) and got[1][t] is None
        assert case["m"][t] is None or M.same_bits(got[3][t], case["m"][t])
    assert not M.is_nan16(got[0][0]).any() and M.is_nan16(case["p"][0]).all()        # p started as NaNs: it was written, not read
    on, off = M.build_case("zero_on"), M.build_case("zero_off")
    g_on, g_off = M.run_raw(emu, HostMemory(), on)[1][1], M.run_raw(emu, HostMemory(), off)[1][1]
    assert all(g.dtype == np.uint16 and not g.any() for g in g_on)                   # +0: every bit clear
    assert all(M.same_bits(g, keep) for g, keep in zip(g_off, off["g"]))


@pytest.mark.parametrize("name", list(S.CASES))
def test_emulated_float32_rows_are_bit_identical_to_ccnet_sgd_step(emu, emu_sgd, name):
    scase = S.build_case(name)
    code, theirs, intact = S.run_raw(emu_sgd, HostMemory(), scase)
    assert code == 0 and intact
    code, mine, intact = M.run_raw(emu, HostMemory(), M.from_sgd_case(scase))
    assert code == 0 and intact, emu.last_error()
    assert mine[4] == theirs[3]
    for key, a_list, b_list in zip("pgb", mine[:3], theirs[:3]):
        for t, (a, b) in enumerate(zip(a_list, b_list)):
            assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32)), (key, t)
