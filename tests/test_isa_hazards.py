"""The hand-waited LDS reads of the projection GEMMs, checked where a missing wait shows: in the gfx950 instruction stream.

tests/isa_hazards.py walks the assembly of every kernel of the six libraries (compiled here with the product's own flags,
device only) and reports every instruction that touches the destination registers of an LDS read that may still be in flight.
The SIMT emulator cannot see this (its reads are synchronous) and a device run passes whenever the LDS answers in time.  The
first half of this file pins the walk itself down on hand-written snippets; the second holds every kernel to zero findings."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import isa_hazards as H  # noqa: E402


def verdict(text):
    """(the texts of the flagged instructions, the final queue) of a snippet"""
    report, last = H.check_snippet(text)
    return [v.text for v in report], last


# ---------------------------------------------------------------------------------------------------------------------
# the walk on hand-written snippets
# ---------------------------------------------------------------------------------------------------------------------
def test_use_without_a_wait_is_flagged():
    got, _ = verdict("""
        ds_read_b128 v[4:7], v1
        v_add_f32 v9, v5, v8
        s_endpgm""")
    assert got == ["v_add_f32 v9, v5, v8"]
    report, _ = H.check_snippet("ds_read_b128 v[4:7], v1\nv_add_f32 v9, v5, v8\ns_endpgm", name="k")
    assert report == [H.Violation("k", "entry", "v_add_f32 v9, v5, v8", (5,))]


def test_use_after_a_full_wait_is_clean():
    got, last = verdict("""
        ds_read_b128 v[4:7], v1
        s_waitcnt lgkmcnt(0)
        v_add_f32 v9, v5, v8
        s_endpgm""")
    assert got == [] and last == ()


def _sixteen_reads():
    return "\n".join(f"ds_read_b128 v[{4 * i}:{4 * i + 3}], v100 offset:{16 * i}" for i in range(16))


def test_counted_wait_retires_the_oldest_reads_only():
    # reads 1..16 target v[0:3] .. v[60:63]; lgkmcnt(8) leaves reads 9..16 in flight
    head = _sixteen_reads() + "\ns_waitcnt lgkmcnt(8)\n"
    assert verdict(head + "v_mov_b32 v101, v31\ns_endpgm")[0] == []                              # the 8th read's last register
    assert verdict(head + "v_mov_b32 v101, v32\ns_endpgm")[0] == ["v_mov_b32 v101, v32"]       # the 9th read's first
    _, last = verdict(head + "s_endpgm")
    assert [sorted(e.regs) for e in last] == [list(range(4 * i, 4 * i + 4)) for i in range(8, 16)]


def test_a_copy_of_an_outstanding_destination_is_flagged():
    got, _ = verdict("""
        ds_read_b128 v[126:129], v1
        s_waitcnt vmcnt(0)
        v_mov_b64 v[106:107], v[126:127]
        s_waitcnt lgkmcnt(0)
        v_mov_b64 v[108:109], v[128:129]
        s_endpgm""")
    assert got == ["v_mov_b64 v[106:107], v[126:127]"]


def test_a_write_to_an_outstanding_destination_is_flagged():
    got, _ = verdict("""
        ds_read_b128 v[42:45], v1
        v_lshlrev_b32 v43, 2, v40
        s_endpgm""")
    assert got == ["v_lshlrev_b32 v43, 2, v40"]


def test_read_after_read_into_the_same_destination_is_clean():
    got, last = verdict("""
        ds_read_b128 v[4:7], v1
        ds_read_b128 v[4:7], v2 offset:2048
        s_endpgm""")
    assert got == [] and len(last) == 2
    # ... but an LDS instruction that READS an outstanding destination (address or data) is not
    assert verdict("ds_read_b128 v[4:7], v1\nds_read_b128 v[8:11], v4\ns_endpgm")[0] == ["ds_read_b128 v[8:11], v4"]
    assert verdict("ds_read_b128 v[4:7], v1\nds_write_b32 v2, v6\ns_endpgm")[0] == ["ds_write_b32 v2, v6"]


LOOP = """
        v_mov_b32 v20, 0
        ds_read_b128 v[4:7], v1
    .LBB0_1:
        v_add_f32 v20, v20, v4
        {before_read}
        ds_read_b128 v[4:7], v1 offset:64
        {after_read}
        s_add_i32 s4, s4, 1
        s_cmp_lt_i32 s4, s5
        s_cbranch_scc1 .LBB0_1
        s_waitcnt lgkmcnt(0)
        global_store_dword v[2:3], v20, off
        s_endpgm"""


def test_loop_back_edge_carries_an_outstanding_read_into_the_header():
    # the header's use is covered on entry (first iteration: also outstanding) and over the back edge
    got, _ = verdict(LOOP.format(before_read="s_waitcnt lgkmcnt(0)", after_read="s_nop 0"))
    assert got == ["v_add_f32 v20, v20, v4"]


def test_loop_with_the_wait_before_the_back_edge_is_clean():
    text = LOOP.format(before_read="s_nop 0", after_read="s_waitcnt lgkmcnt(0)")
    text = text.replace("ds_read_b128 v[4:7], v1\n", "ds_read_b128 v[4:7], v1\n        s_waitcnt lgkmcnt(0)\n", 1)
    assert verdict(text)[0] == []


def test_back_edge_alone_is_enough_to_flag():
    # entry is clean (waited before the loop); only the path over the back edge leaves the read in flight
    text = LOOP.format(before_read="s_nop 0", after_read="s_nop 0")
    text = text.replace("ds_read_b128 v[4:7], v1\n", "ds_read_b128 v[4:7], v1\n        s_waitcnt lgkmcnt(0)\n", 1)
    assert verdict(text)[0] == ["v_add_f32 v20, v20, v4"]


def test_diamond_with_a_wait_on_one_arm_is_flagged_at_the_join():
    got, _ = verdict("""
        ds_read_b128 v[4:7], v1
        s_cbranch_scc1 .LBB0_2
        s_waitcnt lgkmcnt(0)
        s_branch .LBB0_3
    .LBB0_2:
        s_nop 0
    .LBB0_3:
        v_add_f32 v9, v5, v8
        s_endpgm""")
    assert got == ["v_add_f32 v9, v5, v8"]
    # both arms wait: clean
    got, _ = verdict("""
        ds_read_b128 v[4:7], v1
        s_cbranch_scc1 .LBB0_2
        s_waitcnt lgkmcnt(0)
        s_branch .LBB0_3
    .LBB0_2:
        s_waitcnt vmcnt(3) lgkmcnt(0)
    .LBB0_3:
        v_add_f32 v9, v5, v8
        s_endpgm""")
    assert got == []


def test_scalar_loads_retire_at_zero_only():
    text = """
        ds_read_b128 v[0:3], v100
        ds_read_b128 v[4:7], v100 offset:16
        s_load_dwordx2 s[0:1], s[4:5], 0x0
        ds_read_b128 v[8:11], v100 offset:32
        ds_read_b128 v[12:15], v100 offset:48
        s_waitcnt lgkmcnt(2)
        {use}
        s_endpgm"""
    _, last = verdict(text.format(use="s_nop 0"))
    assert [(sorted(e.regs), e.scalar) for e in last] == [([], True), ([8, 9, 10, 11], False), ([12, 13, 14, 15], False)]
    assert verdict(text.format(use="v_mov_b32 v50, v7"))[0] == []               # the two oldest LDS reads have retired
    assert verdict(text.format(use="v_mov_b32 v50, v8"))[0] == ["v_mov_b32 v50, v8"]
    _, last = verdict(text.format(use="s_waitcnt lgkmcnt(0)"))
    assert last == ()
    for mn in ("s_buffer_load_dword s0, s[4:7], 0x0", "s_memtime s[0:1]", "s_memrealtime s[0:1]", "s_sendmsg sendmsg(MSG_INTERRUPT)",
               "flat_load_dword v60, v[62:63]"):
        _, last = verdict(mn + "\ns_waitcnt lgkmcnt(1)\ns_endpgm")
        assert [e.scalar for e in last] == [True], mn


def test_waits_without_an_lgkmcnt_field_retire_nothing():
    for wait in ("s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(2) expcnt(0)"):
        got, last = verdict(f"ds_read_b128 v[4:7], v1\n{wait}\nv_add_f32 v9, v5, v8\ns_endpgm")
        assert got == ["v_add_f32 v9, v5, v8"] and len(last) == 1, wait


def test_raw_immediate_waits_decode_bits_11_to_8():
    assert H.waitcnt_lgkm("0xc07f") == 0 and H.waitcnt_lgkm("0xc87f") == 8 and H.waitcnt_lgkm("49279") == 0
    assert H.waitcnt_lgkm("vmcnt(0)") is None and H.waitcnt_lgkm("vmcnt(1) lgkmcnt(3)") == 3
    head = _sixteen_reads()
    assert verdict(head + "\ns_waitcnt 0xc87f\nv_mov_b32 v101, v31\nv_mov_b32 v102, v32\ns_endpgm")[0] == ["v_mov_b32 v102, v32"]
    assert verdict(head + "\ns_waitcnt 0xc07f\nv_mov_b32 v102, v63\ns_endpgm")[0] == []


def test_stores_append_entries_without_destinations_and_the_queue_is_capped():
    got, last = verdict("ds_read_b128 v[4:7], v1\nds_write_b128 v2, v[8:11]\ns_waitcnt lgkmcnt(1)\nv_mov_b32 v0, v4\ns_endpgm")
    assert got == [] and [sorted(e.regs) for e in last] == [[]]
    text = "\n".join(f"ds_read_b32 v{i}, v200" for i in range(100)) + "\ns_endpgm"
    _, last = verdict(text)
    assert len(last) == H.QUEUE_CAP and set().union(*(e.regs for e in last)) == set(range(100))


def test_an_unresolved_branch_target_is_an_error():
    with pytest.raises(AssertionError):
        H.check_snippet("s_cbranch_scc1 .LBB9_9\ns_endpgm")


def test_functions_are_cut_at_their_type_directive_and_func_end():
    asm = """
        .text
        .type _Z1av,@function
_Z1av:
        ds_read_b32 v1, v0
        v_mov_b32 v2, v1
        s_endpgm
.Lfunc_end0:
        .size _Z1av, .Lfunc_end0-_Z1av
        .type _Z1bv,@function
_Z1bv:
        ds_read_b32 v1, v0
        s_waitcnt lgkmcnt(0)
        v_mov_b32 v2, v1
        s_endpgm
.Lfunc_end1:
        .type some_table,@object
some_table:
        .long 0
"""
    got = H.check_assembly(asm)
    assert sorted(got) == ["_Z1av", "_Z1bv"]
    assert [v.text for v in got["_Z1av"]] == ["v_mov_b32 v2, v1"] and got["_Z1bv"] == []


# ---------------------------------------------------------------------------------------------------------------------
# the product: every kernel of every library
# ---------------------------------------------------------------------------------------------------------------------
def _libraries():
    import __graft_entry__ as g
    return {"cca": (g.CSRC, "cca_api.hip", g.HIPCC_FLAGS), "ohem": (g.OHEM_CSRC, "ohem_api.hip", g.OHEM_HIPCC_FLAGS),
            "eval": (g.EVAL_CSRC, "eval_api.hip", g.EVAL_HIPCC_FLAGS), "lovasz": (g.LOVASZ_CSRC, "lovasz_api.hip", g.LOVASZ_HIPCC_FLAGS),
            "abn": (g.ABN_CSRC, "abn_api.hip", g.ABN_HIPCC_FLAGS), "proj": (g.PROJ_CSRC, "proj_api.hip", g.PROJ_HIPCC_FLAGS)}


LIBRARIES = ("cca", "ohem", "eval", "lovasz", "abn", "proj")
# the kernels that read LDS outside the compiler's bookkeeping: library -> name -> the template instantiations that must be there
HAND_WAITED = {"cca": ("proj_gemm_kernel", ("ILb0E", "ILb1E")), "proj": ("gemm_bf16_kernel", ("ILb0E", "ILb1E"))}


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """library -> {function name: lines}; each translation unit is compiled once (device only, the product's flags)"""
    done = {}

    def get(name):
        if name not in done:
            src_dir, unit, flags = _libraries()[name]
            flags = [f for f in flags if f not in ("-shared", "-fPIC") and not f.startswith("-Wl,")]
            out = str(tmp_path_factory.mktemp("isa_" + name) / (name + ".s"))
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(src_dir, unit), "-o", out], check=True, cwd=src_dir)
            with open(out) as f:
                done[name] = H.functions(f.read())
        return done[name]

    return get


@pytest.mark.parametrize("library", LIBRARIES)
def test_no_instruction_touches_an_outstanding_lds_destination(assembly, library):
    funcs = assembly(library)
    assert funcs, "no function found in the assembly"
    bad = {}
    for name, lines in funcs.items():
        report = H.analyse(name, lines)[0]
        if report:
            bad[name] = report
    lines = [f"{name}: {len(r)} violation(s), first:\n" + "\n".join(f"    [{v.block}] {v.text}    <- v{list(v.regs)} in flight" for v in r[:4])
             for name, r in sorted(bad.items())]
    assert not bad, f"{len(bad)} of {len(funcs)} kernels of '{library}' touch registers of LDS reads in flight:\n" + "\n".join(lines)


@pytest.mark.parametrize("library", sorted(HAND_WAITED))
def test_the_hand_waited_gemms_are_among_the_checked_kernels(assembly, library):
    """a renamed or re-templated kernel must not leave the check silently: both instantiations are found by name and hold the
    uncounted fragment reads (2 x 8 ds_read_b128 per k step at least)"""
    funcs = assembly(library)
    kernel, insts = HAND_WAITED[library]
    for inst in insts:
        names = [n for n in funcs if kernel + inst in n]
        assert len(names) == 1, (kernel, inst, names)
        assert H.count_mnemonic(funcs[names[0]], "ds_read_b128") >= 16, names[0]
