"""Option "stream_policy" in the instruction stream: a cache policy (ccnet_amd/csrc/cca_policy.hpp) puts a modifier on vector-memory
instructions and changes nothing else.

The attention library is compiled for gfx950 with the product's flags (the compile helper of tests/test_isa_hazards.py, by
import; the instruction reader of tests/isa_hazards.py).  For the two kernels of the split-plane step that ship a policy -- the
forward NCHW row pass (v, partial and x loads non-temporal) and the dv row pass (plane and partial loads, dv stores):

  * the DEFAULT instantiation (policy 0: what every launch outside the option runs, and every launch under mask 0) carries no
    cache modifier on any vector-memory instruction -- it is the instruction stream of before the option;
  * the SHIPPED instantiation has the same number of vector-memory instructions per opcode and the same sequence of
    ``s_waitcnt vmcnt(N)`` operands as the default one;
  * its modifiers sit only where its policy says: ``nt`` on 16-byte loads (LDS-DMA fills: all of them where the features are
    non-temporal, none otherwise; register loads: the addend / residual / source only, so where the attention block is read
    16 bytes wide some stay plain), ``nt`` or ``sc1`` on every 16-byte store and on nothing narrower.

No kernel has more than the two instantiations, and no other kernel of the library carries a modifier of the option."""
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import isa_hazards as H  # noqa: E402
from test_isa_hazards import assembly  # noqa: E402,F401  (the fixture: compiles a library's translation unit once)

FEAT_NT, ADD_NT, SRC_NT, ST_NT, ST_WT = 1, 2, 4, 8, 16            # cca::SP_* of cca_policy.hpp
# launch -> (mangled name with the policy left open, shipped policy)
KERNELS = {
    "L4 forward NCHW row pass": ("_ZN3cca11gmap_kernelILi100ELb1ELb0ELb1EffLb1ELb0ELi2ELb0ELb0ELb0ELb0ELi%dEEEv", FEAT_NT | ADD_NT | SRC_NT),
    "L8 dv row pass": ("_ZN3cca11gmap_kernelILi100ELb1ELb1ELb1ENS_7bf16p_tEfLb0ELb0ELi2ELb0ELb0ELb0ELb0ELi%dEEEv", FEAT_NT | ADD_NT | ST_NT),
}
_VMEM = ("buffer_", "global_", "flat_", "scratch_")
_MODIFIER = re.compile(r"(?<![\w.])(nt|sc0|sc1|glc|slc|dlc)(?![\w.])")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def vmem(lines):
    """[(mnemonic, is LDS-DMA, modifiers)] of a function's vector-memory instructions, in order"""
    out = []
    for _, mn, ops, _ in H._instructions(lines):
        if mn and mn.startswith(_VMEM):
            text = ops if isinstance(ops, str) else " ".join(ops)
            out.append((mn, re.search(r"(?<![\w.])lds(?![\w.])", text) is not None, tuple(sorted(set(_MODIFIER.findall(text))))))
    return out


def vmcnt_sequence(lines):
    seq = []
    for _, mn, ops, _ in H._instructions(lines):
        if mn == "s_waitcnt":
            m = _VMCNT.search(ops if isinstance(ops, str) else " ".join(ops))
            if m:
                seq.append(int(m.group(1)))
    return seq


def opcode_counts(insts):
    counts = {}
    for mn, lds, _ in insts:
        counts[(mn, lds)] = counts.get((mn, lds), 0) + 1
    return counts


def find(funcs, pattern):
    """{policy: function name} of the instantiations of one kernel"""
    rx = re.compile("^" + re.escape(pattern).replace("%d", r"(\d+)"))
    return {int(m.group(1)): n for n in funcs for m in [rx.match(n)] if m}


def check_pair(default, shipped, pol):
    """the three properties of the module docstring for one kernel; returns a list of complaints"""
    bad = []
    d, s = vmem(default), vmem(shipped)
    if any(mods for _, _, mods in d):
        bad.append("default instantiation carries modifiers: %r" % sorted({(mn, mods) for mn, _, mods in d if mods}))
    if opcode_counts(d) != opcode_counts(s):
        bad.append("vector-memory instructions per opcode differ: %r vs %r" % (opcode_counts(d), opcode_counts(s)))
    if vmcnt_sequence(default) != vmcnt_sequence(shipped):
        bad.append("s_waitcnt vmcnt sequences differ: %r vs %r" % (vmcnt_sequence(default), vmcnt_sequence(shipped)))
    store_mod = ("sc1",) if pol & ST_WT else ("nt",) if pol & ST_NT else ()
    for mn, lds, mods in s:
        if mn == "buffer_store_dwordx4":
            want = mods == store_mod
        elif mn == "buffer_load_dwordx4" and lds:
            want = mods == (("nt",) if pol & FEAT_NT else ())
        elif mn == "buffer_load_dwordx4":
            want = mods in ((), ("nt",)) if pol & (ADD_NT | SRC_NT) else mods == ()
        else:
            want = mods == ()
        if not want:
            bad.append("%s%s carries %r under policy %d" % (mn, " lds" if lds else "", mods, pol))
    if pol & (ADD_NT | SRC_NT) and not any(mn == "buffer_load_dwordx4" and not lds and mods == ("nt",) for mn, lds, mods in s):
        bad.append("no non-temporal register load under policy %d" % pol)
    return bad


@pytest.fixture(scope="module")
def funcs(assembly):
    return assembly("cca")


@pytest.mark.parametrize("launch", sorted(KERNELS))
def test_policy_puts_modifiers_on_and_changes_nothing_else(funcs, launch):
    pattern, pol = KERNELS[launch]
    found = find(funcs, pattern)
    assert sorted(found) == [0, pol], (launch, "instantiations by policy", sorted(found))
    default = funcs[found[0]]
    assert vmem(default), (launch, "no vector-memory instruction found")
    bad = check_pair(default, funcs[found[pol]], pol)
    assert not bad, (launch, bad)


def test_no_other_kernel_carries_a_modifier_of_the_option(funcs):
    """every other kernel of the library is untouched: `nt` appears in no function but the two shipped instantiations"""
    shipped = {find(funcs, p)[pol] for p, pol in KERNELS.values()}
    bad = sorted(n for n, lines in funcs.items() if n not in shipped and any("nt" in mods for _, _, mods in vmem(lines)))
    assert not bad, bad
