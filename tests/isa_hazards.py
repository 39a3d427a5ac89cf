"""A register-hazard walk over gfx950 assembly for LDS reads whose completion the kernel waits for by hand.

cca::lds_read_x4_uncounted (ccnet_amd/csrc/cca_platform.hpp) is an inline-asm ds_read_b128: hipcc keeps no lgkmcnt
bookkeeping for it, and neither the compiler nor the hardware keeps an instruction from touching the destination registers of
such a read before the hand-placed ``s_waitcnt lgkmcnt``.  The SIMT emulator completes the read at once, and on the device the
LDS usually answers in time -- so the only place where a missing wait shows reliably is the instruction stream.  This module
reads it.  A plain module, test infrastructure only; tests/test_isa_hazards.py holds its self-tests and runs it over every
library.

Per function (``.type NAME,@function`` ... ``.Lfunc_end``): basic blocks at ``.LBB`` labels and after branches, a forward
fixpoint over the ordered queue of outstanding lgkm operations (oldest first; an entry = the destination VGPRs + "scalar-memory
class"), joined at the NEWEST end position by position.  The walk is path-insensitive on purpose: it does not know that two
branch conditions agree, so source that is only correct because they do does not pass.

    ds_*                                appends an entry: the first operand of the returning forms, nothing for the others
    s_load* s_buffer_load* s_memtime    append a scalar-class entry (these return out of order: retired by lgkmcnt(0) only)
    s_memrealtime s_sendmsg* flat_*
    s_waitcnt .. lgkmcnt(N)             keeps the newest N LDS entries (LDS answers in order), N = 0 clears the queue; the
                                        raw-immediate form carries lgkmcnt in bits 11:8; without the field nothing changes
    anything else                       a VGPR operand (read or written) inside an outstanding destination is a violation;
                                        a returning ds_* is checked on its address / data operands only (another in-order
                                        LDS read may re-target an outstanding destination)
"""
import re
from collections import namedtuple

QUEUE_CAP = 64
Violation = namedtuple("Violation", "kernel block text regs")
Entry = namedtuple("Entry", "regs scalar")

SCALAR_PREFIXES = ("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_sendmsg", "flat_")
DS_RETURNING_PREFIXES = ("ds_read", "ds_load")
DS_RETURNING_OTHER = ("ds_bpermute_b32", "ds_permute_b32", "ds_swizzle_b32", "ds_consume", "ds_append", "ds_ordered_count")

_VREG = re.compile(r"(?<![\w.])v(\d+)\b|(?<![\w.])v\[(\d+):(\d+)\]")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_FUNC_TYPE = re.compile(r"^\s*\.type\s+([\w.$]+),@function")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def vregs(text):
    """the VGPR numbers named in an operand string: vN and v[a:b]"""
    out = set()
    for m in _VREG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return frozenset(out)


def _split_operands(ops):
    """top-level commas only (v[0:3] holds none, but stay safe)"""
    parts, depth, cur = [], 0, ""
    for ch in ops:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur.strip())
    return parts


def _ds_returns(mn):
    return mn.startswith(DS_RETURNING_PREFIXES) or "_rtn" in mn or mn in DS_RETURNING_OTHER


def waitcnt_lgkm(ops):
    """the lgkmcnt an s_waitcnt operand string asks for, or None when it has no such field"""
    m = _LGKM.search(ops)
    if m:
        return int(m.group(1))
    raw = ops.strip()
    if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", raw):
        return (int(raw, 0) >> 8) & 0xF
    return None


def step(queue, mn, ops):
    """one instruction: (the queue after it, the outstanding destination registers it touches)"""
    if mn == "s_waitcnt":
        n = waitcnt_lgkm(ops)
        if n is None:
            return queue, frozenset()
        if n == 0:
            return (), frozenset()
        kept, left = [], n
        for e in reversed(queue):
            if e.scalar:
                kept.append(e)
            elif left > 0:
                kept.append(e)
                left -= 1
        return tuple(reversed(kept)), frozenset()
    outstanding = frozenset().union(*(e.regs for e in queue)) if queue else frozenset()
    if mn.startswith("ds_"):
        parts = _split_operands(ops)
        ret = _ds_returns(mn)
        dest = vregs(parts[0]) if ret and parts else frozenset()
        touched = vregs(", ".join(parts[1:] if ret else parts)) & outstanding
        return _push(queue, Entry(dest, False)), touched
    touched = vregs(ops) & outstanding
    if mn.startswith(SCALAR_PREFIXES):
        return _push(queue, Entry(frozenset(), True)), touched
    return queue, touched


def _push(queue, entry):
    queue = queue + (entry,)
    while len(queue) > QUEUE_CAP:                # the two oldest become one: never retired earlier than either would be
        a, b = queue[0], queue[1]
        queue = (Entry(a.regs | b.regs, a.scalar or b.scalar),) + queue[2:]
    return queue


def join(a, b):
    """queues aligned at the newest end, entries united position by position"""
    if a is None:
        return b
    if b is None:
        return a
    if len(a) < len(b):
        a, b = b, a
    head = len(a) - len(b)
    return a[:head] + tuple(Entry(x.regs | y.regs, x.scalar or y.scalar) for x, y in zip(a[head:], b))


Block = namedtuple("Block", "name insts succ")


def _instructions(lines):
    """[(label or None, mnemonic, operands, text)] of a function body: comments, directives and blank lines dropped"""
    out = []
    for line in lines:
        line = line.split(";", 1)[0].split("//", 1)[0].rstrip()
        if not line.strip():
            continue
        m = _LABEL.match(line.strip())
        if m:
            out.append((m.group(1), None, None, None))
            continue
        s = line.strip()
        if s.startswith("."):
            continue
        mn, _, ops = s.partition(" ")
        out.append((None, mn.strip(), ops.strip(), s))
    return out


def basic_blocks(name, lines):
    """the blocks of one function in layout order: a new one at every .LBB label and after every branch / s_endpgm; every
    branch target must be a block of the function"""
    blocks, n = [Block("entry", [], [])], 0
    for label, mn, ops, text in _instructions(lines):
        if label is not None:
            if label.startswith(".LBB"):
                blocks.append(Block(label, [], []))
            continue
        last = blocks[-1]
        if last.insts and _ends_flow(last.insts[-1][0]):         # an instruction straight after a branch: an unnamed block
            n += 1
            blocks.append(Block(f"{last.name}+{n}", [], []))
        blocks[-1].insts.append((mn, ops, text))
    names = {b.name for b in blocks}
    for i, b in enumerate(blocks):
        mn, ops = (b.insts[-1][0], b.insts[-1][1]) if b.insts else ("", "")
        if mn == "s_branch" or mn.startswith("s_cbranch"):
            b.succ.append(ops.split(",")[-1].strip())
        if (mn.startswith("s_cbranch") or not _ends_flow(mn)) and i + 1 < len(blocks):
            b.succ.append(blocks[i + 1].name)
        for t in b.succ:
            assert t in names, (name, b.name, "branch target is no block of this function", t)
    return blocks


def _ends_flow(mn):
    return mn in ("s_branch", "s_endpgm", "s_setpc_b64") or mn.startswith("s_cbranch")


def _run_block(block, queue, report=None, kernel=None):
    for mn, ops, text in block.insts:
        queue, touched = step(queue, mn, ops)
        if touched and report is not None:
            report.append(Violation(kernel, block.name, text, tuple(sorted(touched))))
    return queue


def analyse(name, lines):
    """(violations, {block name: queue on entry}, queue at the end of the last block) of one function"""
    blocks = basic_blocks(name, lines)
    by_name = {b.name: b for b in blocks}
    state = {b.name: None for b in blocks}
    state[blocks[0].name] = ()
    work = [blocks[0].name]
    while work:
        b = by_name[work.pop()]
        out = _run_block(b, state[b.name])
        for t in b.succ:
            merged = join(state[t], out)
            if merged != state[t]:
                state[t] = merged
                if t not in work:
                    work.append(t)
    report, last = [], ()
    for b in blocks:
        if state[b.name] is not None:
            last = _run_block(b, state[b.name], report, name)
    return report, state, last


def functions(asm_text):
    """{function name: its lines} of an assembly file"""
    lines = asm_text.splitlines()
    names = {m.group(1) for m in map(_FUNC_TYPE.match, lines) if m}
    out, cur = {}, None
    for line in lines:
        m = _LABEL.match(line)
        if m and m.group(1) in names and cur is None:
            cur = m.group(1)
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            out[cur].append(line)
    return out


def check_snippet(text, name="snippet"):
    """the self-tests' entry: a function body given as a string -> (violations, final queue)"""
    report, _, last = analyse(name, text.splitlines())
    return report, last


def check_assembly(asm_text):
    """{function name: [Violation]} for every function of an assembly file (an empty list = clean)"""
    return {name: analyse(name, lines)[0] for name, lines in functions(asm_text).items()}


def count_mnemonic(lines, mnemonic):
    return sum(1 for _, mn, _, _ in _instructions(lines) if mn == mnemonic)
