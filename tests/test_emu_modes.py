"""The emulator's case tables under the emulator's other modes (tests/emu/hip_emu.hpp).

LATE      every LDS-DMA lands at the latest moment the kernel's own waits allow: a counted barrier whose count is one too high,
          or a barrier_lds_only() where a counted one belongs, reads a stage whose fill has not landed.
REVERSED  wavefronts, and lanes within them, run in descending order: the half of the missing-barrier races that the ascending
          order hides.
Every run is held BIT FOR BIT to a default-mode run computed first, with every variable unset: for tests/cca_cases.py the
case on dense, unguarded buffers (what run_case compares with), for everything else the same call.  The variables are set with
``monkeypatch`` around the calls under test only.

No float result of these tables depends on the order of arrival -- the kernels reduce in a fixed order (per-workgroup partial
sums combined by index) and their atomics are integer ones -- so one bar, equality, serves every case, the reversed schedule
included.  A kernel that legitimately sums floats in arrival order would have to be named here and held to its existing bar.

``test_every_counted_barrier_line_is_reached`` is a condition on the tables, ``test_a_keep_one_too_high_is_seen_in_every_family``
is the proof that the late mode has teeth on the real kernels."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
import emu_modes as M  # noqa: E402
import proj_cases as P  # noqa: E402
from emu_util import EmuOps  # noqa: E402
from guarded_memory import HostMemory  # noqa: E402

ROOT = os.path.dirname(HERE)
MFMA = 2


@pytest.fixture(scope="module")
def ops():
    o = EmuOps()
    yield o
    o.set_impl(0)
    o.lib.ccnet_cca_set_precision(2)


@pytest.fixture(scope="module")
def lib(ops):
    return ops.lib


@pytest.fixture(scope="module")
def proj():
    import test_emu_proj
    from ccnet_amd._proj_lib import ProjLibrary
    return ProjLibrary(test_emu_proj.build_emu())


@pytest.fixture(scope="module")
def mem():
    return HostMemory()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the three sets of the attention core and the projection library
# ---------------------------------------------------------------------------------------------------------------------
# tests/cca_cases.py in the two forms with padding between rows and images (the dense and packed repeats add no kernel path)
CCA_IDS = [(cid, form) for cid, form in K.ids(emulator=True) if form in ("padded", "tight")]


def cca_case(lib, mem, monkeypatch, mode, cid, form):
    M.set_mode(monkeypatch)
    K.plain_case(lib, mem, cid)                      # the default mode's result, if no test has computed it yet
    M.set_mode(monkeypatch, *mode)
    K.run_case_bits(lib, mem, cid, form)


@pytest.mark.parametrize("cid,form", CCA_IDS, ids=lambda v: v)
def test_cca_table_with_late_dma(lib, mem, monkeypatch, cid, form):
    cca_case(lib, mem, monkeypatch, (M.LATE,), cid, form)


@pytest.mark.parametrize("cid,form", CCA_IDS, ids=lambda v: v)
def test_cca_table_in_reversed_order(lib, mem, monkeypatch, cid, form):
    cca_case(lib, mem, monkeypatch, (M.REVERSE,), cid, form)


_GEMM = {}            # (case, variant) -> the default mode's bits


def gemm_case(proj, mem, monkeypatch, mode, cid, variant):
    M.set_mode(monkeypatch)
    if (cid, variant) not in _GEMM:
        _GEMM[cid, variant] = P.gemm_bits(proj, mem, cid, variant)
    M.set_mode(monkeypatch, *mode)
    return same_bits(P.gemm_bits(proj, mem, cid, variant), _GEMM[cid, variant])


@pytest.mark.parametrize("cid,variant", P.gemm_ids(), ids=lambda v: v)
def test_proj_gemm_table_with_late_dma(proj, mem, monkeypatch, cid, variant):
    assert gemm_case(proj, mem, monkeypatch, (M.LATE,), cid, variant)


@pytest.mark.parametrize("cid,variant", P.gemm_ids(), ids=lambda v: v)
def test_proj_gemm_table_in_reversed_order(proj, mem, monkeypatch, cid, variant):
    assert gemm_case(proj, mem, monkeypatch, (M.REVERSE,), cid, variant)


# The fp32 strip family (cca_map.hpp, cca_weight.hpp, cca_long.hpp) is not in tests/cca_cases.py.  The smallest shapes of
# tests/test_emu_kernels.py that reach each of its counted barriers with a nonzero keep and with a tail:
STRIP_SHAPES = [
    (1, 16, 9, 99),      # odd H and W; row strips 99 long: the EXACT bodies (97..100), cca_map.hpp's <QF> and <NSTORE_MIN> sites, in
                         # one full group of 8 strips (the counted form) and a last group of one strip
    (1, 16, 65, 12),     # column strips 65 long: the FULL bodies below 97 with out-of-range pieces, the barrier_dma_keep_n(nstore) site
    (1, 24, 99, 9),      # C = 24 is no multiple of the channel group: cca_map.hpp falls back to __syncthreads(), cca_weight.hpp's <QT> counts
    (1, 16, 129, 12),    # a long-row geometry beyond 128: cca_long.hpp (fills in flight across barrier_lds_only(), no counted barrier)
]
_STRIP = {}


def strip_family(ops, shape, given=None):
    """every entry point of the fp32 NCHW family on one shape, exact-fp32 arithmetic, the MFMA kernels.  ``given``: the default
    mode's results -- the un-fused entry points then take ITS attention and dA as their inputs, so that each output shows
    its own kernel's behaviour under the mode and not a wrong input from the kernel before it"""
    rng = np.random.default_rng(sum(shape))
    B, C, H, W = shape
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)                     # noqa: E731
    q, k, v, x, dy = f(B, max(C // 8, 1), H, W), f(B, max(C // 8, 1), H, W), f(B, C, H, W), f(B, C, H, W), f(B, C, H, W)
    gamma = np.array([0.5], np.float32)
    ops.lib.ccnet_cca_set_precision(0)
    ops.set_impl(MFMA)
    try:
        y, A = ops.cca_forward(q, k, v, x, gamma)
        dq, dk, dv, dg = ops.cca_backward(dy, q, k, v, A, gamma)
        A_in = given["A"] if given else A
        o = ops.ca_map_forward(A_in, v)
        dA, dv1 = ops.ca_map_backward(dy, A_in, v, gamma)
        dq1, dk1 = ops.ca_backward(given["dA"] if given else dA, q, k)
    finally:
        ops.set_impl(0)
        ops.lib.ccnet_cca_set_precision(2)
    return dict(y=y, A=A, dq=dq, dk=dk, dv=dv, dgamma=dg, map=o, dA=dA, dv1=dv1, dq1=dq1, dk1=dk1)


def strip_case(ops, monkeypatch, mode, shape):
    M.set_mode(monkeypatch)
    if shape not in _STRIP:
        _STRIP[shape] = strip_family(ops, shape)
    M.set_mode(monkeypatch, *mode)
    got = strip_family(ops, shape, _STRIP[shape])
    return [name for name, ref in _STRIP[shape].items() if not same_bits(got[name], ref)]


@pytest.mark.parametrize("shape", STRIP_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_fp32_strip_family_with_late_dma(ops, monkeypatch, shape):
    assert strip_case(ops, monkeypatch, (M.LATE,), shape) == []


@pytest.mark.parametrize("shape", STRIP_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_fp32_strip_family_in_reversed_order(ops, monkeypatch, shape):
    assert strip_case(ops, monkeypatch, (M.REVERSE,), shape) == []


# Cases the counted barriers need beyond tests/cca_cases.py (the coverage condition below).  The emulator's default device has
# 256 CUs, for which the host cuts a small problem's strips into one channel group per workgroup: the barriers between channel
# groups never run.  On a device with two CUs (tests/emu/cca_platform.hpp) the same small shapes run whole rounds of strips.
#   id -> (table entry, CUs)
EXTRA = {
    # three channel groups per workgroup: cca_gmap.hpp's keep_n between groups with the next fill in flight (gmap_kernel and gmap3)
    "pm_bf16-1x192x5x6-2cu": ((K.run_pm, K.check_pm, ("bf16", (1, 192, 5, 6), 24), {"bf16_partial": 1}, False), 2),
    "pm_f32-1x192x5x6-2cu": ((K.run_pm, K.check_pm, ("f32", (1, 192, 5, 6), 24), {}, False), 2),
    # ... with a partial last group (136 = 2 x 64 + 8), the D = 1 form and the streaming dA kernel's keep_n with a nonzero keep
    "planes_bias-1x136x5x6-2cu": ((K.run_planes, K.check_planes, ((1, 136, 5, 6), 8, "bias"), {}, False), 2),
    # ... at full strip length, where one instruction more in flight is seen (the teeth check)
    "pm_bf16-1x192x2x97-2cu": ((K.run_pm, K.check_pm, ("bf16", (1, 192, 2, 97), 24), {"bf16_partial": 1}, False), 2),
    # the three-stage gweight_kernel of the split-plane dA ("planes_stream" 0) with more than one chunk: its keep_n(npw)
    "planes_nobias-1x136x2x97-gweight": ((K.run_planes, K.check_planes, ((1, 136, 2, 97), 8, "nobias"), {"planes_stream": 0}, False), 0),
}


def extra_case(lib, mem, monkeypatch, mode, cid, form="tight"):
    case, cus = EXTRA[cid]
    lib.dll.cca_emu_set_device(1 if cus else 0, cus)
    try:
        M.set_mode(monkeypatch)
        K.plain_case(lib, mem, cid, case)
        M.set_mode(monkeypatch, *mode)
        K.run_case_bits(lib, mem, cid, form, case)
    finally:
        lib.dll.cca_emu_set_device(0, 0)


@pytest.mark.parametrize("cid", sorted(EXTRA))
@pytest.mark.parametrize("mode", ["late", "reversed"])
def test_multi_stage_cases_in_both_modes(lib, mem, monkeypatch, cid, mode):
    extra_case(lib, mem, monkeypatch, (M.LATE,) if mode == "late" else (M.REVERSE,), cid)


# ---------------------------------------------------------------------------------------------------------------------
# the coverage condition and the teeth
# ---------------------------------------------------------------------------------------------------------------------
# lines that call a counted barrier but are not a wait of a kernel: "file:line" -> reason
EXEMPT = {
    "cca_common.hpp:249": "the body of barrier_dma_keep_n: the barrier is charged to the line of the CALL of barrier_dma_keep_n",
    "cca_common.hpp:254": "the body of barrier_dma_keep_n (its default: branch), as above",
}


def counted_barrier_lines():
    """{"file:line": needs a keep above 0} for every source line under ccnet_amd/csrc*/ that calls barrier_dma_keep<K>() or
    barrier_dma_keep_n(): every _n line and every template keep other than the literal 0 must be seen with a keep above 0"""
    out = {}
    base = os.path.join(ROOT, "ccnet_amd")
    for d in sorted(os.listdir(base)):
        if not d.startswith("csrc"):
            continue
        for f in sorted(os.listdir(os.path.join(base, d))):
            if not f.endswith((".hpp", ".hip")) or f == "cca_probe.hpp":           # (the probe kernels are exempt)
                continue
            for i, text in enumerate(open(os.path.join(base, d, f)).read().splitlines()):
                code = text.split("//")[0]
                if "__device__" in code:                                          # the definitions
                    continue
                for m in re.finditer(r"\bbarrier_dma_keep(_n\s*\(|\s*<([^>]*)>\s*\()", code):
                    key = f"{f}:{i + 1}"
                    out[key] = out.get(key, False) or m.group(2) is None or m.group(2).strip() != "0"
    return out


def test_the_source_scan_finds_the_counted_barriers():
    lines = counted_barrier_lines()
    files = {k.split(":")[0] for k in lines}
    assert {"cca_gemm.hpp", "cca_gmap.hpp", "cca_map.hpp", "cca_weight.hpp", "proj_kernels.hpp", "cca_common.hpp"} <= files
    assert "cca_probe.hpp" not in files and "cca_platform.hpp" not in files and len(lines) >= 30
    assert set(EXEMPT) <= set(lines)
    assert "cca_long.hpp" not in files              # the long-strip family has no counted barrier (see the teeth check)


def _unreached(lines, *stats):
    sites = {}
    for st in stats:
        for key, (runs, unlanded, keep, keep_unlanded) in st["sites"].items():
            old = sites.get(key, (0, -1))
            sites[key] = (old[0] + unlanded, max(old[1], keep_unlanded))
    missing = {}
    for key, needs_keep in lines.items():
        if key in EXEMPT:
            continue
        unlanded, keep = sites.get(key, (0, -1))
        if not unlanded:
            missing[key] = "never reached with an un-landed DMA in the queue"
        elif needs_keep and keep <= 0:
            missing[key] = "never reached with a keep above 0 and an un-landed DMA in the queue"
    return missing


def test_every_counted_barrier_line_is_reached(ops, lib, proj, mem, monkeypatch):
    """A condition on the tables above: every line of the sources that calls a counted barrier has run in late mode with an
    un-landed LDS-DMA in the wave's queue -- where its count can be wrong, it was tested.  The counters accumulate in the two
    emulator libraries over this module's late-mode tests; run on its own, the test runs those cases itself first."""
    lines = counted_barrier_lines()
    stats = lambda: (M.vmem_stats(lib.dll), M.vmem_stats(proj.dll))              # noqa: E731
    if _unreached(lines, *stats()):
        for cid, form in CCA_IDS:
            if form == "tight":
                cca_case(lib, mem, monkeypatch, (M.LATE,), cid, form)
        for cid in sorted(EXTRA):
            extra_case(lib, mem, monkeypatch, (M.LATE,), cid)
        for cid, variant in P.gemm_ids():
            if variant == "plain-dense":
                gemm_case(proj, mem, monkeypatch, (M.LATE,), cid, variant)
        for shape in STRIP_SHAPES:
            strip_case(ops, monkeypatch, (M.LATE,), shape)
    M.set_mode(monkeypatch)
    missing = _unreached(lines, *stats())
    assert not missing, missing
    for st in stats():
        assert st["dma_issued"] > 0 and 0 < st["retired_by_counted_barriers"] <= st["dma_issued"]


def _differs(call):
    """what the case's own bit checks say: Arena.settle's (the poison a kernel read from an un-landed stage is a NaN in a written
    view) or the comparison with the default mode's result; "" where the run passes both"""
    try:
        call()
    except AssertionError as e:
        assert "differs from the dense, unguarded call" in str(e) or "in-view elements left unwritten or NaN" in str(e), e
        return str(e)
    return ""


# kernel family -> a late-mode case that must fail its bit comparison when every counted barrier keeps one instruction more
TEETH_CCA = {
    "projection GEMM (cca_gemm.hpp)": ("projection-300x136x192", ("'out'",)),
    "projection adjoint (cca_gemm.hpp)": ("adjoint-1x72x257x64", ("'dx'",)),
    "wgrad (cca_gemm.hpp)": ("wgrad-130x136x264x3", ("'part'",)),
    # the forward's outputs: the energies (gweight_kernel) and the aggregation (gmap_kernel)
    "gmap forward (cca_gmap.hpp)": ("pm_bf16-1x64x3x97-partial1", ("'A'", "'y'")),
    "gmap forward, fp32 (cca_gmap.hpp)": ("pm_f32-1x64x100x3", ("'A'", "'y'")),
}


@pytest.mark.parametrize("family", sorted(TEETH_CCA))
def test_a_keep_one_too_high_is_seen_in_every_family(lib, mem, monkeypatch, family):
    cid, names = TEETH_CCA[family]
    M.set_mode(monkeypatch)
    K.plain_case(lib, mem, cid)
    M.set_mode(monkeypatch, M.LATE, M.KEEP_PLUS)
    why = _differs(lambda: K.run_case_bits(lib, mem, cid, "tight"))
    assert why and any(n in why for n in names), (family, cid, why)


def test_a_keep_one_too_high_is_seen_in_the_gmap_strip_and_dA_kernels(lib, mem, monkeypatch):
    """the backward of the pixel-major family (the dv strip passes of gmap_kernel, the dA contraction) on the attention of a
    DEFAULT-mode forward: run_pm's backward reads the A its own forward wrote, so the forward runs without the extra keep"""
    import cca_cases
    cid = "pm_bf16-1x64x3x97-partial1"
    run, check, args, options, _ = K.CASES[cid]
    M.set_mode(monkeypatch)
    plain = K.plain_case(lib, mem, cid)

    def in_default_mode(entry):
        def call(*a):
            M.set_mode(monkeypatch)
            try:
                return entry(*a)
            finally:
                M.set_mode(monkeypatch, M.LATE, M.KEEP_PLUS)
        return call

    M.set_mode(monkeypatch, M.LATE, M.KEEP_PLUS)
    for name in ("ccnet_cca_forward_pm_bf16", "ccnet_cca_attention_pm"):          # (the forward and the attention recompute)
        monkeypatch.setattr(lib, name, in_default_mode(getattr(lib, name)), raising=False)
    got = {}

    def call():
        with cca_cases._options(lib, options):
            got.update(run(lib, mem, "tight", True, False, *args))

    why = _differs(call)
    if why:                                         # the forward and the attention recompute passed their checks; the backward did not
        assert why.startswith("('backward_pm'"), why
    else:
        assert np.array_equal(got["y"], plain["y"]) and np.array_equal(got["A"], plain["A"])
        assert [n for n in ("dq", "dk", "dv") if not np.array_equal(got[n], plain[n])], "no gradient changed"


def test_a_keep_one_too_high_is_seen_in_the_proj_library(proj, mem, monkeypatch):
    same = []
    why = _differs(lambda: same.append(gemm_case(proj, mem, monkeypatch, (M.LATE, M.KEEP_PLUS), "300x640x192", "plain-dense")))
    assert why or same == [False]


def test_a_keep_one_too_high_is_seen_in_the_fp32_strip_kernels(ops, monkeypatch):
    """map: ca_map_forward (cca_map.hpp); weight: the dA of ca_map_backward (cca_weight.hpp), both on the default mode's attention.
    long: cca_long.hpp has no counted barrier (test_the_source_scan_finds_the_counted_barriers) -- its fills are waited for by
    __syncthreads() -- so one more kept instruction changes nothing there, which is asserted too."""
    changed = strip_case(ops, monkeypatch, (M.LATE, M.KEEP_PLUS), (1, 16, 9, 99))
    assert "map" in changed and "dA" in changed, changed
    assert strip_case(ops, monkeypatch, (M.LATE, M.KEEP_PLUS), (1, 16, 129, 12)) == []


# ---------------------------------------------------------------------------------------------------------------------
# the reversed schedule on the other four libraries' emulator tables (they share tests/emu/hip_emu.cpp's scheduler)
# ---------------------------------------------------------------------------------------------------------------------
def default_then_reversed(monkeypatch, call):
    M.set_mode(monkeypatch)
    want = call()
    M.set_mode(monkeypatch, M.REVERSE)
    got = call()
    M.set_mode(monkeypatch)
    return want, got


def assert_same_results(want, got):
    if isinstance(want, dict):
        want, got = [want[k] for k in sorted(want)], [got[k] for k in sorted(want)]
    for i, (a, b) in enumerate(zip(want, got)):
        if isinstance(a, np.ndarray):
            assert same_bits(a, b), i
        else:                                        # scalars the drivers unpack: floats (NaN compares by bits), counts, None
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=isinstance(a, float)), (i, a, b)


import test_abn_host as ABN  # noqa: E402
import test_eval_host as EVAL  # noqa: E402
import test_lovasz_host as LOVASZ  # noqa: E402
import test_ohem_host as OHEM  # noqa: E402

abn_emu, ohem_emu, lovasz_emu, eval_emu = ABN.emu, OHEM.emu, LOVASZ.emu, EVAL.emu      # the modules' own library fixtures


@pytest.mark.parametrize("name", sorted(ABN.EMU_CASES))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_abn_table_in_reversed_order(abn_emu, monkeypatch, name, bf16):
    """statistics are per-workgroup partial sums combined by index, dweight / dbias likewise: no arrival order in any result"""
    shape, act, p, gm, source, residual, training = ABN.EMU_CASES[name]
    x, w, b, rm, rv, dy, res = ABN._case(shape, seed=len(name), residual=residual)
    want, got = default_then_reversed(monkeypatch, lambda: ABN.emu_abn(
        abn_emu, x, w, b, rm, rv, dy, training=training, act=act, p=p, gamma_mode=gm, residual=res, source=source, bf16=bf16))
    assert_same_results(want, got)


@pytest.mark.parametrize("case", OHEM.O.EDGE_CASES)
def test_ohem_table_in_reversed_order(ohem_emu, monkeypatch, case):
    """the histogram and the kept count are integer atomics; the loss is a fixed-order sum of per-workgroup partials"""
    logits, target, case = OHEM.O.edge_case_inputs(case)
    want, got = default_then_reversed(monkeypatch, lambda: OHEM.emu_ohem(ohem_emu, logits, target, **case))
    assert_same_results(want, got)


@pytest.mark.parametrize("name", sorted(LOVASZ.EMU_CASES))
def test_lovasz_table_in_reversed_order(lovasz_emu, monkeypatch, name):
    """a stable radix sort (integer counts) and fixed-order scans: ties keep pixel order whatever runs first"""
    shape, args = LOVASZ.EMU_CASES[name]
    shape = dict(shape)
    B, C, H, W = (shape.pop(k) for k in ("B", "C", "H", "W"))
    probas, labels = LOVASZ.O.make_case_inputs(B, C, H, W, seed=B * 1000 + H * W + C, **shape)
    probas[..., ::3] = np.round(probas[..., ::3] * 64) / 64
    want, got = default_then_reversed(monkeypatch, lambda: LOVASZ.emu_lovasz(lovasz_emu, probas, labels, **args))
    assert_same_results(want, got)


@pytest.mark.parametrize("case", [dict(N=2, H=70, W=90, tile=33, C=19, flip=False), dict(N=1, H=70, W=90, tile=33, C=19, flip=True),
                                  dict(N=2, H=20, W=25, tile=33, C=7, flip=True)], ids=lambda c: "x".join(str(v) for v in c.values()))
def test_eval_table_in_reversed_order(eval_emu, monkeypatch, case):
    """(the cases of test_eval_host.test_emulated_kernel_matches_oracle) scores summed tile by tile in origin order; the confusion
    matrix is integer atomics"""
    from ccnet_amd.evaluate import tile_grid
    N, H, W, tile, C, flip = (case[k] for k in ("N", "H", "W", "tile", "C", "flip"))
    origins = tile_grid(H, W, (tile, tile))
    rng = np.random.default_rng(H * W + N)
    h = (tile + 7) // 8
    tiles = (rng.standard_normal((N, len(origins) * (2 if flip else 1), C, h, h)) * 3).astype(np.float32)
    _, label = EVAL.O.make_case_inputs(N, H, W, C, seed=7)
    want, got = default_then_reversed(monkeypatch, lambda: EVAL.emu_eval(eval_emu, tiles, origins, (tile, tile), H, W, flip, label))
    assert_same_results(want, got)
