"""What the mixed-precision optimiser tests share: the arithmetic of include/ccnet_sgdmp.h restated in NumPy (float32 with one
rounding per operation, the rounding to bf16 in uint32 integers), the case table, the seeded input builder and the
guarded-buffer driver of the C ABI.

A case is a dict: sizes, master (per tensor: a bf16 row with a float32 master, or a float32 row), offsets (per tensor, the
(p, g, b, m) offsets from a 16-byte boundary in elements of each buffer's own type: one bf16 element is 2 bytes, one float32
element 4), groups ((lr, mu, wd) each) and group (per tensor), null (tensors without a gradient), zero (zero_grads), cap,
schedule / counter, and the inputs p, g, b, m (p and g of a master row are uint16 bf16 bit patterns, m is None in a float32
row).  A master row's p starts as bf16 NaNs: the kernel must never read it.  Everything here is test infrastructure.
"""
import numpy as np

import sgd_oracle as S
from ccnet_amd._sgdmp_lib import CHUNK as C
from ccnet_amd._sgdmp_lib import TENSOR_WORDS
from guarded_memory import Buf

DEFAULT = S.DEFAULT                           # (lr, mu, wd) of a group
SCHEDULE = S.SCHEDULE
ALIGNED = (0, 0, 0, 0)
NAN16 = 0x7FC1                                # what a master row's p holds before the step


def bf16_rne(u):
    """uint32 float32 bit patterns -> uint16 bf16 bit patterns: to nearest, ties to even; a NaN gives (u >> 16) | 0x40"""
    u = np.asarray(u, np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rounded = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32)).astype(np.uint16)


def bf16_of(x):
    """float32 values -> bf16 bit patterns"""
    return bf16_rne(np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)).reshape(np.shape(x))


def float_of(h):
    """bf16 bit patterns -> the float32 values they stand for (exact)"""
    return (np.asarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def is_nan16(h):
    return (np.asarray(h, np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def master_step(g16, m, b, lr, mu, wd):
    """(m', b', p') of one step of a master row: the float32 step on float(g) against the master, then p' = bf16(m')"""
    nm, nb = S.sgd_step(m, float_of(g16), b, lr, mu, wd)
    return nm, nb, bf16_of(nm)


# masters that the rounding case holds (g = 0, wd = mu = 0 and b = 0 leave m' = m, so p' = bf16_rne(m); the two infinities
# aside, where 0 * inf makes a NaN: the nonfinite case reaches them through an infinite gradient) and, for the hand check of
# tests/test_sgdmp_host.py, what they round to
ROUNDING = [
    (0x3F808000, 0x3F80),   # half-way, even lower neighbour: down
    (0x3F818000, 0x3F82),   # half-way, odd lower neighbour: up
    (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80), (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),
    (0x3F7FFFFF, 0x3F80),   # -> 1.0
    (0x3F7F8000, 0x3F80),   # half-way below 1.0, odd lower neighbour: up across the exponent
    (0x7F7FFFFF, 0x7F80),   # past the largest bf16: inf
    (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F), (0xFF7FFFFF, 0xFF80),
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    (0x00000000, 0x0000), (0x80000000, 0x8000),                       # the sign of zero is kept
    (0x00000001, 0x0000), (0x80000001, 0x8000),                       # subnormals
    (0x00008000, 0x0000), (0x00018000, 0x0002), (0x00008001, 0x0001), (0x00400000, 0x0040), (0x807FFFFF, 0x8080),
    (0x007F8000, 0x0080), (0x00010000, 0x0001), (0x3F800000, 0x3F80), (0x40490FDB, 0x4049), (0xC2F6E979, 0xC2F7),
]

CASES = {
    "one_to_17": {"sizes": list(range(1, 18))},
    "round_edges": {"sizes": [2047, 2048, 2049]},
    "chunk_edges": {"sizes": [C - 1, C, C + 1, 2 * C + 3]},
    # p or g 2 and 8 bytes off, m or b 4 bytes off: each alone sends the row down the element path
    "misaligned": {"sizes": [37] * 7, "offsets": [(1, 0, 0, 0), (0, 1, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 1, 0),
                                                  (0, 0, 0, 1), ALIGNED]},
    "misaligned_long": {"sizes": [C + 9, 2049], "offsets": [(1, 0, 0, 0), (0, 0, 0, 1)]},
    "interleaved": {"sizes": [5, 5, C + 1, C + 1, 37, 37, 300, 2049, 9],
                    "master": [False, True, False, True, False, True, True, False, True],
                    "offsets": [ALIGNED, ALIGNED, ALIGNED, ALIGNED, (1, 0, 0, 0), (0, 1, 0, 0), ALIGNED, ALIGNED, ALIGNED]},
    "many_tiny": {"sizes": [1 + k % 3 for k in range(300)], "master": [k % 5 != 4 for k in range(300)]},
    "grid_stride_3": {"sizes": [3 * C + 5, 1, 2 * C], "cap": 3},
    "grid_stride_1": {"sizes": [3 * C + 5, 1, 2 * C], "cap": 1, "master": [True, False, True]},
    "null_grad": {"sizes": [9, 130, 4, 1024, 6], "null": (1, 4), "master": [True, True, False, True, False]},
    "zero_on": {"sizes": [5, C + 2, 64], "zero": True, "offsets": [ALIGNED, ALIGNED, (1, 1, 1, 1)]},
    "zero_off": {"sizes": [5, C + 2, 64], "zero": False, "offsets": [ALIGNED, ALIGNED, (1, 1, 1, 1)]},
    "groups": {"sizes": [33, 1030, 7, 260, 12, 5], "groups": [DEFAULT, (0.1, 0.0, 0.0), (0.0, 0.5, 1e-2)],
               "group": [0, 1, 2, 2, 1, 0], "master": [True, True, True, False, False, True]},
    # inf and NaN in g, m and b, in the vector part, the tail and an element-path row
    "nonfinite": {"sizes": [43, 19, 21], "offsets": [ALIGNED, ALIGNED, (1, 0, 0, 0)],
                  "poke": [("g", 0, 5, np.inf), ("g", 0, 22, np.nan), ("g", 0, 41, -np.inf), ("m", 0, 7, np.inf),
                           ("m", 0, 42, np.nan), ("b", 0, 9, -np.inf), ("b", 0, 30, np.nan), ("g", 1, 18, np.nan),
                           ("m", 1, 3, -np.inf), ("b", 1, 17, np.nan), ("g", 2, 4, np.nan), ("m", 2, 20, np.nan),
                           ("b", 2, 0, np.inf), ("g", 2, 9, np.inf), ("m", 2, 9, np.inf)]},
    # masters from bit patterns: the list twice over and rotated, so that every entry passes through the 16-byte path and the
    # tail, and once more in a row on the element path
    "rounding": {"sizes": [len(ROUNDING) + 4, len(ROUNDING) + 3, len(ROUNDING)], "groups": [(1.0, 0.0, 0.0)],
                 "offsets": [ALIGNED, ALIGNED, (0, 1, 0, 0)], "rounding": True},
}
for _s in (0, 3, 9):                           # 9: past the table, clamped to its last entry
    CASES[f"schedule_{_s}"] = {"sizes": [70, 2 * C + 1, 3], "schedule": SCHEDULE, "counter": _s,
                               "groups": [(1.0, 0.9, 5e-4)]}
    CASES[f"mult_{_s}"] = {"sizes": [70, 2 * C + 1, 3, 18], "schedule": SCHEDULE, "counter": _s, "master": [True, True, True, False],
                           "groups": [(1.0, 0.9, 5e-4), (10.0, 0.9, 5e-4)], "group": [0, 1, 0, 1]}


def rounding_masters(n, shift):
    """n float32 masters out of ROUNDING's bit patterns, starting `shift` entries in"""
    bits = np.array([u for u, _ in ROUNDING], np.uint32)
    return np.roll(bits, -shift)[np.arange(n) % len(bits)].view(np.float32).copy()


def build_case(name):
    """The case with every default filled in and its seeded inputs"""
    raw = CASES[name]
    sizes = list(raw["sizes"])
    n = len(sizes)
    case = {"name": name, "sizes": sizes, "master": list(raw.get("master", [True] * n)),
            "offsets": list(raw.get("offsets", [ALIGNED] * n)),
            "groups": list(raw.get("groups", [DEFAULT])), "group": list(raw.get("group", [0] * n)),
            "null": tuple(raw.get("null", ())), "zero": bool(raw.get("zero", True)),
            "cap": raw.get("cap", 0), "schedule": raw.get("schedule"), "counter": raw.get("counter", 0)}
    seed = (100 + list(CASES).index(name)) * 4096
    case["p"], case["g"], case["b"], case["m"] = [], [], [], []
    for t, s in enumerate(sizes):
        values, g, b = (S.make_data(s, seed + 3 * t + j) for j in range(3))
        if raw.get("rounding"):
            values, g, b = rounding_masters(s, 5 * t), np.zeros(s, np.float32), np.zeros(s, np.float32)
        if case["master"][t]:
            case["p"].append(np.full(s, NAN16, np.uint16)), case["m"].append(values), case["g"].append(bf16_of(g))
        else:
            case["p"].append(values), case["m"].append(None), case["g"].append(g)
        case["b"].append(b)
    for key, t, i, v in raw.get("poke", ()):
        case[key][t][i] = bf16_of(np.float32(v)).item() if key == "g" and case["master"][t] else v
    return case


def from_sgd_case(scase):
    """A case of tests/sgd_oracle.py as a table of float32 rows"""
    case = dict(scase, master=[False] * len(scase["sizes"]), offsets=[tuple(o) + (0,) for o in scase["offsets"]],
                m=[None] * len(scase["sizes"]))
    return case


def group_lr(case, k):
    return S.group_lr(case, k)


def expected(case):
    """(p, g, b, m lists, counter) after the step, by the oracle"""
    P, G, B, M = [], [], [], []
    for t in range(len(case["sizes"])):
        p, g, b, m = case["p"][t], case["g"][t], case["b"][t], case["m"][t]
        if t in case["null"]:
            P.append(p.copy()), G.append(None), B.append(b.copy()), M.append(None if m is None else m.copy())
            continue
        _, mu, wd = case["groups"][case["group"][t]]
        lr = group_lr(case, case["group"][t])
        if case["master"][t]:
            nm, nb, np_ = master_step(g, m, b, lr, mu, wd)
        else:
            (np_, nb), nm = S.sgd_step(p, g, b, lr, mu, wd), None
        P.append(np_), B.append(nb), M.append(nm), G.append(np.zeros_like(g) if case["zero"] else g.copy())
    return P, G, B, M, case["counter"] + (1 if case["schedule"] is not None else 0)


def run_raw(lib, mem, case, mutate=None):
    """One ccnet_sgdmp_step call on guarded buffers of the back end ``mem``: every p, g, b and m between guard bands at the
    case's offset, the tables, the schedule and the counter guarded too.  ``mutate(args)`` may change the call's arguments (a
    dict, see below) first.  Returns (code, (p, g, b, m lists, counter), every guard band intact)."""
    n = len(case["sizes"])
    cols = {"p": 0, "g": 1, "b": 2, "m": 5}
    bufs = {key: [] for key in cols}
    tensors = np.zeros((n, TENSOR_WORDS), np.int64)
    for t, size in enumerate(case["sizes"]):
        master = case["master"][t]
        for at, (key, col) in enumerate(cols.items()):
            if (key == "g" and t in case["null"]) or (key == "m" and not master):
                bufs[key].append(None)
                continue
            kind = "bf16" if master and key in "pg" else "f32"
            buf = Buf(mem, f"{key}{t}", kind, size, offset=case["offsets"][t][at], data=case[key][t])
            bufs[key].append(buf)
            tensors[t, col] = buf.ptr
        tensors[t, 3:5] = [size, case["group"][t]]
    chunks = S.plan(case["sizes"])
    tdev = Buf(mem, "tensors", "f64", tensors.size, data=tensors)
    cdev = Buf(mem, "chunks", "f32", chunks.size, data=chunks)
    sched = counter = None
    if case["schedule"] is not None:
        table = np.asarray(case["schedule"], np.float32)
        sched = Buf(mem, "schedule", "f32", table.size, data=table)
        counter = Buf(mem, "counter", "f32", 1, data=np.array([case["counter"]], np.int32))
    lr, mu, wd = (np.array([g[k] for g in case["groups"]], np.float32) for k in range(3))
    args = {"tensors_host": tensors, "tensors_device": tdev.ptr, "n_tensors": n, "chunks_host": chunks,
            "chunks_device": cdev.ptr, "n_chunks": len(chunks), "lr": lr, "wd": wd, "mu": mu, "n_groups": len(case["groups"]),
            "schedule": sched.ptr if sched else None, "schedule_len": len(case["schedule"]) if sched else 0,
            "counter": counter.ptr if counter else None, "zero_grads": int(case["zero"]), "cap": case["cap"]}
    if mutate is not None:
        mutate(args)
    host = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data          # noqa: E731
    keep = [np.ascontiguousarray(args[k]) if args[k] is not None else None for k in ("tensors_host", "chunks_host", "lr", "wd", "mu")]
    code = lib.ccnet_sgdmp_step(host(keep[0]), args["tensors_device"], args["n_tensors"], host(keep[1]), args["chunks_device"],
                                args["n_chunks"], host(keep[2]), host(keep[3]), host(keep[4]), args["n_groups"], args["schedule"],
                                args["schedule_len"], args["counter"], args["zero_grads"], args["cap"], mem.stream)
    intact, out = True, {}
    for key in cols:
        out[key] = []
        for buf in bufs[key]:
            data, ok = buf.read(np.uint16 if buf.kind == "bf16" else np.float32) if buf is not None else (None, True)
            out[key].append(data)
            intact = intact and ok
    intact = intact and all(b.read(np.uint8)[1] for b in (tdev, cdev, sched, counter) if b is not None)
    count = int(counter.read(np.int32)[0][0]) if counter is not None else case["counter"]
    return code, (out["p"], out["g"], out["b"], out["m"], count), intact


def bits(a):
    return a if a.dtype == np.uint16 else a.view(np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.dtype in (np.float32, np.uint16) and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_matches(case, got, want=None):
    """Every p, g, b and m bit for bit the oracle's (NaN payloads aside: a NaN wherever the oracle has one), and the counter"""
    want = expected(case) if want is None else want
    for key, mine, theirs in zip("pgbm", got[:4], want[:4]):
        for t, (a, e) in enumerate(zip(mine, theirs)):
            if e is None:
                assert a is None, f"{case['name']}: {key}{t}"
                continue
            assert a.dtype == e.dtype and a.shape == e.shape, f"{case['name']}: {key}{t}: {a.dtype}{a.shape}"
            nan, mine_nan = (is_nan16(e), is_nan16(a)) if e.dtype == np.uint16 else (np.isnan(e), np.isnan(a))
            assert np.array_equal(mine_nan, nan), f"{case['name']}: {key}{t}: NaN positions differ"
            zero = np.zeros((), e.dtype)
            assert same_bits(np.where(nan, zero, a), np.where(nan, zero, e)), \
                f"{case['name']}: {key}{t}: {int((bits(a) != bits(e)).sum())} of {a.size} elements differ"
    assert got[4] == want[4], f"{case['name']}: counter {got[4]}, expected {want[4]}"


def unchanged(case, got):
    """True when every p, g, b and m and the counter are bitwise the inputs (a refused call wrote nothing)"""
    ok = got[4] == case["counter"]
    for key, mine in zip("pgbm", got[:4]):
        for t, a in enumerate(mine):
            ok = ok and (a is None or np.array_equal(bits(a), bits(case[key][t])))
    return ok
