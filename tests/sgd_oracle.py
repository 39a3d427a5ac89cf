"""What the optimiser tests share: the arithmetic of include/ccnet_sgd.h restated in NumPy float32 (one rounding per
operation), the chunk plan restated, the case table, the seeded input builder and the guarded-buffer driver of the C ABI.

The oracle is the contract: torch.optim.SGD's own result is compared against it, within a derived bound, by
tests/test_gpu_sgd.py.  Everything here is test infrastructure.
"""
import numpy as np

from ccnet_amd._sgd_lib import CHUNK as C
from ccnet_amd._sgd_lib import TENSOR_WORDS
from guarded_memory import Buf

DEFAULT = (0.01, 0.9, 5e-4)                   # (lr, mu, wd) of a group


def sgd_step(p, g, b, lr, mu, wd):
    """(p', b') of one step on float32 arrays: every product and every sum rounded to float32 on its own"""
    assert p.dtype == g.dtype == b.dtype == np.float32
    lr, mu, wd = np.float32(lr), np.float32(mu), np.float32(wd)
    with np.errstate(all="ignore"):
        d = g + wd * p
        nb = mu * b + d
        return p - lr * nb, nb


def plan(sizes, chunk=C):
    """The chunk table: (tensor, chunk in the tensor) pairs, tensors in order"""
    rows = [(t, k) for t, n in enumerate(sizes) for k in range((n + chunk - 1) // chunk)]
    return np.array(rows, np.int32).reshape(-1, 2)


def make_data(n, seed):
    """N(0, 1) float32 with about one exact zero in sixteen and nothing subnormal"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    x[np.abs(x) < 1e-30] = 1.0
    x[rng.random(n) < 1 / 16] = 0.0
    return x


ALIGNED = (0, 0, 0)
SCHEDULE = (0.02, 0.015, 0.01, 0.005)

# name: sizes, and where they differ from the defaults: offsets (per tensor, the (p, g, b) element offsets from a 16-byte
# boundary), groups ((lr, mu, wd) each) and group (per tensor), null (tensors without a gradient), zero (zero_grads, on by
# default), cap, schedule / counter (the device-side LR table; the groups' lr are then multipliers), poke ((tensor, element,
# value) into g)
CASES = {
    "one": {"sizes": [1]},
    "tails": {"sizes": [1, 2, 3, 4, 5, 7, 8, 9]},
    "chunk_edges": {"sizes": [C - 1, C, C + 1, 2 * C + 3]},
    "misaligned": {"sizes": [37] * 5, "offsets": [(1, 0, 0), (0, 2, 0), (0, 0, 3), (3, 3, 3), ALIGNED]},
    "many_tiny": {"sizes": [1 + k % 11 for k in range(300)]},
    "grid_stride_3": {"sizes": [3 * C + 5, 1, 2 * C], "cap": 3},
    "grid_stride_1": {"sizes": [3 * C + 5, 1, 2 * C], "cap": 1},
    "null_grad": {"sizes": [9, 130, 4, 1024, 6], "null": (1, 4)},
    "zero_on": {"sizes": [5, C + 2, 64], "zero": True, "offsets": [ALIGNED, ALIGNED, (1, 1, 1)]},
    "zero_off": {"sizes": [5, C + 2, 64], "zero": False, "offsets": [ALIGNED, ALIGNED, (1, 1, 1)]},
    "groups": {"sizes": [33, 1030, 7, 260, 12, 5], "groups": [DEFAULT, (0.1, 0.0, 0.0), (0.0, 0.5, 1e-2)],
               "group": [0, 1, 2, 2, 1, 0]},
    "nonfinite": {"sizes": [40, 19], "poke": [(0, 5, np.inf), (0, 22, np.nan), (1, 18, -np.inf), (1, 3, np.nan)]},
}
for _s in (0, 3, 9):                           # 9: past the table, clamped to its last entry
    CASES[f"schedule_{_s}"] = {"sizes": [70, 2 * C + 1, 3], "schedule": SCHEDULE, "counter": _s,
                               "groups": [(1.0, 0.9, 5e-4)]}
    CASES[f"mult_{_s}"] = {"sizes": [70, 2 * C + 1, 3, 18], "schedule": SCHEDULE, "counter": _s,
                           "groups": [(1.0, 0.9, 5e-4), (10.0, 0.9, 5e-4)], "group": [0, 1, 0, 1]}


def build_case(name):
    """The case with every default filled in and its seeded inputs: dict with sizes, offsets, groups, group, null, zero, cap,
    schedule, counter and the float32 lists p, g, b"""
    raw = CASES[name]
    sizes = list(raw["sizes"])
    n = len(sizes)
    case = {"name": name, "sizes": sizes, "offsets": list(raw.get("offsets", [ALIGNED] * n)),
            "groups": list(raw.get("groups", [DEFAULT])), "group": list(raw.get("group", [0] * n)),
            "null": tuple(raw.get("null", ())), "zero": bool(raw.get("zero", True)),
            "cap": raw.get("cap", 0), "schedule": raw.get("schedule"), "counter": raw.get("counter", 0)}
    seed = list(CASES).index(name) * 4096
    case["p"] = [make_data(s, seed + 3 * t) for t, s in enumerate(sizes)]
    case["g"] = [make_data(s, seed + 3 * t + 1) for t, s in enumerate(sizes)]
    case["b"] = [make_data(s, seed + 3 * t + 2) for t, s in enumerate(sizes)]
    for t, i, v in raw.get("poke", ()):
        case["g"][t][i] = v
    return case


def group_lr(case, k):
    """The float32 learning rate the kernel uses for group k"""
    lr = np.float32(case["groups"][k][0])
    if case["schedule"] is None:
        return lr
    table = np.asarray(case["schedule"], np.float32)
    return table[min(max(case["counter"], 0), len(table) - 1)] * lr          # (float32 * float32: rounded once)


def expected(case):
    """(p, g, b lists, counter) after the step, by the oracle"""
    P, G, B = [], [], []
    for t in range(len(case["sizes"])):
        p, g, b = case["p"][t], case["g"][t], case["b"][t]
        if t in case["null"]:
            P.append(p.copy()), G.append(None), B.append(b.copy())
            continue
        _, mu, wd = case["groups"][case["group"][t]]
        np_, nb = sgd_step(p, g, b, group_lr(case, case["group"][t]), mu, wd)
        P.append(np_), B.append(nb), G.append(np.zeros_like(g) if case["zero"] else g.copy())
    return P, G, B, case["counter"] + (1 if case["schedule"] is not None else 0)


def run_raw(lib, mem, case, mutate=None):
    """One ccnet_sgd_step call on guarded buffers of the back end ``mem``: every p, g and b between guard bands at the case's
    element offset, the tables, the schedule and the counter guarded too.  ``mutate(args)`` may change the call's arguments (a
    dict, see below) first.  Returns (code, (p, g, b lists, counter), every guard band intact)."""
    n = len(case["sizes"])
    bufs = {"p": [], "g": [], "b": []}
    tensors = np.zeros((n, TENSOR_WORDS), np.int64)
    for t, size in enumerate(case["sizes"]):
        for col, key in enumerate("pgb"):
            if key == "g" and t in case["null"]:
                bufs[key].append(None)
                continue
            buf = Buf(mem, f"{key}{t}", "f32", size, offset=case["offsets"][t][col], data=case[key][t])
            bufs[key].append(buf)
            tensors[t, col] = buf.ptr
        tensors[t, 3:] = [size, case["group"][t]]
    chunks = plan(case["sizes"])
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
    code = lib.ccnet_sgd_step(host(keep[0]), args["tensors_device"], args["n_tensors"], host(keep[1]), args["chunks_device"],
                              args["n_chunks"], host(keep[2]), host(keep[3]), host(keep[4]), args["n_groups"], args["schedule"],
                              args["schedule_len"], args["counter"], args["zero_grads"], args["cap"], mem.stream)
    intact, out = True, {}
    for key in "pgb":
        out[key] = []
        for buf in bufs[key]:
            data, ok = buf.read(np.float32) if buf is not None else (None, True)
            out[key].append(data)
            intact = intact and ok
    intact = intact and all(b.read(np.uint8)[1] for b in (tdev, cdev, sched, counter) if b is not None)
    count = int(counter.read(np.int32)[0][0]) if counter is not None else case["counter"]
    return code, (out["p"], out["g"], out["b"], count), intact


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_matches(case, got, want=None):
    """Every p, g and b bit for bit the oracle's (NaN payloads aside: a NaN wherever the oracle has one), and the counter"""
    want = expected(case) if want is None else want
    for key, mine, theirs in zip("pgb", got[:3], want[:3]):
        for t, (a, e) in enumerate(zip(mine, theirs)):
            if e is None:
                assert a is None
                continue
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(a), nan), f"{case['name']}: {key}{t}: NaN positions differ"
            assert same_bits(np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), e)), \
                f"{case['name']}: {key}{t}: {int((a.view(np.uint32) != e.view(np.uint32)).sum())} of {a.size} elements differ"
    assert got[3] == want[3], f"{case['name']}: counter {got[3]}, expected {want[3]}"


def unchanged(case, got):
    """True when every p, g and b and the counter are bitwise the inputs (a refused call wrote nothing)"""
    ok = got[3] == case["counter"]
    for key, mine in zip("pgb", got[:3]):
        for t, a in enumerate(mine):
            ok = ok and (a is None or np.array_equal(a.view(np.uint32), case[key][t].view(np.uint32)))
    return ok
