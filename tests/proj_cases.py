"""One driver and one case table for libccnet_proj.so (include/ccnet_proj.h): the bf16 projection GEMM, the weight packer and the
column sums, shared by the SIMT-emulator tests (tests/test_emu_proj.py, ``HostMemory``) and the device tests
(tests/test_gpu_proj.py, ``DeviceMemory``).  A plain module, test infrastructure only.

Every buffer of a call sits between two guard bands (``cca_cases.Arena``); inputs' gaps, the bands and the outputs are prefilled
with a quiet NaN.  ``Arena.settle`` compares bit patterns after the call: bands intact, every input unchanged, every element
of an output buffer outside the (M, N) result unchanged -- columns N .. ldo of its rows and the two rows past M that every
output buffer carries -- and no NaN inside the result.

The bars are derived, not measured:
    GEMM      |got - ref| <= 2^-8 |ref| + 2e-6 mag against the fp64 product of the same bf16 operands, mag = |A| |Wt|^T + |bias| +
              |add|: 2e-6 mag is the project's bar for an fp32 accumulation in MFMA order (cca_cases._within), 2^-8 |ref| one bf16
              ulp (8 significant bits) for the single rounding of the result
    colsum    |got - ref| <= 2^-23 |ref| + 1e-12 sum |d| against the fp64 sum: a double accumulation (2^-53 per addition, far
              below 1e-12 of the magnitude at any row count here) and one rounding to fp32 (half an ulp <= 2^-24 |ref|)
    placement, epilogue, pack: bit for bit
"""
import numpy as np

from cca_cases import Arena, View, bf16_bits, bf16_vals, f32_bits

# (M, N, K): smallest shape | nk = 1, one row past a tile | nk = 2, K tail, N tail | nk = 3, five n tiles | nk = 9, K tail |
# the module's forward and dx shapes at (2,64,20,24) | the same at (1,512,17,19): the workload's real K and N with a small M
GEMM_CASES = [(1, 8, 8), (257, 128, 64), (255, 136, 72), (300, 640, 192), (513, 72, 520), (960, 80, 64), (960, 64, 80),
              (323, 640, 512), (323, 512, 640)]
# name -> (bias, addend, form): both values of each of the three, on guarded buffers throughout
GEMM_VARIANTS = {"bias-add-dense": (True, True, "dense"), "plain-dense": (False, False, "dense"),
                 "bias-packed": (True, False, "packed"), "add-packed": (False, True, "packed")}
PLACEMENT_CASES = [(1, 8), (257, 64), (300, 136)]          # (M, K = N): nk = 1 and nk = 3 with a K tail and an N tail
EPILOGUE_CASES = [(1, 8, 8), (300, 136, 72), (257, 640, 64)]
PACK_CASES = [(16, 2), (64, 8), (200, 25), (72, 12)]       # (C, Cq)
COLSUM_CASES = [(1, 8, 0), (4097, 80, 0), (70000, 640, 0), (4097, 80, 12)]      # (M, N, extra row stride): the last is the strided form


def gemm_ids():
    return [("x".join(map(str, mnk)), v) for mnk in GEMM_CASES for v in GEMM_VARIANTS]


def _mnk(cid):
    return tuple(int(t) for t in cid.split("x"))


_INPUTS = {}           # (M, N, K) -> operands and the fp64 reference parts, computed once and left unchanged


def gemm_inputs(mnk):
    if mnk not in _INPUTS:
        M, N, K = mnk
        rng = np.random.default_rng(1000003 * M + 1009 * N + K)
        a, w, add = (bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((M, K), (N, K), (M, N)))
        bias = rng.standard_normal(N, dtype=np.float32)
        a64, w64 = bf16_vals(a).astype(np.float64), bf16_vals(w).astype(np.float64)
        ref = dict(prod=a64 @ w64.T, mag=np.abs(a64) @ np.abs(w64).T)
        for v in (a, w, add, bias, ref["prod"], ref["mag"]):
            v.setflags(write=False)
        _INPUTS[mnk] = (a, w, add, bias, ref)
    return _INPUTS[mnk]


def _matrix(ar, name, kind, rows, cols, data, al, spare=0):
    """(rows, cols) with a row stride in a buffer of its own: ``packed`` = the column slice at offset ``al`` of rows 2 ``al``
    wider.  ``spare`` more rows (NaN) follow the matrix inside the buffer; the view returned covers the matrix alone."""
    if data is not None and spare:
        data = np.concatenate([np.asarray(data), np.full((spare, cols), 0x7FC0, np.uint16)])
    if ar.form == "packed":
        full = ar.view(name, kind, 1, rows + spare, cols, data, al, lead=al, wide=cols + 2 * al)
    else:
        full = ar.view(name, kind, 1, rows + spare, cols, data, al)
    return View(full.buf, full.off, 1, rows, cols, full.bs, full.ps)


def launch_gemm(lib, mem, form, a_, w_, bias_, add_, what="gemm_bf16"):
    """one guarded call of ccnet_proj_gemm_bf16 -> the (M, N) result as bf16 bit patterns"""
    M, K = a_.shape
    N = w_.shape[0]
    ar = Arena(mem, form, True)
    a, w = _matrix(ar, "a", "bf16", M, K, a_, 8), _matrix(ar, "wt", "bf16", N, K, w_, 8)
    bias = ar.flat("bias", "f32", N, f32_bits(bias_)) if bias_ is not None else None
    add = _matrix(ar, "add", "bf16", M, N, add_, 4) if add_ is not None else None
    out = _matrix(ar, "out", "bf16", M, N, None, 4, spare=2)
    assert out.ps % 4 == 0 and (form != "packed" or out.ps > N)
    lib.check(lib.ccnet_proj_gemm_bf16(a.ptr, w.ptr, bias.ptr if bias else None, add.ptr if add else None, out.ptr, M, N, K,
                                       a.ps, w.ps, add.ps if add else 0, out.ps, mem.stream), what)
    ar.settle(what, (out,))
    return ar.get(out)[0]


def gemm_bits(lib, mem, cid, variant):
    """the guarded call of one case -> the result's bf16 bit patterns"""
    use_bias, use_add, form = GEMM_VARIANTS[variant]
    a, w, add, bias, ref = gemm_inputs(_mnk(cid))
    return launch_gemm(lib, mem, form, a, w, bias if use_bias else None, add if use_add else None)


def run_gemm(lib, mem, cid, variant):
    mnk = _mnk(cid)
    use_bias, use_add, form = GEMM_VARIANTS[variant]
    a, w, add, bias, ref = gemm_inputs(mnk)
    got = bf16_vals(gemm_bits(lib, mem, cid, variant)).astype(np.float64)
    want, mag = ref["prod"], ref["mag"]
    if use_bias:
        want, mag = want + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    if use_add:
        a64 = bf16_vals(add).astype(np.float64)
        want, mag = want + a64, mag + np.abs(a64)
    err, bar = np.abs(got - want), 2.0 ** -8 * np.abs(want) + 2e-6 * mag
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f"gemm {cid} {variant}: max err {err.max():.3e}, worst err/bar {float((err / (bar + 1e-300)).max()):.3f}")
    assert bool((err <= bar).all()), (cid, variant, worst, float(err[worst]), float(bar[worst]))


def run_placement(lib, mem, M, K, form="packed"):
    """K = N, Wt = identity, no bias, no addend: out is A, bit for bit"""
    rng = np.random.default_rng(7 * M + K)
    a = bf16_bits(rng.standard_normal((M, K), dtype=np.float32))
    eye = bf16_bits(np.eye(K, dtype=np.float32))
    got = launch_gemm(lib, mem, form, a, eye, None, None, "gemm_bf16(identity)")
    assert np.array_equal(got, a), np.argwhere(got != a)[:4].tolist()


def run_epilogue(lib, mem, mnk, form="dense"):
    """A = 0: out is bf16_rne(float(bias) + float(add)), bit for bit"""
    M, N, K = mnk
    rng = np.random.default_rng(11 * M + 3 * N + K)
    w, add = (bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((N, K), (M, N)))
    bias = rng.standard_normal(N, dtype=np.float32)
    got = launch_gemm(lib, mem, form, np.zeros((M, K), np.uint16), w, bias, add, "gemm_bf16(A = 0)")
    want = bf16_bits(bias[None, :] + bf16_vals(add))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


def run_pack(lib, mem, C, cq, f32):
    """bit-identical to: cat, transpose, RNE of fp32 parameters (copy of bf16 ones), bias widened to fp32"""
    n = 2 * cq + C
    rng = np.random.default_rng(C + 31 * cq)
    g = lambda *s: rng.standard_normal(s, dtype=np.float32)                     # noqa: E731
    p = dict(wq=g(cq, C), bq=g(cq), wk=g(cq, C), bk=g(cq), wv=g(C, C), bv=g(C))
    ar = Arena(mem, "dense", True)
    kind, enc = ("f32", f32_bits) if f32 else ("bf16", bf16_bits)
    t = {k: ar.flat(k, kind, v.size, enc(v)) for k, v in p.items()}
    w, wt, b = ar.flat("w", "bf16", n * C), ar.flat("wt", "bf16", C * n), ar.flat("b", "f32", n)
    lib.check(lib.ccnet_proj_pack(t["wq"].ptr, t["bq"].ptr, t["wk"].ptr, t["bk"].ptr, t["wv"].ptr, t["bv"].ptr, 1 if f32 else 0,
                                  w.ptr, wt.ptr, b.ptr, C, cq, mem.stream), "pack")
    ar.settle("pack", (w, wt, b))
    wbits = bf16_bits(np.concatenate([p["wq"], p["wk"], p["wv"]]))
    bvals = np.concatenate([p["bq"], p["bk"], p["bv"]])
    if not f32:
        bvals = bf16_vals(bf16_bits(bvals))
    assert np.array_equal(ar.get(w).reshape(n, C), wbits)
    assert np.array_equal(ar.get(wt).reshape(C, n), wbits.T)
    assert np.array_equal(ar.get(b).ravel(), f32_bits(bvals))


def run_colsum(lib, mem, M, N, extra):
    rng = np.random.default_rng(M + 13 * N)
    d = bf16_bits(rng.standard_normal((M, N), dtype=np.float32) + 0.25)
    nbytes = lib.ccnet_proj_colsum_workspace_bytes(M, N)
    assert nbytes > 0 and nbytes % 8 == 0
    results = []
    for zero in (False, True, False):            # the workspace holds NaN, zero bytes, NaN: the same bits every time
        ar = Arena(mem, "dense", True)
        dv = ar.view("d", "bf16", 1, M, N, d, 4, ps=N + extra) if extra else ar.view("d", "bf16", 1, M, N, d, 4)
        assert dv.ps == N + extra
        db = ar.flat("db", "f32", N)
        ws = ar.workspace("workspace", nbytes, zero)
        lib.check(lib.ccnet_proj_colsum_bf16(dv.ptr, db.ptr, M, N, dv.ps, ws.ptr, nbytes, mem.stream), "colsum_bf16")
        ar.settle("colsum_bf16", (db,), unspecified=(ws,))
        results.append(ar.get(db).ravel())
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2]), "the column sums are not reproducible"
    d64 = bf16_vals(d).astype(np.float64)
    ref, mag = d64.sum(0), np.abs(d64).sum(0)
    err = np.abs(results[0].view(np.float32).astype(np.float64) - ref)
    bar = 2.0 ** -23 * np.abs(ref) + 1e-12 * mag
    print(f"colsum {M}x{N}+{extra}: max err {err.max():.3e}, worst err/bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all())
