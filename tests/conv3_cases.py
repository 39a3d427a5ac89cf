"""One driver and one case table for libccnet_conv3.so (include/ccnet_conv3.h): the implicit-GEMM 3x3 convolution (forward and
input gradient through one entry point), the weight gradient with its finishing launch and the packer, shared by the
SIMT-emulator tests (tests/test_emu_conv3.py, ``HostMemory``) and the device tests (tests/test_gpu_conv3.py, ``DeviceMemory``).
A plain module, test infrastructure only.

Every buffer of a call sits between two guard bands (``cca_cases.Arena``); inputs' gaps, the bands and the outputs are prefilled
with a quiet NaN.  ``Arena.settle`` compares bit patterns after the call: bands intact, every input unchanged, every element of
an output buffer outside the (B H W, N) result unchanged -- columns N .. ldo of its rows and the two rows past B H W that every
output buffer carries -- and no NaN inside the result.  Inputs are N(0, 1) rounded to bf16; the fp64 references
(tests/conv3_oracle.py) are computed once per shape, shared and left unchanged.

The bars are derived, not measured:
    forward, adjoint   |got - ref| <= 2^-8 |ref| + 2e-6 mag, mag = sum |a| |wt| + |bias| + |add|: 2e-6 mag is the project's bar
                       for an fp32 accumulation in MFMA order, 2^-8 |ref| one bf16 ulp for the single rounding of the result
    dW                 <= 2e-6 mag for the fp32 finish, + 2^-8 |ref| for the bf16 finish, mag = sum |dy| |x|; the finish itself is
                       held bit for bit to the fp32 sum of the partials in slab order
    tap geometry, epilogue, one-hot dy, pack: bit for bit
"""
import numpy as np

import conv3_oracle as O
from cca_cases import Arena, bf16_bits, bf16_vals, f32_bits
from proj_cases import _matrix

# name -> (bias, addend, form): both values of each of the three, on guarded buffers throughout
VARIANTS = {"bias-add-dense": (True, True, "dense"), "plain-dense": (False, False, "dense"),
            "bias-packed": (True, False, "packed"), "add-packed": (False, True, "packed")}
ALL = tuple(VARIANTS)

# (B, H, W, Cin, Cout, d), the variants run, the directions run ("fwd": a = x, K = Cin, N = Cout; "adj": a = dy, K = Cout, N = Cin)
CONV_CASES = [
    ((1, 5, 7, 64, 8, 1), ALL, ("fwd", "adj")),                       # one partial tile, nk = 9; adjoint: K = 8 (a K tail), N = 64
    ((1, 3, 5, 64, 8, 4), ("bias-add-dense",), ("fwd", "adj")),       # a dilation larger than the map: the centre tap alone
    ((2, 9, 15, 64, 64, 2), ALL, ("fwd", "adj")),                     # 270 rows: a full tile across the image boundary at row 135 + 14 rows
    ((1, 5, 7, 128, 8, 1), ("plain-dense",), ("fwd",)),               # two k steps per tap, nk = 18
    ((1, 5, 7, 192, 8, 2), ("bias-packed",), ("fwd",)),               # nk = 27
    ((1, 5, 7, 72, 8, 1), ("add-packed",), ("fwd", "adj")),           # a K tail inside a tap
    ((1, 5, 7, 8, 8, 2), ("bias-add-dense",), ("fwd", "adj")),        # every k step a tail
    ((1, 5, 7, 64, 136, 1), ("bias-packed",), ("fwd", "adj")),        # two N tiles, the second partial; adjoint: K = 136
    ((1, 5, 7, 64, 4, 1), ("add-packed",), ("fwd",)),                 # N = 4, the kernel's smallest (the adjoint would need K = 4)
    ((1, 1, 1, 16, 8, 1), ("bias-add-dense",), ("fwd", "adj")),       # one pixel
    ((1, 1, 1, 16, 8, 2), ("plain-dense",), ("fwd", "adj")),
    ((1, 1, 20, 16, 8, 1), ("bias-packed",), ("fwd", "adj")),         # one row
    ((1, 1, 20, 16, 8, 2), ("add-packed",), ("fwd", "adj")),
    ((1, 20, 1, 16, 8, 1), ("bias-add-dense",), ("fwd", "adj")),      # one column
    ((1, 20, 1, 16, 8, 2), ("plain-dense",), ("fwd", "adj")),
    ((1, 6, 10, 256, 256, 2), ("plain-dense",), ("fwd", "adj")),      # the model's channel pairs at a small map: layer3
    ((1, 6, 10, 512, 512, 4), ("add-packed",), ("fwd", "adj")),       # layer4, convb
    ((1, 6, 10, 1024, 512, 1), ("bias-packed",), ("fwd", "adj")),     # the DSN head, with its bias
    ((1, 4, 4, 2560, 512, 1), ("plain-dense",), ("fwd", "adj")),      # the bottleneck after the concat
]
# (B, H, W, K = N, d): wt one-hot on one tap -- nk = 9 with every step a tail | a boundary-spanning tile | a tail after a full step
TAP_CASES = [(1, 5, 7, 8, 1), (2, 9, 15, 64, 2), (1, 3, 5, 72, 4), (1, 1, 20, 8, 2), (1, 20, 1, 8, 1)]
EPILOGUE_CASES = [(1, 1, 1, 8, 8, 1), (2, 9, 15, 72, 136, 2)]           # (B, H, W, K, N, d)
# (B, H, W, N = Cout, C = Cin, d, S, form): S forced through the entry point's argument (0: the library's own choice)
WGRAD_CASES = [
    (1, 5, 7, 8, 64, 1, 1, "dense"),            # 35 rows: no multiple of 64
    (2, 9, 15, 64, 64, 2, 2, "packed"),         # 270 rows, slabs of 192 and 78 across the image boundary
    (1, 10, 10, 136, 72, 1, 3, "dense"),        # 100 rows in slabs of 64: the third slab has no rows; two n tiles, a C tail
    (1, 6, 10, 16, 264, 4, 1, "packed"),        # two c tiles, the second partial
    (1, 6, 10, 256, 256, 2, 0, "dense"),        # layer3's pair, the library's slab count
    (1, 4, 4, 512, 2560, 1, 0, "dense"),        # the bottleneck's pair: tiles alone exceed the CU count, S = 1
    (1, 5, 7, 8, 16, 1, 3, "dense"),            # 35 rows in three slabs of 64: two slabs start past the last row
    (1, 1, 1, 8, 8, 1, 1, "dense"), (1, 1, 20, 8, 16, 2, 2, "packed"), (1, 20, 1, 8, 16, 1, 1, "dense"),
]
ONEHOT_CASES = [(2, 5, 7, 16, 24, 2, (1, 2, 3)), (2, 5, 7, 16, 24, 2, (0, 0, 6)), (1, 3, 5, 8, 8, 4, (0, 1, 1))]   # .., (b, h, w) of the one
PACK_CASES = [(8, 8), (16, 24), (136, 72)]      # (Cout, Cin)


def sid(shape):
    B, H, W, ci, co, d = shape
    return f"{B}x{H}x{W}-{ci}-{co}-d{d}"


def conv_ids():
    return [(sid(s), direction, v) for s, vs, ds in CONV_CASES for direction in ds for v in vs]


_SHAPES = {sid(s): s for s, _, _ in CONV_CASES}
_INPUTS, _REFS = {}, {}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def conv_inputs(shape):
    """bf16 bit patterns of x, w, dy and the two addends, an fp32 bias per direction: made once per shape"""
    if shape not in _INPUTS:
        B, H, W, ci, co, d = shape
        rng = np.random.default_rng(1000003 * H * W + 1009 * ci + 31 * co + d + 7 * B)
        g = lambda *s: bf16_bits(rng.standard_normal(s, dtype=np.float32))         # noqa: E731
        t = dict(x=g(B, H, W, ci), w=g(co, ci, 3, 3), dy=g(B, H, W, co), add_fwd=g(B, H, W, co), add_adj=g(B, H, W, ci),
                 bias_fwd=rng.standard_normal(co, dtype=np.float32), bias_adj=rng.standard_normal(ci, dtype=np.float32))
        _freeze(*t.values())
        _INPUTS[shape] = t
    return _INPUTS[shape]


def operands(shape, direction):
    """(a bits (B, H, W, K), wt bits (N, 9 K), bias, add bits) of one direction"""
    t = conv_inputs(shape)
    if direction == "fwd":
        return t["x"], O.pack_forward(t["w"]), t["bias_fwd"], t["add_fwd"]
    return t["dy"], O.pack_adjoint(t["w"]), t["bias_adj"], t["add_adj"]


def conv_reference(shape, direction):
    """fp64 product and magnitude of one direction, without bias and addend: computed once"""
    key = (shape, direction)
    if key not in _REFS:
        a, wt, _, _ = operands(shape, direction)
        a64, w64 = bf16_vals(a).astype(np.float64), bf16_vals(wt).astype(np.float64)
        ref = (O.conv_rows(a64, w64, shape[5]), O.conv_rows(np.abs(a64), np.abs(w64), shape[5]))
        _freeze(*ref)
        _REFS[key] = ref
    return _REFS[key]


def launch_conv(lib, mem, form, a_, wt_, bias_, add_, d, what="conv3_bf16"):
    """one guarded call of ccnet_conv3_bf16 -> the (B H W, N) result as bf16 bit patterns"""
    B, H, W, K = a_.shape
    M, N = B * H * W, wt_.shape[0]
    ar = Arena(mem, form, True)
    a = _matrix(ar, "a", "bf16", M, K, np.asarray(a_).reshape(M, K), 8)
    w = ar.flat("wt", "bf16", N * 9 * K, wt_)
    bias = ar.flat("bias", "f32", N, f32_bits(bias_)) if bias_ is not None else None
    add = _matrix(ar, "add", "bf16", M, N, np.asarray(add_).reshape(M, N), 4) if add_ is not None else None
    out = _matrix(ar, "out", "bf16", M, N, None, 4, spare=2)
    assert a.ps % 8 == 0 and out.ps % 4 == 0 and (form != "packed" or (out.ps > N and a.ps > K))
    lib.check(lib.ccnet_conv3_bf16(a.ptr, w.ptr, bias.ptr if bias else None, add.ptr if add else None, out.ptr, B, H, W, K, N, d,
                                   a.ps, add.ps if add else 0, out.ps, mem.stream), what)
    ar.settle(what, (out,))
    return ar.get(out)[0]


def conv_bits(lib, mem, cid, direction, variant):
    use_bias, use_add, form = VARIANTS[variant]
    shape = _SHAPES[cid]
    a, wt, bias, add = operands(shape, direction)
    return launch_conv(lib, mem, form, a, wt, bias if use_bias else None, add if use_add else None, shape[5])


def run_conv(lib, mem, cid, direction, variant):
    use_bias, use_add, form = VARIANTS[variant]
    shape = _SHAPES[cid]
    _, wt, bias, add = operands(shape, direction)
    N = wt.shape[0]
    got = bf16_vals(conv_bits(lib, mem, cid, direction, variant)).astype(np.float64)
    want, mag = (r.reshape(-1, N) for r in conv_reference(shape, direction))
    if use_bias:
        want, mag = want + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    if use_add:
        a64 = bf16_vals(add).astype(np.float64).reshape(-1, N)
        want, mag = want + a64, mag + np.abs(a64)
    err, bar = np.abs(got - want), 2.0 ** -8 * np.abs(want) + 2e-6 * mag
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f"conv3 {cid} {direction} {variant}: max err {err.max():.3e}, worst err/bar {float((err / (bar + 1e-300)).max()):.3f}")
    assert bool((err <= bar).all()), (cid, direction, variant, worst, float(err[worst]), float(bar[worst]))


def run_tap_shift(lib, mem, case, form="packed"):
    """wt one-hot on tap t (the identity on the channels, N = K), no bias, no addend: out is the input shifted by (ky d, kx d)
    with zeros where the source is outside, bit for bit, for all nine taps"""
    B, H, W, K, d = case
    rng = np.random.default_rng(7 * H * W + K + d)
    a = bf16_bits(rng.standard_normal((B, H, W, K), dtype=np.float32))
    for t in range(9):
        wt = np.zeros((K, 9, K), np.uint16)
        wt[np.arange(K), t, np.arange(K)] = 0x3F80
        got = launch_conv(lib, mem, form, a, wt.reshape(K, 9 * K), None, None, d, f"conv3_bf16(tap {t})")
        want = O.shifted(a, t, d).reshape(-1, K)
        assert np.array_equal(got, want), (case, t, np.argwhere(got != want)[:4].tolist())


def run_epilogue(lib, mem, case, form="dense"):
    """a = 0: out is bf16_rne(float(bias) + float(add)), bit for bit"""
    B, H, W, K, N, d = case
    M = B * H * W
    rng = np.random.default_rng(11 * M + 3 * N + K)
    wt, add = (bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((N, 9 * K), (M, N)))
    bias = rng.standard_normal(N, dtype=np.float32)
    got = launch_conv(lib, mem, form, np.zeros((B, H, W, K), np.uint16), wt, bias, add, d, "conv3_bf16(a = 0)")
    want = bf16_bits(bias[None, :] + bf16_vals(add))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


def run_pack(lib, mem, co, ci, f32):
    """both packs equal NumPy index permutations of the parameter bit for bit; fp32 parameters are rounded to nearest even"""
    rng = np.random.default_rng(co + 31 * ci)
    p = rng.standard_normal((co, ci, 3, 3), dtype=np.float32)
    ar = Arena(mem, "dense", True)
    w = ar.flat("weight", "f32", p.size, f32_bits(p)) if f32 else ar.flat("weight", "bf16", p.size, bf16_bits(p))
    fwd, adj = ar.flat("fwd", "bf16", p.size), ar.flat("adj", "bf16", p.size)
    lib.check(lib.ccnet_conv3_pack(w.ptr, 1 if f32 else 0, fwd.ptr, adj.ptr, co, ci, mem.stream), "pack")
    ar.settle("pack", (fwd, adj))
    bits = bf16_bits(p)
    assert np.array_equal(ar.get(fwd).reshape(co, 9 * ci), O.pack_forward(bits))
    assert np.array_equal(ar.get(adj).reshape(ci, 9 * co), O.pack_adjoint(bits))


def launch_wgrad(lib, mem, form, dy_, x_, d, S, zero=False, what="wgrad_bf16"):
    """one guarded call of ccnet_conv3_wgrad_bf16 and of both finishes -> (part (S, 9, N, C) fp32, dw fp32 bits, dw bf16 bits, S)"""
    B, H, W, N = dy_.shape
    C, M = x_.shape[3], B * H * W
    auto = lib.ccnet_conv3_wgrad_slabs(B, H, W, N, C)
    assert auto >= 1 and auto == lib.ccnet_conv3_wgrad_slabs(B, H, W, N, C)               # a function of the shape alone
    slabs = S or auto
    nbytes = lib.ccnet_conv3_wgrad_workspace_bytes(B, H, W, N, C, S)
    assert nbytes == slabs * 9 * N * C * 4
    ar = Arena(mem, form, True)
    dy = _matrix(ar, "dy", "bf16", M, N, np.asarray(dy_).reshape(M, N), 8)
    x = _matrix(ar, "x", "bf16", M, C, np.asarray(x_).reshape(M, C), 8)
    part = ar.workspace("part", nbytes, zero)
    dw32, dw16 = ar.flat("dw32", "f32", N * C * 9), ar.flat("dw16", "bf16", N * C * 9)
    lib.check(lib.ccnet_conv3_wgrad_bf16(dy.ptr, x.ptr, part.ptr, nbytes, B, H, W, N, C, d, dy.ps, x.ps, S, mem.stream), what)
    lib.check(lib.ccnet_conv3_wgrad_finish(part.ptr, dw32.ptr, 1, N, C, slabs, mem.stream), what + "(finish fp32)")
    lib.check(lib.ccnet_conv3_wgrad_finish(part.ptr, dw16.ptr, 0, N, C, slabs, mem.stream), what + "(finish bf16)")
    ar.settle(what, (part, dw32, dw16))                                          # every element of part is written
    return ar.get(part).ravel().view(np.float32).reshape(slabs, 9, N, C), ar.get(dw32).ravel(), ar.get(dw16).ravel(), slabs


def run_wgrad(lib, mem, case):
    B, H, W, N, C, d, S, form = case
    rng = np.random.default_rng(13 * H * W + N + 3 * C + d)
    dy, x = (bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in ((B, H, W, N), (B, H, W, C)))
    part, dw32, dw16, slabs = launch_wgrad(lib, mem, form, dy, x, d, S)
    if S:
        assert slabs == S
    rows = ((B * H * W + slabs - 1) // slabs + 63) // 64 * 64
    for s in range(slabs):                          # a slab without rows holds zeros
        if s * rows >= B * H * W:
            assert not part[s].any(), s
    # the finish: the partials added in slab order in fp32, laid out (N, C, 3, 3); the bf16 form is that, rounded once
    total = part[0].copy()
    for s in range(1, slabs):
        total = (total + part[s]).astype(np.float32)
    want32 = np.ascontiguousarray(total.transpose(1, 2, 0)).ravel()
    assert np.array_equal(dw32, f32_bits(want32)), "the fp32 finish is not the sum of the partials in slab order"
    assert np.array_equal(dw16, bf16_bits(want32)), "the bf16 finish is not that sum rounded once"
    d64, x64 = bf16_vals(dy).astype(np.float64), bf16_vals(x).astype(np.float64)
    ref = O.weight_grad(d64, x64, d).ravel()
    mag = O.weight_grad(np.abs(d64), np.abs(x64), d).ravel()
    for name, got, bar in (("fp32", dw32.view(np.float32).astype(np.float64), 2e-6 * mag),
                           ("bf16", bf16_vals(dw16).astype(np.float64), 2e-6 * mag + 2.0 ** -8 * np.abs(ref))):
        err = np.abs(got - ref)
        print(f"wgrad {case} {name}: S = {slabs}, max err {err.max():.3e}, worst err/bar {float((err / (bar + 1e-300)).max()):.3f}")
        assert bool((err <= bar).all()), (case, name, int(np.argmax(err - bar)))
    return part, dw32, dw16


def run_wgrad_onehot(lib, mem, case):
    """dy one-hot in a single pixel (channel n0 = 3): part of tap t is that pixel's shifted x row in row n0, bit for bit, zero elsewhere"""
    B, H, W, N, C, d, (b, h, w) = case
    rng = np.random.default_rng(5 * H * W + N + C)
    x = bf16_bits(rng.standard_normal((B, H, W, C), dtype=np.float32))
    dy = np.zeros((B, H, W, N), np.uint16)
    n0 = 3
    dy[b, h, w, n0] = 0x3F80
    part, _, _, slabs = launch_wgrad(lib, mem, "dense", dy, x, d, 1, what="wgrad_bf16(one-hot)")
    want = np.zeros((9, N, C), np.float32)
    for t in range(9):
        want[t, n0] = bf16_vals(O.shifted(x, t, d)[b, h, w])
    assert slabs == 1 and np.array_equal(part[0].view(np.uint32), want.view(np.uint32)), np.argwhere(part[0] != want)[:4].tolist()
