"""One driver and one case table for the memory behaviour of the pixel-major and split-plane families of the attention core
(include/ccnet_cca.h: *_pm_*, *_planes_*, their producers and the projection GEMMs), shared by the SIMT-emulator tests
(tests/test_cca_bounds_host.py) and the device tests (tests/test_gpu_cca_bounds.py).  A plain module, test infrastructure only.

Every tensor of a call is laid into its buffer by a VIEW FORM:
    dense    ps = C, bs = H W C
    packed   q | k | v (and dq | dk | dv) are channel slices of one buffer, ps = 2 Cq + C (what the module does); producers and
             GEMMs read a channel / column slice at an offset > 0 of a wider tensor
    padded   ps = C + one alignment unit, bs = H W ps + one alignment unit (8 elements for bf16 and planes, 4 for fp32)
    tight    the padded ps with the smallest bs the entry point accepts; the buffer ends at the last in-view element of the
             last image, where its upper guard band starts
Every buffer -- inputs, outputs, the exact-size 256-byte aligned workspace -- sits between two guard bands of GUARD elements.
Input gaps and all bands hold a quiet NaN; outputs are prefilled with the NaN pattern throughout.  After every call
``Arena.settle`` compares bit patterns: bands intact, every element outside the views the call writes unchanged (the gaps of
outputs, every input), no NaN inside a written view.  ``run_case`` then holds the results of a form bitwise to the same call
on dense unguarded buffers, runs the form again with the workspace and scratch prefilled with zero bytes instead of NaN
(same bits), and holds the padded form to the oracle at the bars the families already have (tests/test_gpu_parity.py)."""
import numpy as np
import torch

from guarded_memory import Buf
from oracle import cca_oracle as O

GUARD = 4096                                 # guard elements on each side: a stray store lands in a band
NAN = {"f32": 0x7FC00000, "bf16": 0x7FC0}
UT = {"f32": np.uint32, "bf16": np.uint16}
FORMS = ("dense", "packed", "padded", "tight")
TOL = 1e-3                                   # tests/test_gpu_parity.py: the north_star bar (max abs, fp32)
TIGHT = 5e-5                                 # ... and what exact-fp32 energies deliver on O(1) data (the attention tensor)
HL, HLH, HHL = 2, 3, 4                       # CCNET_PLANES_*
WS = {"pm_fwd": 3, "pm_bwd": 4, "planes_fwd": 5, "planes_bwd": 6, "colsum": 7, "planes3": 8}     # CCNET_WS_*


def bf16_bits(a):
    """float32 -> bf16 bit patterns, round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_vals(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def is_nan(bits):
    if bits.dtype == np.uint16:
        return (bits & 0x7FFF) > 0x7F80
    return (bits & 0x7FFFFFFF) > 0x7F800000


def up(n, al):
    return (n + al - 1) // al * al


class View:
    """(B, P, C) elements inside ``buf``: element (b, p, c) at  off + b bs + p ps + c"""

    def __init__(self, buf, off, B, P, C, bs, ps):
        self.buf, self.off, self.B, self.P, self.C, self.bs, self.ps = buf, off, B, P, C, bs, ps
        self.ptr = buf.ptr + off * buf.size

    def idx(self):
        b, p, c = np.ogrid[:self.B, :self.P, :self.C]
        return self.off + b * self.bs + p * self.ps + c


class Arena:
    """the buffers of one run, all in one form; ``guarded`` False: no bands (the plain buffers every other test uses)"""

    def __init__(self, mem, form, guarded=True):
        self.mem, self.form, self.guard = mem, form, GUARD if guarded else 0
        self.bufs, self.images = {}, {}

    def raw(self, name, kind, n, bits=None, align=16, fill=None):
        img = np.full(n, NAN[kind] if fill is None else fill, UT[kind]) if bits is None else np.ascontiguousarray(bits, UT[kind])
        assert img.size == n and name not in self.bufs
        buf = Buf(self.mem, name, kind, n, data=img, guard=self.guard, align=align, pattern=NAN[kind])
        self.bufs[name], self.images[name] = buf, img.ravel().copy()
        return buf

    def flat(self, name, kind, n, bits=None, fill=None):
        """a dense tensor of n elements (NCHW tensors, A, scratch, vectors)"""
        return View(self.raw(name, kind, n, None if bits is None else np.asarray(bits).ravel(), fill=fill), 0, 1, 1, n, n, n)

    def workspace(self, name, nbytes, zero):
        assert nbytes % 4 == 0 and nbytes > 0
        return self.flat_ws(name, nbytes // 4, zero)

    def flat_ws(self, name, n, zero):
        buf = self.raw(name, "f32", n, align=256, fill=0 if zero else None)
        assert buf.ptr % 256 == 0
        return View(buf, 0, 1, 1, n, n, n)

    def strides(self, P, width, al, form=None, ps=None):
        """(ps, bs, elements of one buffer holding B images) -> the last as a function of B"""
        form = form or self.form
        if form in ("dense", "packed"):
            ps = ps or width
            return ps, P * ps, lambda B: B * P * ps
        ps = ps or up(width, al) + al
        if form == "padded":
            bs = P * ps + al
            return ps, bs, lambda B: B * bs
        bs = up((P - 1) * ps + width, al)                    # tight: the smallest stride the view checks accept
        return ps, bs, lambda B: (B - 1) * bs + (P - 1) * ps + width

    def view(self, name, kind, B, P, C, data, al, form=None, ps=None, lead=0, wide=0):
        """one tensor in a buffer of its own.  ``lead`` / ``wide``: the tensor is the channel slice [lead, lead + C) of rows
        ``wide`` channels across (the rest NaN)"""
        if wide:
            ps = wide if (form or self.form) in ("dense", "packed") else wide + al
        ps, bs, total = self.strides(P, C, al, form, ps)
        n = lead + total(B) if not wide or (form or self.form) == "tight" else total(B)
        buf = self.raw(name, kind, n, self._image(kind, n, [(lead, B, P, C, bs, ps, data)]))
        return View(buf, lead, B, P, C, bs, ps)

    def packed(self, name, kind, B, P, parts, al):
        """``parts`` [(name, C, data)] side by side in the rows of one buffer (form 'packed'), else one buffer each"""
        if self.form != "packed":
            return {n: self.view(n, kind, B, P, C, d, al) for n, C, d in parts}
        ps = sum(C for _, C, _ in parts)
        assert ps % al == 0
        offs = np.cumsum([0] + [C for _, C, _ in parts])
        buf = self.raw(name, kind, B * P * ps, self._image(kind, B * P * ps, [(int(o), B, P, C, P * ps, ps, d)
                                                                             for o, (_, C, d) in zip(offs, parts)]))
        return {n: View(buf, int(o), B, P, C, P * ps, ps) for o, (n, C, _) in zip(offs, parts)}

    @staticmethod
    def _image(kind, n, parts):
        img = np.full(n, NAN[kind], UT[kind])
        for off, B, P, C, bs, ps, data in parts:
            if data is not None:
                b, p, c = np.ogrid[:B, :P, :C]
                img[off + b * bs + p * ps + c] = np.asarray(data, UT[kind]).reshape(B, P, C)
        return img

    def settle(self, what, written, unspecified=()):
        """after a call: every band intact, nothing changed outside ``written`` (views whose every element the call must
        have overwritten with a number) and ``unspecified`` (scratch memory: any content)"""
        out = {}
        for name, buf in self.bufs.items():
            got, intact = buf.read(UT[buf.kind])
            assert intact, (what, "guard band written", name)
            mask = np.zeros(buf.n, bool)
            for v in written + tuple(unspecified):
                if v.buf is buf:
                    mask[v.idx().ravel()] = True
            keep = ~mask
            same = np.array_equal(got[keep], self.images[name][keep])
            assert same, (what, "written outside its view" if mask.any() else "input changed", name,
                          np.flatnonzero(keep & (got != self.images[name]))[:8])
            for v in written:
                if v.buf is buf:
                    bad = is_nan(got[v.idx()])
                    assert not bad.any(), (what, "in-view elements left unwritten or NaN", name, int(bad.sum()),
                                           np.argwhere(bad)[:4].tolist())
            self.images[name] = got
            out[name] = got
        return out

    def get(self, v):
        return self.images[v.buf.name][v.idx()].copy()


def _rng_inputs(B, C, cq, H, W, seed):
    rng = np.random.default_rng(seed)
    f = lambda c: rng.standard_normal((B, H * W, c), dtype=np.float32)                     # noqa: E731
    return dict(q=f(cq), k=f(cq), v=f(C), x=f(C), dy=f(C))


def _nchw(a, H, W):
    """(B, P, C) -> torch (B, C, H, W) float32"""
    a = np.asarray(a, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[0], H, W, a.shape[2]).transpose(0, 3, 1, 2)))


def _oracle(c, H, W, gamma):
    g = torch.tensor([gamma])
    t = {n: _nchw(c[n], H, W) for n in ("q", "k", "v", "x", "dy")}
    yo, Ao = O.cca_core_forward(t["q"], t["k"], t["v"], t["x"], g)
    go = O.cca_core_backward(t["dy"], t["q"], t["k"], t["v"], Ao, g)
    return t, yo, Ao, go, g


GAMMA = 0.5


# ---------------------------------------------------------------------------------------------------------------------
# pixel-major entry points: ccnet_cca_forward_pm_* / ccnet_cca_attention_pm / ccnet_cca_backward_pm_*
# ---------------------------------------------------------------------------------------------------------------------
def run_pm(lib, mem, form, guarded, zero, kind, shape, cq):
    B, C, H, W = shape
    P, al = H * W, 8 if kind == "bf16" else 4
    c = _rng_inputs(B, C, cq, H, W, seed=B + 3 * C + 5 * H + 7 * W)
    enc = bf16_bits if kind == "bf16" else f32_bits
    ar = Arena(mem, form, guarded)
    s = mem.stream
    qkv = ar.packed("qkv", kind, B, P, [("q", cq, enc(c["q"])), ("k", cq, enc(c["k"])), ("v", C, enc(c["v"]))], al)
    q, k, v = qkv["q"], qkv["k"], qkv["v"]
    x = ar.view("x", kind, B, P, C, enc(c["x"]), al)
    dy = ar.view("dy", kind, B, P, C, enc(c["dy"]), al)
    y = ar.view("y", kind, B, P, C, None, al)
    gamma = ar.flat("gamma", "f32", 1, f32_bits(np.float32([GAMMA])))
    A = ar.flat("A", "f32", B * P * (H + W))
    A2 = ar.flat("A2", "f32", B * P * (H + W))
    nf, nb = (lib.ccnet_cca_workspace_bytes(WS[e], B, C, cq, H, W) for e in ("pm_fwd", "pm_bwd"))
    wf, wb = ar.workspace("ws_forward", nf, zero), ar.workspace("ws_backward", nb, zero)
    fwd, bwd = ((lib.ccnet_cca_forward_pm_bf16, lib.ccnet_cca_backward_pm_bf16) if kind == "bf16" else
                (lib.ccnet_cca_forward_pm_f32, lib.ccnet_cca_backward_pm_f32))
    lib.check(fwd(q.ptr, k.ptr, v.ptr, x.ptr, gamma.ptr, y.ptr, A.ptr, B, C, cq, H, W, q.bs, q.ps, k.bs, k.ps, v.bs, v.ps,
                  x.bs, x.ps, y.bs, y.ps, wf.ptr, nf, s), "forward_pm")
    ar.settle("forward_pm", (y, A), (wf,))
    lib.check(lib.ccnet_cca_attention_pm(q.ptr, k.ptr, A2.ptr, int(kind == "bf16"), B, cq, H, W, q.bs, q.ps, k.bs, k.ps, s),
              "attention_pm")
    ar.settle("attention_pm", (A2,))
    d = ar.packed("dqkv", kind, B, P, [("dq", cq, None), ("dk", cq, None), ("dv", C, None)], al)
    dq, dk, dv = d["dq"], d["dk"], d["dv"]
    dgamma = ar.flat("dgamma", "f32", 1)
    scratch = ar.flat("scratch", "f32", B * P * (H + W), fill=0 if zero else None)
    lib.check(bwd(dy.ptr, q.ptr, k.ptr, v.ptr, A.ptr, gamma.ptr, dq.ptr, dk.ptr, dv.ptr, dgamma.ptr, scratch.ptr, B, C, cq, H, W,
                  dy.bs, dy.ps, q.bs, q.ps, k.bs, k.ps, v.bs, v.ps, dq.bs, dq.ps, dk.bs, dk.ps, dv.bs, dv.ps, wb.ptr, nb, s),
              "backward_pm")
    ar.settle("backward_pm", (dq, dk, dv, dgamma), (scratch, wb))
    # one short workspace is refused before anything is launched
    assert bwd(dy.ptr, q.ptr, k.ptr, v.ptr, A.ptr, gamma.ptr, dq.ptr, dk.ptr, dv.ptr, dgamma.ptr, scratch.ptr, B, C, cq, H, W,
               dy.bs, dy.ps, q.bs, q.ps, k.bs, k.ps, v.bs, v.ps, dq.bs, dq.ps, dk.bs, dk.ps, dv.bs, dv.ps, wb.ptr, nb - 256,
               s) == -4
    r = {n: ar.get(t) for n, t in (("y", y), ("A", A), ("A2", A2), ("dq", dq), ("dk", dk), ("dv", dv), ("dgamma", dgamma))}
    assert np.array_equal(r["A"], r["A2"]), "ccnet_cca_attention_pm: not what the forward leaves in A"
    return r


def check_pm(lib, r, kind, shape, cq):
    """the padded form against the oracle: test_pixel_major_{bf16,fp32}_kernels_match_oracle of tests/test_gpu_parity.py"""
    B, C, H, W = shape
    c = _rng_inputs(B, C, cq, H, W, seed=B + 3 * C + 5 * H + 7 * W)
    if kind == "bf16":
        c = {n: bf16_vals(bf16_bits(a)) for n, a in c.items()}
    t, yo, Ao, go, g = _oracle(c, H, W, GAMMA)
    dec = bf16_vals if kind == "bf16" else (lambda b: b.view(np.float32))
    A = torch.from_numpy(r["A"].view(np.float32).reshape(B, H, W, H + W))
    assert float((A - Ao).abs().max()) < TIGHT
    assert bool((A[:, torch.arange(H), :, torch.arange(H)] == 0).all())
    col = {}
    if kind == "bf16" and lib.get_option("bf16_partial"):
        col = {"y": g * torch.einsum("bhwj,bcjw->bchw", Ao[..., :H], t["v"]),
               "dv": g * torch.einsum("bhwj,bchw->bcjw", Ao[..., :H], t["dy"])}
    for n, ref in (("y", yo), ("dq", go["dq"]), ("dk", go["dk"]), ("dv", go["dv"])):
        got = _nchw(dec(r[n]), H, W)
        allow = TOL
        if kind == "bf16":
            allow = 2.0 ** -8 * ref.abs() + (2.0 ** -8 * col[n].abs() if n in col else 0.0) + TOL
        assert bool(((got - ref).abs() <= allow).all()), (n, float((got - ref).abs().max()))
    dg = float(r["dgamma"].view(np.float32).ravel()[0])
    assert abs(dg - float(go["dgamma"])) < 1e-3 * max(1.0, abs(float(go["dgamma"])))


# ---------------------------------------------------------------------------------------------------------------------
# split-plane entry points: ccnet_cca_forward_planes_f32 / _backward_planes_f32 / _backward_planes3_f32
# ---------------------------------------------------------------------------------------------------------------------
def run_planes(lib, mem, form, guarded, zero, shape, cq, mode, p3=False):
    """``mode``: 'free' (v fp32 pixel-major, no planes tensor), 'bias' / 'nobias' (the forward splits v (+ v_bias) into
    ``v_planes``, which the backward reads).  ``p3``: the three-plane backward as well, on the same inputs."""
    B, C, H, W = shape
    P, ct = H * W, 2 * cq + C
    seed = B + 3 * C + 5 * H + 7 * W
    c = _rng_inputs(B, C, cq, H, W, seed)
    bias = np.random.default_rng(seed + 1).standard_normal(C, dtype=np.float32) if mode == "bias" else None
    ar = Arena(mem, form, guarded)
    s = mem.stream
    qkv = ar.packed("qkv", "f32", B, P, [("q", cq, f32_bits(c["q"])), ("k", cq, f32_bits(c["k"])), ("v", C, f32_bits(c["v"]))], 4)
    q, k, v = qkv["q"], qkv["k"], qkv["v"]
    nchw = lambda a: f32_bits(np.ascontiguousarray(a.reshape(B, P, C).transpose(0, 2, 1)))              # noqa: E731
    x, dy = ar.flat("x", "f32", B * C * P, nchw(c["x"])), ar.flat("dy", "f32", B * C * P, nchw(c["dy"]))
    y = ar.flat("y", "f32", B * C * P)
    gamma = ar.flat("gamma", "f32", 1, f32_bits(np.float32([GAMMA])))
    vb = None if bias is None else ar.flat("v_bias", "f32", C, f32_bits(bias))
    A, A2 = ar.flat("A", "f32", B * P * (H + W)), ar.flat("A2", "f32", B * P * (H + W))
    vp = None
    if mode != "free":                                # (the packed form has no say about the planes: they take the padded one)
        vp = ar.view("v_planes", "bf16", B, P, 2 * C, None, 8, form="padded" if form == "packed" else None)
    nf, nb = (lib.ccnet_cca_workspace_bytes(WS[e], B, C, cq, H, W) for e in ("planes_fwd", "planes_bwd"))
    wf, wb = ar.workspace("ws_forward", nf, zero), ar.workspace("ws_backward", nb, zero)
    ptr = lambda t: None if t is None else t.ptr                                                          # noqa: E731
    vpbs, vpps = (vp.bs, vp.ps) if vp else (0, 0)
    lib.check(lib.ccnet_cca_forward_planes_f32(q.ptr, k.ptr, v.ptr, ptr(vb), ptr(vp), x.ptr, gamma.ptr, y.ptr, A.ptr, B, C, cq, H, W,
                                               q.bs, q.ps, k.bs, k.ps, v.bs, v.ps, vpbs, vpps, wf.ptr, nf, s), "forward_planes")
    ar.settle("forward_planes", (y, A) + ((vp,) if vp else ()), (wf,))
    lib.check(lib.ccnet_cca_attention_pm(q.ptr, k.ptr, A2.ptr, 0, B, cq, H, W, q.bs, q.ps, k.bs, k.ps, s), "attention_pm")
    ar.settle("attention_pm", (A2,))
    d = ar.packed("dqkv", "f32", B, P, [("dq", cq, None), ("dk", cq, None), ("dv", C, None)], 4)
    dq, dk, dv = d["dq"], d["dk"], d["dv"]
    dgamma = ar.flat("dgamma", "f32", 1)
    scratch = ar.flat("scratch", "f32", B * P * (H + W), fill=0 if zero else None)
    back = lambda nbytes: lib.ccnet_cca_backward_planes_f32(                                               # noqa: E731
        dy.ptr, q.ptr, k.ptr, None if vp else v.ptr, ptr(vp), A.ptr, gamma.ptr, dq.ptr, dk.ptr, dv.ptr, dgamma.ptr, scratch.ptr,
        B, C, cq, H, W, q.bs, q.ps, k.bs, k.ps, v.bs, v.ps, vpbs, vpps, dq.bs, dq.ps, dk.bs, dk.ps, dv.bs, dv.ps, wb.ptr, nbytes, s)
    lib.check(back(nb), "backward_planes")
    ar.settle("backward_planes", (dq, dk, dv, dgamma), (scratch, wb))
    assert back(nb - 256) == -4
    names = [("y", y), ("A", A), ("A2", A2), ("dq", dq), ("dk", dk), ("dv", dv), ("dgamma", dgamma)] + ([("v_planes", vp)] if vp else [])
    if p3:
        d3_ps = 3 * ct if form == "dense" else 3 * ct + 8
        d3 = ar.view("d3", "bf16", B, P, 3 * ct, None, 4, form="padded" if form == "packed" else None, ps=d3_ps)
        dbias, dgamma3 = ar.flat("dbias", "f32", ct), ar.flat("dgamma3", "f32", 1)
        scratch3 = ar.flat("scratch3", "f32", B * P * (H + W), fill=0 if zero else None)
        n3 = lib.ccnet_cca_workspace_bytes(WS["planes3"], B, C, cq, H, W)
        w3 = ar.workspace("ws_planes3", n3, zero)
        back3 = lambda nbytes: lib.ccnet_cca_backward_planes3_f32(                                         # noqa: E731
            dy.ptr, q.ptr, k.ptr, v.ptr, A.ptr, gamma.ptr, d3.ptr, dbias.ptr, dgamma3.ptr, scratch3.ptr, B, C, cq, H, W,
            q.bs, q.ps, k.bs, k.ps, v.bs, v.ps, d3.bs, d3.ps, w3.ptr, nbytes, s)
        lib.check(back3(n3), "backward_planes3")
        ar.settle("backward_planes3", (d3, dbias, dgamma3), (scratch3, w3))
        assert back3(n3 - 256) == -4
        names += [("d3", d3), ("dbias", dbias), ("dgamma3", dgamma3)]
    r = {n: ar.get(t) for n, t in names}
    assert np.array_equal(r["A"], r["A2"]), "ccnet_cca_attention_pm: not what the forward leaves in A"
    return r


def check_planes(lib, r, shape, cq, mode, p3=False):
    """the padded form against the oracle (TOL; the attention at TIGHT), the planes against the exact hi | lo split"""
    B, C, H, W = shape
    seed = B + 3 * C + 5 * H + 7 * W
    c = _rng_inputs(B, C, cq, H, W, seed)
    if mode == "bias":
        c["v"] = c["v"] + np.random.default_rng(seed + 1).standard_normal(C, dtype=np.float32)
    if mode != "free":
        hi = bf16_bits(c["v"])
        lo = bf16_bits(c["v"] - bf16_vals(hi))
        assert np.array_equal(r["v_planes"], np.concatenate([hi, lo], axis=2)), "v_planes: not the hi | lo split of v (+ bias)"
    t, yo, Ao, go, g = _oracle(c, H, W, GAMMA)
    A = torch.from_numpy(r["A"].view(np.float32).reshape(B, H, W, H + W))
    assert float((A - Ao).abs().max()) < TIGHT
    assert bool((A[:, torch.arange(H), :, torch.arange(H)] == 0).all())
    y = torch.from_numpy(r["y"].view(np.float32).reshape(B, C, H, W))
    assert float((y - yo).abs().max()) < TOL
    for n in ("dq", "dk", "dv"):
        got = _nchw(r[n].view(np.float32), H, W)
        assert float((got - go[n]).abs().max()) < TOL, n
    dg = float(r["dgamma"].view(np.float32).ravel()[0])
    assert abs(dg - float(go["dgamma"])) < 1e-3 * max(1.0, abs(float(go["dgamma"])))
    if p3:
        # test_three_plane_backward_writes_the_exact_split_of_the_fp32_gradients / test_three_plane_backward_on_the_device
        dqkv = np.concatenate([r["dq"], r["dk"], r["dv"]], axis=2).view(np.float32)
        hi = bf16_bits(dqkv)
        lo = bf16_bits(dqkv - bf16_vals(hi))
        assert np.array_equal(r["d3"], np.concatenate([hi, lo, hi], axis=2)), "d3: not the hi | lo | hi split of dq | dk | dv"
        assert np.array_equal(r["dgamma3"], r["dgamma"])
        ref = dqkv.astype(np.float64).sum(axis=(0, 1))
        db = r["dbias"].view(np.float32).ravel().astype(np.float64)
        assert float(np.abs(db - ref).max()) < 1e-5 * max(1.0, float(np.abs(ref).max())) + 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# producers
# ---------------------------------------------------------------------------------------------------------------------
def _planes_of(x, layout):
    hi = bf16_bits(x)
    lo = bf16_bits(x - bf16_vals(hi))
    return np.concatenate({HL: (hi, lo), HLH: (hi, lo, hi), HHL: (hi, hi, lo)}[layout], axis=-1)


def _split_source(ar, B, P, C, data):
    """the source of the split entry points: dense, else channels [8, 8 + C) of rows C + 16 channels across"""
    if ar.form == "dense":
        return ar.view("src", "f32", B, P, C, data, 4)
    return ar.view("src", "f32", B, P, C, data, 4, lead=8, wide=C + 16)


def run_split(lib, mem, form, guarded, zero, shape, layout, bias, colsum):
    """ccnet_cca_split_planes_f32 (``colsum`` False; ``bias`` given or NULL) / ccnet_cca_split_planes_colsum_f32"""
    B, C, H, W = shape
    P, npl = H * W, 2 if layout == HL else 3
    rng = np.random.default_rng(B + 3 * C + 5 * H + 7 * W + layout)
    x = rng.standard_normal((B, P, C), dtype=np.float32) * np.float32(3.0)
    ar = Arena(mem, form, guarded)
    src = _split_source(ar, B, P, C, f32_bits(x))
    dst = ar.view("dst", "bf16", B, P, npl * C, None, 8, form="padded" if form == "packed" else None)
    if colsum:
        cs = ar.flat("colsum", "f32", C)
        n = lib.ccnet_cca_workspace_bytes(WS["colsum"], B, C, 0, H, W)
        ws = ar.workspace("workspace", n, zero)
        call = lambda nbytes: lib.ccnet_cca_split_planes_colsum_f32(src.ptr, dst.ptr, cs.ptr, ws.ptr, nbytes, B, C, H, W,     # noqa: E731
                                                                    src.bs, src.ps, dst.bs, dst.ps, layout, mem.stream)
        lib.check(call(n), "split_planes_colsum")
        ar.settle("split_planes_colsum", (dst, cs), (ws,))
        assert call(n - 4) == -4
        return {"dst": ar.get(dst), "colsum": ar.get(cs)}
    b = None if not bias else ar.flat("bias", "f32", C, f32_bits(rng.standard_normal(C, dtype=np.float32)))
    lib.check(lib.ccnet_cca_split_planes_f32(src.ptr, dst.ptr, B, C, H, W, src.bs, src.ps, dst.bs, dst.ps, layout,
                                             None if b is None else b.ptr, mem.stream), "split_planes")
    ar.settle("split_planes", (dst,))
    return {"dst": ar.get(dst)}


def check_split(lib, r, shape, layout, bias, colsum):
    B, C, H, W = shape
    rng = np.random.default_rng(B + 3 * C + 5 * H + 7 * W + layout)
    x = rng.standard_normal((B, H * W, C), dtype=np.float32) * np.float32(3.0)
    if bias and not colsum:
        x = x + rng.standard_normal(C, dtype=np.float32)
    assert np.array_equal(r["dst"], _planes_of(x, layout))
    if colsum:                                    # the bar of test_split_planes_with_column_sums_on_the_device's kind: fp32 sums
        ref = x.astype(np.float64).sum(axis=(0, 1))
        got = r["colsum"].view(np.float32).ravel().astype(np.float64)
        assert float(np.abs(got - ref).max()) < 1e-5 * max(1.0, float(np.abs(ref).max())) + 1e-3


def run_nchw_to_planes(lib, mem, form, guarded, zero, shape, layout):
    B, C, H, W = shape
    P, npl = H * W, 2 if layout == HL else 3
    x = np.random.default_rng(C + H).standard_normal((B, C, P), dtype=np.float32) * np.float32(3.0)
    ar = Arena(mem, form, guarded)
    # NCHW source: batch stride C H W, in the padded form 4 elements more (NaN)
    sbs = C * P + (4 if form == "padded" else 0)
    img = np.full(B * sbs, NAN["f32"], np.uint32)
    img.reshape(B, sbs)[:, :C * P] = f32_bits(x).reshape(B, C * P)
    if form != "padded":
        img = img[:(B - 1) * sbs + C * P]
    src = View(ar.raw("src", "f32", img.size, img), 0, 1, 1, img.size, img.size, img.size)
    dst = ar.view("dst", "bf16", B, P, npl * C, None, 8, form="padded" if form == "packed" else None)
    lib.check(lib.ccnet_cca_nchw_to_planes_f32(src.ptr, dst.ptr, B, C, H, W, sbs, dst.bs, dst.ps, layout, mem.stream), "nchw_to_planes")
    ar.settle("nchw_to_planes", (dst,))
    return {"dst": ar.get(dst)}


def check_nchw_to_planes(lib, r, shape, layout):
    B, C, H, W = shape
    x = np.random.default_rng(C + H).standard_normal((B, C, H * W), dtype=np.float32) * np.float32(3.0)
    assert np.array_equal(r["dst"], _planes_of(np.ascontiguousarray(x.transpose(0, 2, 1)), layout))


def run_pack_projection(lib, mem, form, guarded, zero, C, split):
    """no views here: every operand dense between bands, in every form"""
    cq, n = C // 8, 2 * (C // 8) + C
    rng = np.random.default_rng(C)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)                     # noqa: E731
    ins = dict(wq=f(cq, C), bq=f(cq), wk=f(cq, C), bk=f(cq), wv=f(C, C), bv=f(C))
    ar = Arena(mem, form, guarded)
    t = {k: ar.flat(k, "f32", a.size, f32_bits(a)) for k, a in ins.items()}
    w, b = ar.flat("w", "f32", n * C), ar.flat("b", "f32", n)
    w3 = ar.flat("w3", "bf16", n * 3 * C) if split else None
    w3t = ar.flat("w3t", "bf16", C * 3 * n) if split else None
    lib.check(lib.ccnet_cca_pack_projection_f32(t["wq"].ptr, t["bq"].ptr, t["wk"].ptr, t["bk"].ptr, t["wv"].ptr, t["bv"].ptr, w.ptr, b.ptr,
                                                w3.ptr if split else None, w3t.ptr if split else None, C, cq, mem.stream), "pack_projection")
    outs = (w, b) + ((w3, w3t) if split else ())
    ar.settle("pack_projection", outs)
    return {v.buf.name: ar.get(v) for v in outs}


def check_pack_projection(lib, r, C, split):
    cq, n = C // 8, 2 * (C // 8) + C
    rng = np.random.default_rng(C)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)                     # noqa: E731
    wq, bq, wk, bk, wv, bv = f(cq, C), f(cq), f(cq, C), f(cq), f(C, C), f(C)
    w = np.concatenate([wq, wk, wv])
    assert np.array_equal(r["w"].ravel(), f32_bits(w).ravel()) and np.array_equal(r["b"].ravel(), f32_bits(np.concatenate([bq, bk, bv])))
    if split:
        wh = bf16_bits(w)
        wl = bf16_bits(w - bf16_vals(wh))
        assert np.array_equal(r["w3"].reshape(n, 3 * C), np.concatenate([wh, wl, wh], axis=1))
        assert np.array_equal(r["w3t"].reshape(C, 3 * n), np.concatenate([wh.T, wh.T, wl.T], axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# projection GEMMs.  Operands are (rows, cols) matrices with a row stride: View(B = 1, P = rows, C = cols)
# ---------------------------------------------------------------------------------------------------------------------
def _matrix(ar, name, kind, rows, cols, data, al, batches=1):
    """(a width that is no multiple of the alignment unit -- an odd N -- keeps the smallest stride the entry points accept in the
    dense form, up(cols, al): the elements between cols and the stride are gap, NaN before and after)"""
    if ar.form == "packed":                       # a column slice at an offset of wider rows
        return ar.view(name, kind, batches, rows, cols, data, al, lead=al, wide=up(cols, al) + 2 * al)
    return ar.view(name, kind, batches, rows, cols, data, al, ps=up(cols, al) if ar.form == "dense" else None)


def _gemm_inputs(seed, *shapes):
    rng = np.random.default_rng(seed)
    return [bf16_bits(rng.standard_normal(s, dtype=np.float32)) for s in shapes]


def _projection_calls(lib, mem, form, guarded, M, N, K, a_, w_, biases):
    """ccnet_cca_projection_bf16 on one pair of operands, once per entry of ``biases`` {output name: fp32 values or None}"""
    ar = Arena(mem, form, guarded)
    a, w = _matrix(ar, "a", "bf16", M, K, a_, 8), _matrix(ar, "wt", "bf16", N, K, w_, 8)
    got = {}
    for name, bias_ in biases.items():
        bias = None if bias_ is None else ar.flat("bias_" + name, "f32", N, f32_bits(bias_))
        out = _matrix(ar, name, "f32", M, N, None, 4)
        lib.check(lib.ccnet_cca_projection_bf16(a.ptr, w.ptr, None if bias is None else bias.ptr, out.ptr, M, N, K, a.ps, w.ps, out.ps,
                                                mem.stream), "projection_bf16")
        ar.settle(f"projection_bf16({name})", (out,))
        got[name] = ar.get(out)
    return got


def run_projection(lib, mem, form, guarded, zero, mnk):
    M, N, K = mnk
    a_, w_ = _gemm_inputs(M + N + K, (1, M, K), (1, N, K))
    bias_ = np.random.default_rng(K).standard_normal(N, dtype=np.float32)
    return _projection_calls(lib, mem, form, guarded, M, N, K, a_, w_, {"out": bias_, "out_nobias": None})


def run_projection_placement(lib, mem, form, guarded, zero, mnk):
    """Wt = the first N rows of the K x K identity, no bias: out is A[:, :N] widened to fp32, bit for bit, in every form (every
    product but one per output is an exact zero).  The columns from the last 32 k of the range come from the last half k step."""
    M, N, K = mnk
    assert N <= K
    a_, = _gemm_inputs(7 * M + N + K, (1, M, K))
    r = _projection_calls(lib, mem, form, guarded, M, N, K, a_, bf16_bits(np.eye(K, dtype=np.float32)[None, :N]), {"out": None})
    want = f32_bits(bf16_vals(a_[:, :, :N]))
    assert np.array_equal(r["out"], want), ("placement", mnk, form, np.argwhere(r["out"] != want)[:4].tolist())
    return r


def run_projection_epilogue(lib, mem, form, guarded, zero, mnk):
    """A = 0: out is the fp32 bias, bit for bit, in every form"""
    M, N, K = mnk
    w_, = _gemm_inputs(11 * M + 3 * N + K, (1, N, K))
    bias_ = np.random.default_rng(K + 1).standard_normal(N, dtype=np.float32)
    r = _projection_calls(lib, mem, form, guarded, M, N, K, np.zeros((1, M, K), np.uint16), w_, {"out": bias_})
    want = np.broadcast_to(f32_bits(bias_), (1, M, N))
    assert np.array_equal(r["out"], want), ("epilogue", mnk, form, np.argwhere(r["out"] != want)[:4].tolist())
    return r


def check_in_run(lib, r, *args):
    """the bit-exact forms hold their expectation inside the runner, in every view form and on plain buffers"""


def _within(got, ref, mag):
    """fp32 accumulation in MFMA order: 2e-6 of sum |a||b| per output (tests/test_gpu_parity.py, the projection GEMM tests)"""
    assert bool((np.abs(got.astype(np.float64) - ref) <= 2e-6 * mag + 1e-30).all())


def check_projection(lib, r, mnk):
    M, N, K = mnk
    a_, w_ = _gemm_inputs(M + N + K, (1, M, K), (1, N, K))
    bias = np.random.default_rng(K).standard_normal(N, dtype=np.float32).astype(np.float64)
    a, w = bf16_vals(a_[0]).astype(np.float64), bf16_vals(w_[0]).astype(np.float64)
    mag = np.abs(a) @ np.abs(w).T
    _within(r["out"].view(np.float32)[0], a @ w.T + bias, mag + np.abs(bias))
    _within(r["out_nobias"].view(np.float32)[0], a @ w.T, mag)


def run_adjoint(lib, mem, form, guarded, zero, bcpk):
    B, C, P, K = bcpk
    w_, d_ = _gemm_inputs(B + C + P + K, (1, C, K), (B, P, K))
    add_ = np.random.default_rng(P).standard_normal((B, C, P), dtype=np.float32)
    ar = Arena(mem, form, guarded)
    w, d = _matrix(ar, "w", "bf16", C, K, w_, 8), _matrix(ar, "d", "bf16", P, K, d_, 8, batches=B)
    add = ar.flat("add", "f32", B * C * P, f32_bits(add_))
    dx, dx0 = ar.flat("dx", "f32", B * C * P), ar.flat("dx_noadd", "f32", B * C * P)
    lib.check(lib.ccnet_cca_projection_adjoint_bf16(w.ptr, d.ptr, add.ptr, dx.ptr, B, C, P, K, w.ps, d.ps, d.bs, mem.stream), "adjoint")
    ar.settle("projection_adjoint_bf16", (dx,))
    lib.check(lib.ccnet_cca_projection_adjoint_bf16(w.ptr, d.ptr, None, dx0.ptr, B, C, P, K, w.ps, d.ps, d.bs, mem.stream), "adjoint")
    ar.settle("projection_adjoint_bf16(no addend)", (dx0,))
    return {"dx": ar.get(dx), "dx_noadd": ar.get(dx0)}


def run_adjoint_zero(lib, mem, form, guarded, zero, bcpk):
    """d = 0: dx is the addend, bit for bit, in every form"""
    B, C, P, K = bcpk
    w_, = _gemm_inputs(B + C + P + K, (1, C, K))
    add_ = np.random.default_rng(P + 1).standard_normal((B, C, P), dtype=np.float32)
    ar = Arena(mem, form, guarded)
    w, d = _matrix(ar, "w", "bf16", C, K, w_, 8), _matrix(ar, "d", "bf16", P, K, np.zeros((B, P, K), np.uint16), 8, batches=B)
    add, dx = ar.flat("add", "f32", B * C * P, f32_bits(add_)), ar.flat("dx", "f32", B * C * P)
    lib.check(lib.ccnet_cca_projection_adjoint_bf16(w.ptr, d.ptr, add.ptr, dx.ptr, B, C, P, K, w.ps, d.ps, d.bs, mem.stream), "adjoint")
    ar.settle("projection_adjoint_bf16(d = 0)", (dx,))
    r = {"dx": ar.get(dx)}
    want = f32_bits(add_).reshape(r["dx"].shape)
    assert np.array_equal(r["dx"], want), ("adjoint, d = 0", bcpk, form, np.argwhere(r["dx"] != want)[:4].tolist())
    return r


def check_adjoint(lib, r, bcpk):
    B, C, P, K = bcpk
    w_, d_ = _gemm_inputs(B + C + P + K, (1, C, K), (B, P, K))
    add = np.random.default_rng(P).standard_normal((B, C, P), dtype=np.float32).astype(np.float64)
    w, d = bf16_vals(w_[0]).astype(np.float64), bf16_vals(d_).astype(np.float64)
    ref, mag = np.einsum("ck,bpk->bcp", w, d), np.einsum("ck,bpk->bcp", np.abs(w), np.abs(d))
    _within(r["dx"].view(np.float32).reshape(B, C, P), ref + add, mag + np.abs(add))
    _within(r["dx_noadd"].view(np.float32).reshape(B, C, P), ref, mag)


def run_wgrad(lib, mem, form, guarded, zero, rncs):
    R, N, C, S = rncs
    d_, x_ = _gemm_inputs(R + N + C, (1, R, N), (1, R, C))
    ar = Arena(mem, form, guarded)
    d, x = _matrix(ar, "d", "bf16", R, N, d_, 8), _matrix(ar, "x", "bf16", R, C, x_, 8)
    part = ar.flat("part", "f32", S * N * C)
    lib.check(lib.ccnet_cca_projection_wgrad_bf16(d.ptr, x.ptr, part.ptr, R, N, C, d.ps, x.ps, S, mem.stream), "wgrad")
    ar.settle("projection_wgrad_bf16", (part,))
    return {"part": ar.get(part)}


def check_wgrad(lib, r, rncs):
    R, N, C, S = rncs
    d_, x_ = _gemm_inputs(R + N + C, (1, R, N), (1, R, C))
    d, x = bf16_vals(d_[0]).astype(np.float64), bf16_vals(x_[0]).astype(np.float64)
    slab = (R + S * 64 - 1) // (S * 64) * 64                      # rows per slab as the entry point cuts them: a multiple of the k step
    for sl in range(S):
        if sl * slab >= R:                                        # a slab without rows: "every element written" means zeros
            assert not r["part"].reshape(S, N, C)[sl].any(), ("wgrad: a slab without rows is not all +0", rncs, sl)
    got = r["part"].view(np.float32).reshape(S, N, C).astype(np.float64).sum(0)
    assert bool((np.abs(got - d.T @ x) <= 2e-6 * (np.abs(d).T @ np.abs(x)) + 1e-30).all())


# ---------------------------------------------------------------------------------------------------------------------
# the table: id -> (runner, oracle check, arguments, options to set for the run, GPU only)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(cid, run, check, args, options=None, gpu_only=False):
    assert cid not in CASES
    CASES[cid] = (run, check, args, options or {}, gpu_only)


def _sid(shape, cq=None):
    return "x".join(map(str, shape)) + (f"-cq{cq}" if cq is not None and cq != shape[1] // 8 else "")


# bf16 pixel-major: a small map; 100-padded strips; 132-padded strips; a whole round of strips + a remainder cut into channel
# ranges (gmap_plan); a partial 64-channel group; one-pixel-wide and one-pixel-high maps.  Both values of "bf16_partial".
PM_BF16 = [((2, 64, 5, 6), 8), ((1, 64, 3, 97), 8), ((1, 64, 2, 99), 8), ((1, 64, 2, 101), 8), ((1, 64, 101, 2), 8),
           ((1, 64, 132, 3), 8), ((2, 128, 3, 130), 16), ((1, 72, 9, 7), 8), ((1, 64, 9, 1), 8), ((1, 64, 1, 9), 8)]
for _shape, _cq in PM_BF16:
    for _part in (1, 0):
        _case(f"pm_bf16-{_sid(_shape, _cq)}-partial{_part}", run_pm, check_pm, ("bf16", _shape, _cq), {"bf16_partial": _part})
PM_F32 = [((2, 64, 5, 6), 8), ((1, 32, 2, 99), 4), ((1, 64, 100, 3), 8), ((1, 64, 1, 9), 8), ((1, 68, 7, 9), 4)]
for _shape, _cq in PM_F32:
    _case(f"pm_f32-{_sid(_shape, _cq)}", run_pm, check_pm, ("f32", _shape, _cq))

# split planes, plane-free form (v fp32 pixel-major); with the three-plane backward where the issue lists the shape for it
for _shape, _cq, _p3 in [((2, 64, 5, 6), 8, True), ((1, 96, 17, 20), 12, True), ((1, 64, 3, 97), 8, True), ((1, 64, 100, 3), 8, True),
                         ((1, 72, 9, 7), 12, False)]:
    _case(f"planes_free{'_p3' if _p3 else ''}-{_sid(_shape, _cq)}", run_planes, check_planes, (_shape, _cq, "free", _p3))
# planes form: 132-padded strips with and without v_bias; long rows (two blocks; three, the last of one position; four), long
# columns, both long
for _shape in [(1, 64, 3, 129), (1, 64, 132, 2)]:
    for _mode in ("bias", "nobias"):
        _case(f"planes_{_mode}-{_sid(_shape)}", run_planes, check_planes, (_shape, 8, _mode))
for _shape, _cq in [((1, 64, 3, 133), 8), ((1, 64, 2, 265), 8), ((1, 32, 133, 5), 4), ((1, 32, 265, 2), 4)]:
    _case(f"planes_long-{_sid(_shape)}", run_planes, check_planes, (_shape, _cq, "nobias"))
# on the device only: four blocks per row (38 s in the emulator, a fifth of this table's time there); both sides long
_case("planes_long-1x64x2x528", run_planes, check_planes, ((1, 64, 2, 528), 8, "nobias"), gpu_only=True)
_case("planes_long-1x32x134x133", run_planes, check_planes, ((1, 32, 134, 133), 4, "nobias"), gpu_only=True)

SPLIT_SHAPES = [(2, 80, 5, 6), (3, 8, 9, 1), (1, 640, 17, 20)]
for _shape in SPLIT_SHAPES:
    for _layout, _ln in ((HL, "hl"), (HLH, "hlh"), (HHL, "hhl")):
        for _bias in (True, False):
            _case(f"split-{_sid(_shape)}-{_ln}-{'bias' if _bias else 'nobias'}", run_split, check_split, (_shape, _layout, _bias, False))
for _shape in SPLIT_SHAPES + [(8, 72, 13, 11)]:          # (the last: a grid extent that is no plain multiple, split_colsum_gx)
    for _layout, _ln in ((HL, "hl"), (HLH, "hlh"), (HHL, "hhl")):
        _case(f"split_colsum-{_sid(_shape)}-{_ln}", run_split, check_split, (_shape, _layout, False, True))
for _shape in [(2, 8, 3, 5), (1, 200, 7, 9)]:
    for _layout, _ln in ((HL, "hl"), (HLH, "hlh"), (HHL, "hhl")):
        _case(f"nchw_to_planes-{_sid(_shape)}-{_ln}", run_nchw_to_planes, check_nchw_to_planes, (_shape, _layout))
for _C in (16, 64, 200):
    for _split in (True, False):
        _case(f"pack_projection-C{_C}-{'w3' if _split else 'no_w3'}", run_pack_projection, check_pack_projection, (_C, _split))
# The projection GEMMs (csrc/cca_gemm.hpp: tiles of 256 x 128, k steps of 64, three stages).  (M, N, K): the smallest problem
# (nk = 1, a scalar N tail); one row past a tile (nk = 1, no tails); nk = 2 with a K tail and an odd N; nk = 4 -- the first nk
# at which a stage it + 3 is filled -- with a K tail; nk = 9.  The loop's only, first and last k steps all run.
for _mnk in [(37, 24, 72), (300, 136, 192), (1, 5, 8), (257, 128, 64), (255, 133, 72), (129, 72, 200), (513, 72, 520)]:
    _case(f"projection-{_sid(_mnk)}", run_projection, check_projection, (_mnk,))
for _mnk in [(1, 8, 8), (257, 61, 64), (300, 136, 136), (130, 197, 200)]:
    _case(f"projection_placement-{_sid(_mnk)}", run_projection_placement, check_in_run, (_mnk,))
for _mnk in [(1, 5, 8), (300, 133, 72)]:
    _case(f"projection_epilogue-{_sid(_mnk)}", run_projection_epilogue, check_in_run, (_mnk,))
# (B, C, P, K): the second is one past a tile on either axis under either operand assignment, nk = 4 with a K tail
for _bcpk in [(2, 40, 35, 72), (1, 72, 257, 64), (3, 264, 131, 200)]:
    _case(f"adjoint-{_sid(_bcpk)}", run_adjoint, check_adjoint, (_bcpk,))
_case("adjoint_zero-3x264x131x200", run_adjoint_zero, check_in_run, ((3, 264, 131, 200),))
# (R, N, C, S): the smallest; one k step of one full tile; uneven slabs with N and C past a tile; slabs shorter than a k step;
# more slabs than rows (slabs without rows write zeros)
for _rncs in [(700, 24, 40, 5), (1, 8, 8, 1), (64, 128, 256, 1), (130, 136, 264, 3), (40, 8, 8, 5), (3, 8, 8, 5)]:
    _case(f"wgrad-{_sid(_rncs)}", run_wgrad, check_wgrad, (_rncs,))

_PLAIN = {}            # (back end, case id) -> the results on dense, unguarded buffers, computed once and left unchanged


def ids(emulator):
    return [(cid, form) for cid, case in CASES.items() if not (emulator and case[4]) for form in FORMS]


class _options:
    """the case's library options set for the length of a ``with`` block, and restored"""

    def __init__(self, lib, options):
        self.lib, self.options = lib, options

    def __enter__(self):
        self.previous = {name: self.lib.set_option(name, value) for name, value in self.options.items()}

    def __exit__(self, *exc):
        for name, value in self.previous.items():
            self.lib.set_option(name, value)
        assert all(self.lib.get_option(name) == value for name, value in self.previous.items())


def plain_case(lib, mem, cid, case=None):
    """(``case``: a table entry that is not in CASES, under an id of its own)  the case on dense, unguarded buffers: computed once per back end -- by whichever test asks first, so a test that runs the
    emulator in another mode (tests/test_emu_modes.py) asks BEFORE it sets the mode -- and left unchanged"""
    run, check, args, options, _ = case or CASES[cid]
    if (mem.name, cid) not in _PLAIN:
        with _options(lib, options):
            _PLAIN[mem.name, cid] = run(lib, mem, "dense", False, False, *args)
    return _PLAIN[mem.name, cid]


def run_case_bits(lib, mem, cid, form, case=None):
    """one guarded run of the case in ``form``, held bitwise to ``plain_case``"""
    run, check, args, options, _ = case or CASES[cid]
    plain = plain_case(lib, mem, cid, case)
    with _options(lib, options):
        got = run(lib, mem, form, True, False, *args)
    for name, ref in plain.items():
        assert np.array_equal(got[name], ref), (cid, form, name, "differs from the dense, unguarded call", int((got[name] != ref).sum()))
    return got


def run_case(lib, mem, cid, form):
    run, check, args, options, _ = CASES[cid]
    plain = plain_case(lib, mem, cid)
    with _options(lib, options):
        got = run(lib, mem, form, True, False, *args)
        for name, ref in plain.items():
            assert np.array_equal(got[name], ref), (name, "differs from the dense, unguarded call", int((got[name] != ref).sum()))
        again = run(lib, mem, form, True, True, *args)
        for name, ref in got.items():
            assert np.array_equal(again[name], ref), (name, "depends on what the workspace / scratch held")
        if form == "padded":
            check(lib, got, *args)
