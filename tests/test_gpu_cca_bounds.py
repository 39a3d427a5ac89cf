"""GPU checks of the memory behaviour of the pixel-major and split-plane families of the attention core: the case table of
tests/cca_cases.py -- the one tests/test_cca_bounds_host.py runs in the SIMT emulator -- through the gfx950 library on device
buffers with guard bands, in the dense, packed, padded and tight view forms with an exact-size workspace; then what only the
Python host layer (ccnet_amd.functions) can show: non-contiguous but qualifying views taken without a copy, views that do not
qualify copied, the producers on sliced sources."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cca_cases as K  # noqa: E402
from guarded_memory import DeviceMemory  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _lib
    return _lib.get_lib()


@pytest.fixture(scope="module")
def mem(lib):
    return DeviceMemory()


# ---------------------------------------------------------------------------------------------------------------------
# the shared table over the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", K.ids(emulator=False), ids=lambda v: v)
def test_views_bands_and_workspace(lib, mem, cid, form):
    K.run_case(lib, mem, cid, form)


# ---------------------------------------------------------------------------------------------------------------------
# through ccnet_amd.functions
# ---------------------------------------------------------------------------------------------------------------------
SHAPE = (2, 64, 5, 6)
CQ = 8
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])


def bits(t):
    """the bit patterns of a tensor as integers (NaN compares equal to itself)"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def sliced(values, ps, bs, offset=0):
    """``values`` (B, H, W, c) laid into a NaN-filled flat tensor at pixel stride ``ps`` and batch stride ``bs``, starting
    ``offset`` elements in; the buffer ends at the last in-view element.  Returns (the view, the flat tensor)."""
    B, H, W, c = values.shape
    n = offset + (B - 1) * bs + (H * W - 1) * ps + c
    flat = torch.full((n,), NAN, device=values.device, dtype=values.dtype)
    view = flat.as_strided((B, H, W, c), (bs, W * ps, ps, 1), offset)
    view.copy_(values)
    return view, flat


def pm_tensors(dtype, seed=3):
    B, C, H, W = SHAPE
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda c: torch.randn((B, H, W, c), generator=g).to(DEV, dtype)                  # noqa: E731
    return r(2 * CQ + C), r(C), r(C), torch.tensor([0.5], device=DEV)


def pm_call(qkv, x, dy, gamma):
    from ccnet_amd.functions import CrissCrossPMFunction
    qkv, gamma = qkv.detach().requires_grad_(True), gamma.clone().requires_grad_(True)
    y = CrissCrossPMFunction.apply(qkv, x, gamma, CQ)
    y.backward(dy)
    torch.cuda.synchronize()
    assert qkv.grad.is_contiguous()
    return bits(y.detach()), bits(qkv.grad), bits(gamma.grad)


@DTYPES
@pytest.mark.parametrize("form", ["padded", "tight"])
def test_pm_function_takes_strided_views_without_copying(lib, dtype, form):
    """qkv, x and grad_output as non-contiguous views that qualify (a padded pixel stride; a padded batch stride, or the
    smallest one with the buffer ending at the last element): _pm_view hands the kernels the view itself, y / dqkv / dgamma
    are bitwise those of the contiguous call and the NaN around the views stays what it was."""
    from ccnet_amd import functions as F
    B, C, H, W = SHAPE
    al = 8 if dtype == torch.bfloat16 else 4
    qkv, x, dy, gamma = pm_tensors(dtype)
    want = pm_call(qkv, x, dy, gamma)
    views, flats = [], []
    for t in (qkv, x, dy):
        ps = t.shape[3] + al
        bs = H * W * ps + al if form == "padded" else (H * W - 1) * ps + t.shape[3]
        v, flat = sliced(t, ps, bs)
        assert not v.is_contiguous()
        kept, kbs, kps = F._pm_view("view", v)
        assert kept.data_ptr() == v.data_ptr() and (kbs, kps) == (bs, ps)
        views.append(v)
        flats.append(flat)
    before = [bits(f).clone() for f in flats]
    got = pm_call(*views, gamma)
    for a, b, name in zip(got, want, ("y", "dqkv", "dgamma")):
        assert torch.equal(a, b), name
    for f, b in zip(flats, before):
        assert torch.equal(bits(f), b)


@DTYPES
@pytest.mark.parametrize("how", ["pointer", "pixel_stride", "batch_stride"])
def test_pm_function_copies_views_that_do_not_qualify(lib, dtype, how):
    """a view whose data pointer is not 16-byte aligned, or whose pixel / batch stride misses the alignment unit, is copied by
    _pm_view; the results are bitwise those of the contiguous call"""
    from ccnet_amd import functions as F
    B, C, H, W = SHAPE
    al = 8 if dtype == torch.bfloat16 else 4
    qkv, x, dy, gamma = pm_tensors(dtype, seed=5)
    want = pm_call(qkv, x, dy, gamma)
    views = []
    for t in (qkv, x, dy):
        c = t.shape[3]
        ps = c + (1 if how == "pixel_stride" else al)
        bs = H * W * ps + (1 if how == "batch_stride" else al)
        v, _ = sliced(t, ps, bs, offset=1 if how == "pointer" else 0)
        if how == "pointer":
            assert v.data_ptr() % 16 != 0
        kept, kbs, kps = F._pm_view("view", v)
        assert kept.data_ptr() != v.data_ptr() and kept.is_contiguous() and (kbs, kps) == (H * W * c, c)
        views.append(v)
    got = pm_call(*views, gamma)
    for a, b, name in zip(got, want, ("y", "dqkv", "dgamma")):
        assert torch.equal(a, b), name


def test_plane_producers_take_sliced_sources(lib):
    """split_planes / split_planes_colsum on a channel slice of wider rows with a padded batch stride, nchw_to_planes on a
    channel slice of a wider NCHW tensor (a batch stride beyond C H W): bitwise what the contiguous copy of the same values
    gives, the NaN around the slices untouched"""
    from ccnet_amd import functions as F
    B, C, H, W = 2, 80, 5, 6
    g = torch.Generator(device="cpu").manual_seed(7)
    t = (torch.randn((B, H, W, C), generator=g) * 3.0).to(DEV)
    ps = C + 16
    v, flat = sliced(t, ps, H * W * ps + 4, offset=8)
    before = bits(flat).clone()
    bias = torch.randn((64,), generator=g).to(DEV)
    for layout in (F.PLANES_HL, F.PLANES_HLH, F.PLANES_HHL):
        for b in (None, bias):
            assert torch.equal(F.split_planes(v, 16, 64, layout, bias=b), F.split_planes(t, 16, 64, layout, bias=b))
        got, want = F.split_planes_colsum(v, layout), F.split_planes_colsum(t, layout)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    wide = torch.full((B, C + 5, H, W), NAN, device=DEV)
    x = wide[:, 3:3 + C]
    x.copy_(t.permute(0, 3, 1, 2))
    wide_before = bits(wide).clone()
    assert not x.is_contiguous()
    for layout in (F.PLANES_HL, F.PLANES_HLH, F.PLANES_HHL):
        assert torch.equal(F.nchw_to_planes(x, layout), F.nchw_to_planes(x.contiguous(), layout))
    torch.cuda.synchronize()
    assert torch.equal(bits(flat), before) and torch.equal(bits(wide), wide_before)
