"""GPU checks of the device ABN at its edges: the case table of tests/abn_cases.py -- the one tests/test_abn_host.py runs in
the SIMT emulator -- through the gfx950 library on device buffers with guard bands (element path, cut groups, reduction
slices that cut planes, uneven ranks, NaN isolation), held to the header's bar against the float64 oracles; then what only
the Python front end (ccnet_amd.abn) can show: input forms, needs_input_grad subsets, an offset view in place, a side
stream."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import abn_cases as K  # noqa: E402
import abn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ccnet_amd import _abn_lib
    return _abn_lib.get_lib()


@pytest.fixture(scope="module")
def mem(lib):
    return K.DeviceMemory()


# ---------------------------------------------------------------------------------------------------------------------
# the shared table over the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape,sem", K.GRID_CASES, ids=lambda v: v)
def test_edge_shapes(lib, mem, shape, sem, bf16):
    K.run_grid_case(lib, mem, shape, sem, bf16)


@DTYPES
@pytest.mark.parametrize("par,shape,sem", K.PARAMETER_CASES, ids=lambda v: v)
def test_parameter_forms(lib, mem, par, shape, sem, bf16):
    K.run_parameter_case(lib, mem, par, shape, sem, bf16)


@pytest.mark.parametrize("name,shape,bf16", K.NUMERIC_CASES, ids=lambda v: {False: "f32", True: "bf16"}.get(v, v))
def test_numeric_edges(lib, mem, name, shape, bf16):
    K.run_numeric_case(lib, mem, name, shape, bf16)


@DTYPES
@pytest.mark.parametrize("sem,shape", K.MISALIGNED_CASES, ids=lambda v: v)
def test_misaligned_tensors_give_the_aligned_result_bitwise(lib, mem, sem, shape, bf16):
    K.run_misaligned_case(lib, mem, sem, shape, bf16)


@pytest.mark.parametrize("N,R,sem", K.RANK_CASES, ids=lambda v: str(v))
def test_uneven_ranks_match_one(lib, mem, N, R, sem):
    K.run_rank_case(lib, mem, N, R, sem)


@pytest.mark.parametrize("sem", ["oop_relu_res", "ip_leaky01_res"])
def test_non_finite_input_stays_in_its_channel_and_in_its_statistics(lib, mem, sem):
    K.run_nonfinite_case(lib, mem, sem)


# ---------------------------------------------------------------------------------------------------------------------
# through ccnet_amd.abn
# ---------------------------------------------------------------------------------------------------------------------
ACTS = {"identity": (O.IDENTITY, 0.0), "relu": (O.RELU, 0.0), "leaky_relu": (O.LEAKY_RELU, 0.01), "elu": (O.ELU, 1.0)}
SHAPE = (3, 5, 9, 11)


def _layer(cls, inputs, activation="leaky_relu", affine=True, training=True):
    """a device layer carrying the case's parameters and running statistics"""
    from ccnet_amd import abn
    _, w, b, rm, rv, _, _ = inputs
    m = getattr(abn, cls)(len(rm), activation=activation, activation_param=ACTS[activation][1] or 0.01, affine=affine)
    with torch.no_grad():
        if affine:
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
        m.running_mean.copy_(torch.from_numpy(rm))
        m.running_var.copy_(torch.from_numpy(rv))
    return m.to(DEV).train(training)


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(a).to(DEV).to(dtype)


def _run(m, x, dy, residual=None, activation=None, x_grad=True, res_grad=True):
    """one forward + backward of layer ``m`` on copies of the device tensors; numpy results under the driver's names"""
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    xa = xi if not m.inplace else xi * 1.0 if x_grad else xi.clone()       # an in-place layer cannot overwrite a leaf
    r = None if residual is None else residual.clone().requires_grad_(res_grad)
    y = m(xa, residual=r, activation=activation)
    assert y.dtype == x.dtype and y.shape == x.shape
    y.backward(dy)
    return {"y": _np(y), "dx": _np(xi.grad), "dresidual": None if r is None else _np(r.grad),
            "dweight": None if m.weight is None else _np(m.weight.grad),
            "dbias": None if m.bias is None else _np(m.bias.grad),
            "running_mean": _np(m.running_mean), "running_var": _np(m.running_var)}


def _check(r, inputs, m, activation, bf16=False, residual=True):
    x, w, b, rm, rv, dy, res = inputs
    act, p = ACTS[activation]
    if not m.affine:
        w = b = None
    K.check_case(r, x, w, b, rm, rv, dy, res if residual else None, training=m.training, act=act, p=p,
                 source=int(m.inplace), bf16=bf16, record=("gpu", "front end"))


@DTYPES
@pytest.mark.parametrize("cls", ["ABN", "InPlaceABN"])
def test_module_without_affine_parameters(lib, cls, bf16):
    inputs = K.table_inputs(SHAPE, 21)
    m = _layer(cls, inputs, affine=False)
    assert m.weight is None and m.bias is None
    dt = torch.bfloat16 if bf16 else torch.float32
    _check(_run(m, _dev(inputs[0], dt), _dev(inputs[5], dt)), inputs, m, "leaky_relu", bf16, residual=False)


@pytest.mark.parametrize("shape", [(6, 5), (2, 5, 3, 4, 5)], ids=["2d", "5d"])
@pytest.mark.parametrize("cls", ["ABN", "InPlaceABN"])
def test_module_takes_2d_and_5d_inputs(lib, cls, shape):
    inputs = K.table_inputs(shape, 22)
    m = _layer(cls, inputs, "elu")
    _check(_run(m, _dev(inputs[0]), _dev(inputs[5])), inputs, m, "elu", residual=False)


def test_module_takes_a_channels_last_input_out_of_place(lib):
    inputs = K.table_inputs(SHAPE, 23, residual=True)
    m = _layer("ABN", inputs, "relu")
    x = _dev(inputs[0]).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    res = _dev(inputs[6]).contiguous(memory_format=torch.channels_last)
    dy = _dev(inputs[5]).contiguous(memory_format=torch.channels_last)
    _check(_run(m, x, dy, res), inputs, m, "relu")


def test_module_in_place_refuses_a_non_contiguous_input(lib):
    inputs = K.table_inputs(SHAPE, 24)
    m = _layer("InPlaceABN", inputs)
    x = _dev(inputs[0])
    for bad in (x.contiguous(memory_format=torch.channels_last), x[:, :, :, ::2].expand(3, 5, 9, 6)):
        with pytest.raises(ValueError, match="contiguous"):
            m(bad)


@DTYPES
def test_module_in_place_on_a_view_one_element_into_a_larger_tensor(lib, bf16):
    """a contiguous view that starts 4 bytes (fp32) or 2 bytes (bf16) into its parent: the element path through the front
    end.  Bitwise the aligned run's result, and the parent's elements outside the view keep their values."""
    inputs = K.table_inputs(SHAPE, 25, residual=True)
    dt = torch.bfloat16 if bf16 else torch.float32
    x, dy, res = _dev(inputs[0], dt), _dev(inputs[5], dt), _dev(inputs[6], dt)
    m = _layer("InPlaceABN", inputs, "elu")
    aligned = _run(m, x, dy, res)
    _check(aligned, inputs, m, "elu", bf16)
    with torch.no_grad():                                   # the same running statistics for the second run
        m.running_mean.copy_(torch.from_numpy(inputs[3]))
        m.running_var.copy_(torch.from_numpy(inputs[4]))
    m.zero_grad(set_to_none=True)
    n = x.numel()
    leaf = torch.full((n + 16,), 7.0, device=DEV, dtype=dt)
    leaf[1:1 + n] = x.reshape(-1)
    leaf.requires_grad_(True)
    parent = leaf * 1.0
    view = parent[1:1 + n].view(SHAPE)
    assert view.is_contiguous() and view.data_ptr() % 16 == x.element_size() and parent.data_ptr() % 16 == 0
    r = res.clone().requires_grad_(True)
    y = m(view, residual=r)
    assert y.data_ptr() == view.data_ptr()
    y.backward(dy)
    got = {"y": _np(y), "dx": _np(leaf.grad[1:1 + n].view(SHAPE)), "dresidual": _np(r.grad), "dweight": _np(m.weight.grad),
           "dbias": _np(m.bias.grad), "running_mean": _np(m.running_mean), "running_var": _np(m.running_var)}
    for k, v in got.items():
        assert np.array_equal(v, aligned[k]), k
    outside = torch.cat([parent.detach()[:1], parent.detach()[1 + n:]])
    assert torch.equal(outside, torch.full_like(outside, 7.0))
    assert torch.equal(parent.detach()[1:1 + n].view(SHAPE), y.detach())


@pytest.mark.parametrize("activation", ["leaky_relu", "elu"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_module_in_place_bf16_matches_the_from_output_oracle(lib, activation, training):
    inputs = K.table_inputs(SHAPE, 26, residual=True)
    m = _layer("InPlaceABN", inputs, activation, training=training)
    x, dy, res = (_dev(inputs[i], torch.bfloat16) for i in (0, 5, 6))
    _check(_run(m, x, dy, res), inputs, m, activation, bf16=True)


@DTYPES
def test_module_relu_overridden_per_call_with_a_residual(lib, bf16):
    inputs = K.table_inputs(SHAPE, 27, residual=True)
    m = _layer("ABN", inputs, "identity")
    dt = torch.bfloat16 if bf16 else torch.float32
    r = _run(m, _dev(inputs[0], dt), _dev(inputs[5], dt), _dev(inputs[6], dt), activation="relu")
    _check(r, inputs, m, "relu", bf16)
    assert (r["y"] >= 0).all() and (r["y"] == 0).any()


@pytest.mark.parametrize("cls", ["ABN", "InPlaceABN"])
def test_module_needs_input_grad_subsets(lib, cls):
    inputs = K.table_inputs(SHAPE, 28, residual=True)
    x, dy, res = _dev(inputs[0]), _dev(inputs[5]), _dev(inputs[6])
    m = _layer(cls, inputs)
    r = _run(m, x, dy, res, x_grad=False, res_grad=False)                 # parameters only: dweight and dbias still right
    assert r["dx"] is None and r["dresidual"] is None and r["dweight"] is not None and r["dbias"] is not None
    _check(r, inputs, m, "leaky_relu")
    m = _layer(cls, inputs)
    m.weight.requires_grad_(False)                                        # a frozen weight gets no gradient
    r = _run(m, x, dy, res)
    assert r["dweight"] is None and m.weight.grad is None and r["dbias"] is not None
    _check(r, inputs, m, "leaky_relu")
    m = _layer(cls, inputs)
    r = _run(m, x, dy, res, res_grad=False)                               # a residual that needs no gradient
    assert r["dresidual"] is None and r["dx"] is not None
    _check(r, inputs, m, "leaky_relu")


@pytest.mark.parametrize("cls", ["ABN", "InPlaceABN"])
def test_module_eval_mode_leaves_the_running_statistics_untouched(lib, cls):
    inputs = K.table_inputs(SHAPE, 29)
    m = _layer(cls, inputs, training=False)
    r = _run(m, _dev(inputs[0]), _dev(inputs[5]))
    assert np.array_equal(r["running_mean"], inputs[3]) and np.array_equal(r["running_var"], inputs[4])
    _check(r, inputs, m, "leaky_relu", residual=False)


@pytest.mark.parametrize("cls", ["ABN", "InPlaceABN"])
def test_module_on_a_side_stream_matches_the_default_stream_bitwise_without_host_sync(lib, cls):
    inputs = K.table_inputs(SHAPE, 30, residual=True)
    x, dy, res = _dev(inputs[0]), _dev(inputs[5]), _dev(inputs[6])
    runs = []
    side = torch.cuda.Stream(device=DEV)
    for stream in (torch.cuda.current_stream(DEV), side):
        m = _layer(cls, inputs)
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        with torch.cuda.stream(stream):
            torch.cuda.set_sync_debug_mode("error")
            try:
                xi = x.clone().requires_grad_(True)
                r = res.clone().requires_grad_(True)
                y = m(xi * 1.0, residual=r)
                y.backward(dy)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        runs.append({"y": _np(y), "dx": _np(xi.grad), "dresidual": _np(r.grad), "dweight": _np(m.weight.grad),
                     "dbias": _np(m.bias.grad), "running_mean": _np(m.running_mean), "running_var": _np(m.running_var)})
    _check(runs[1], inputs, m, "leaky_relu")
    for k, v in runs[0].items():
        assert np.array_equal(v, runs[1][k]), k
