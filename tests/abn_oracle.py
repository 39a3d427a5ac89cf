"""float64 numpy oracle of include/ccnet_abn.h: batch statistics, the activated affine step and its gradients, in both
gamma conventions (weight as is, and |weight| + eps for in-place mode).  Test infrastructure only."""
import numpy as np

IDENTITY, RELU, LEAKY_RELU, ELU = 0, 1, 2, 3


def act_forward(z, act, p):
    if act == RELU:
        return np.where(z > 0, z, 0.0)
    if act == LEAKY_RELU:
        return np.where(z > 0, z, z * p)
    if act == ELU:
        return np.where(z > 0, z, p * np.expm1(np.minimum(z, 0.0)))
    return z


def act_grad(z, act, p):
    """d act / dz at the pre-activation z (exact, not rebuilt from y)"""
    if act == RELU:
        return (z > 0).astype(np.float64)
    if act == LEAKY_RELU:
        return np.where(z > 0, 1.0, p)
    if act == ELU:
        return np.where(z > 0, 1.0, p * np.exp(np.minimum(z, 0.0)))
    return np.ones_like(z)


def gamma_of(weight, C, gamma_mode, eps):
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    return np.abs(w) + eps if gamma_mode == 1 else w


def _bc(v):
    return np.asarray(v, np.float64)[None, :, None]


def forward(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, act=IDENTITY, p=0.01,
            gamma_mode=0, residual=None):
    """x (N, C, ...) -> dict(y, z, xhat, mean, invstd, n, running_mean, running_var), all float64."""
    x = np.asarray(x, np.float64)
    N, C = x.shape[:2]
    x3 = x.reshape(N, C, -1)
    n = x3.shape[0] * x3.shape[2]
    rm = np.asarray(running_mean, np.float64).copy()
    rv = np.asarray(running_var, np.float64).copy()
    if training:
        mean = x3.mean(axis=(0, 2))
        var = ((x3 - _bc(mean)) ** 2).mean(axis=(0, 2))
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var = rm.copy(), rv.copy()
    invstd = 1.0 / np.sqrt(var + eps)
    g = gamma_of(weight, C, gamma_mode, eps)
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64)
    xhat = (x3 - _bc(mean)) * _bc(invstd)
    z = xhat * _bc(g) + _bc(b)
    if residual is not None:
        z = z + np.asarray(residual, np.float64).reshape(N, C, -1)
    y = act_forward(z, act, p)
    return {"y": y.reshape(x.shape), "z": z, "xhat": xhat, "mean": mean, "var": var, "invstd": invstd, "n": n,
            "running_mean": rm, "running_var": rv}


def backward(f, dy, weight, training, eps=1e-5, act=IDENTITY, p=0.01, gamma_mode=0):
    """gradients from forward()'s dict f: dict(dx, dweight, dbias, dresidual)."""
    dy = np.asarray(dy, np.float64)
    shape = dy.shape
    N, C = shape[:2]
    dz = dy.reshape(N, C, -1) * act_grad(f["z"], act, p)
    g = gamma_of(weight, C, gamma_mode, eps)
    sdz = dz.sum(axis=(0, 2))
    sdzx = (dz * f["xhat"]).sum(axis=(0, 2))
    k = _bc(g * f["invstd"])
    if training:
        n = f["n"]
        dx = k * (dz - _bc(sdz / n) - f["xhat"] * _bc(sdzx / n))
    else:
        dx = k * dz
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    dweight = sdzx * (np.sign(w) if gamma_mode == 1 else 1.0)
    return {"dx": dx.reshape(shape), "dweight": dweight, "dbias": sdz, "dresidual": dz.reshape(shape),
            "sum_dz": sdz, "sum_dzx": sdzx}


def act_inverse(y, act, p):
    """z from y as include/ccnet_abn.h specifies it: leaky y / p, elu log1p(max(y / p, -1 + 2^-24)), y itself above 0"""
    if act == LEAKY_RELU:
        return np.where(y > 0, y, y / p)
    if act == ELU:
        return np.where(y > 0, y, np.log1p(np.maximum(np.minimum(y, 0.0) / p, -1.0 + 2.0 ** -24)))
    return y


def act_grad_from_output(y, act, p):
    """d act / dz taken from the output y (y > 0: 1; else relu 0, leaky p, elu y + p)"""
    if act == RELU:
        return (y > 0).astype(np.float64)
    if act == LEAKY_RELU:
        return np.where(y > 0, 1.0, p)
    if act == ELU:
        return np.where(y > 0, 1.0, y + p)
    return np.ones_like(y)


def backward_from_output(y, dy, residual, weight, bias, mean, invstd, n, training, act=IDENTITY, p=0.01, eps=1e-5):
    """CCNET_ABN_FROM_OUTPUT in float64: the gradients rebuilt from a stored (and so rounded) output ``y`` -- the y the code
    under test produced -- with gamma = |weight| + eps: z = act^-1(y), xhat = (z - beta - residual) / gamma, act' from y.
    ``mean`` is unused by the arithmetic (xhat comes from y) and is taken for symmetry with backward(); dict(dx, dweight,
    dbias, dresidual, sum_dz, sum_dzx)."""
    y = np.asarray(y, np.float64)
    shape = y.shape
    N, C = shape[:2]
    y3 = y.reshape(N, C, -1)
    g = gamma_of(weight, C, 1, eps)
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64)
    z = act_inverse(y3, act, p)
    r = 0.0 if residual is None else np.asarray(residual, np.float64).reshape(N, C, -1)
    xhat = (z - _bc(b) - r) / _bc(g)
    dz = np.asarray(dy, np.float64).reshape(N, C, -1) * act_grad_from_output(y3, act, p)
    sdz = dz.sum(axis=(0, 2))
    sdzx = (dz * xhat).sum(axis=(0, 2))
    k = _bc(g * np.asarray(invstd, np.float64))
    dx = k * (dz - _bc(sdz / n) - xhat * _bc(sdzx / n)) if training else k * dz
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    return {"dx": dx.reshape(shape), "dweight": sdzx * np.sign(w), "dbias": sdz, "dresidual": dz.reshape(shape),
            "sum_dz": sdz, "sum_dzx": sdzx, "z": z, "xhat": xhat}


def to_bf16_bits(a):
    """float -> bf16 bit pattern (uint16), round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)
