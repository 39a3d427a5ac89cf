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


def to_bf16_bits(a):
    """float -> bf16 bit pattern (uint16), round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)
