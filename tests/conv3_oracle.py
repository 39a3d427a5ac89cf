"""NumPy fp64 restatement of the 3x3, stride-1, dilated convolution (padding = dilation) on pixel-major (channels_last) tensors,
and of its two adjoints: pad by d, then nine shifted matrix products.  tests/test_conv3_host.py first checks it against
``torch.nn.functional.conv2d`` and autograd in fp64; the emulator and device tests are then held to it.  Test infrastructure only.

Layouts: x (B, H, W, Cin), y and dy (B, H, W, Cout), w (Cout, Cin, 3, 3) -- the parameter's own.  Tap t = 3 (ky + 1) + (kx + 1):
the source of output pixel (h, w) under tap t is (h + ky d, w + kx d), zero outside the image."""
import numpy as np

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def shifted(a, t, d):
    """(B, H, W, C): a[b, h + ky d, w + kx d, :] where that pixel exists, zero elsewhere"""
    B, H, W, C = a.shape
    ky, kx = TAPS[t]
    p = np.zeros((B, H + 2 * d, W + 2 * d, C), a.dtype)
    p[:, d:d + H, d:d + W] = a
    return p[:, d + ky * d:d + ky * d + H, d + kx * d:d + kx * d + W]


def pack_forward(w):
    """(Cout, 9 Cin): [n][t Cin + c] = w[n][c][t]"""
    n, c = w.shape[:2]
    return np.ascontiguousarray(w.reshape(n, c, 9).transpose(0, 2, 1)).reshape(n, 9 * c)


def pack_adjoint(w):
    """(Cin, 9 Cout): [c][t Cout + n] = w[n][c][8 - t] (taps mirrored, channels transposed)"""
    n, c = w.shape[:2]
    return np.ascontiguousarray(w.reshape(n, c, 9)[:, :, ::-1].transpose(1, 2, 0)).reshape(c, 9 * n)


def conv_rows(a, wt, d):
    """what ccnet_conv3_bf16 computes without bias and addend: sum_t shifted(a, t) @ wt[:, t K : (t + 1) K]^T -> (B, H, W, N)"""
    K = a.shape[3]
    return sum(shifted(a, t, d) @ wt[:, t * K:(t + 1) * K].T for t in range(9))


def forward(x, w, bias=None, d=1):
    y = conv_rows(x, pack_forward(w), d)
    return y if bias is None else y + bias


def input_grad(dy, w, d=1):
    return conv_rows(dy, pack_adjoint(w), d)


def weight_grad_taps(dy, x, d=1):
    """(9, Cout, Cin): [t][n][c] = sum_r dy[r][n] x[src(r, t)][c]"""
    n = dy.shape[3]
    D = dy.reshape(-1, n)
    return np.stack([D.T @ shifted(x, t, d).reshape(-1, x.shape[3]) for t in range(9)])


def weight_grad(dy, x, d=1):
    """(Cout, Cin, 3, 3)"""
    g = weight_grad_taps(dy, x, d)
    return np.ascontiguousarray(g.transpose(1, 2, 0)).reshape(g.shape[1], g.shape[2], 3, 3)


def bias_grad(dy):
    return dy.reshape(-1, dy.shape[3]).sum(0)
