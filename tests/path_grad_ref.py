"""CPU restatement of the path-gradient helpers (gava_path_clips, gava_clip_range, gava_unpatchify_path, gava_path_delta; the
"path gradients" section of include/gava_hip.h): the checker of the kernels.  test_path_grad_host.py pins it - Philox4x32-10 to
the Random123 known answers, the weighted fold to fp64 autograd - and test_gpu_path_grad.py holds the kernels against it.
Nothing here touches a device or the library."""
import numpy as np
import torch

import input_grad_ref

LINE, NOISE = 0, 1
GRAD, ABSMAX, L2, ATTR, ATTR_SUM, ATTR_ABS = 0, 1, 2, 3, 4, 5
MAX_STEPS = 64
U = 2.0 ** -24           # fp32 unit roundoff

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al.): ctr = four 32-bit words (ints or equal-shaped integer arrays), key = two ints
    -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)          # 32 x 32 bits: fits 64
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def box_muller(ra, rb):
    """Two 32-bit words -> two standard normals in float64, on the exact 24-bit uniforms u1 = ((ra >> 8) + 1) 2^-24 in (0, 1]
    and u2 = (rb >> 8) 2^-24 in [0, 1)."""
    u1 = ((ra >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    radius = np.sqrt(-2.0 * np.log(u1))
    return radius * np.cos(2.0 * np.pi * u2), radius * np.sin(2.0 * np.pi * u2)


def normals(seed, clip, k, n):
    """The n (a multiple of 4) normals of copy k of global clip `clip`, float64 [n]: group e4 of four consecutive elements comes
    from counter (e4 low, e4 high, k, clip) under key (seed low, seed high)."""
    assert n % 4 == 0
    e4 = np.arange(n // 4, dtype=np.uint64)
    r = philox4x32_10((e4 & _MASK, e4 >> _32, np.full_like(e4, k), np.full_like(e4, clip)), (seed & 0xFFFFFFFF, seed >> 32))
    z0, z1 = box_muller(r[0], r[1])
    z2, z3 = box_muller(r[2], r[3])
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(n)


def noise(seed, clip0, nb, m, n):
    """-> float64 tensor [nb, m, n]: z of clips clip0 ... clip0 + nb - 1."""
    return torch.from_numpy(np.stack([np.stack([normals(seed, clip0 + b, k, n) for k in range(m)]) for b in range(nb)]))


def baseline_like(x, baseline):
    """None / [3] / shaped like x -> a tensor shaped like x, in x's dtype."""
    if baseline is None:
        return torch.zeros_like(x)
    if baseline.dim() == 1:
        return baseline.to(x.dtype).view(1, 3, 1, 1, 1).expand_as(x)
    return baseline.to(x.dtype)


def f32_pair(alpha):
    """The (alpha, beta) the binding passes: both rounded to fp32 from float64, beta = 1 - alpha formed in float64."""
    a = torch.tensor([float(v) for v in alpha], dtype=torch.float64)
    return a.float(), (1.0 - a).float()


def line(x, baseline, alpha):
    """-> float64 [nb, m, 3, T, S, S]: alpha_k x + beta_k x0 on the fp32 alpha / beta, unrounded."""
    a, b = f32_pair(alpha)
    x64, x0 = x.double(), baseline_like(x.double(), baseline)
    shape = (1, -1, 1, 1, 1, 1)
    return a.double().view(shape) * x64.unsqueeze(1) + b.double().view(shape) * x0.unsqueeze(1)


def trapezoid(m):
    return [k / (m - 1) for k in range(m)], [(0.5 if k in (0, m - 1) else 1.0) / (m - 1) for k in range(m)]


def gauss_legendre(n):
    t, w = np.polynomial.legendre.leggauss(n)
    return [0.0] + [float(0.5 * (v + 1.0)) for v in t] + [1.0], [0.0] + [float(0.5 * v) for v in w] + [0.0]


def reduce_path(g, w, mode, x=None, baseline=None):
    """The reduction of gava_unpatchify_path on folded gradients g [B, m, 3, T, S, S], in g's dtype -> (value, s_abs); w as the
    fp32 values the kernel gets.  s_abs is the same expression with every term replaced by its absolute value - what a rounding
    error of the chain is relative to."""
    dt, m = g.dtype, g.shape[1]
    w = torch.tensor([float(v) for v in w], dtype=torch.float32).to(dt)
    G, A = torch.zeros_like(g[:, 0]), torch.zeros_like(g[:, 0])
    for k in range(m):                                   # the kernel's order; a zero weight's step is not read
        if float(w[k]) != 0.0:
            G = G + w[k] * g[:, k]
            A = A + (w[k] * g[:, k]).abs()
    if mode >= ATTR:
        d = x.to(dt) - baseline_like(x.to(dt), baseline)
        G, A = d * G, d.abs() * A
    if mode in (GRAD, ATTR):
        return G, A
    if mode == ABSMAX:
        return G.abs().amax(1), A.amax(1)
    if mode == L2:
        return (G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2]).sqrt(), (A * A).sum(1).sqrt()
    if mode == ATTR_SUM:
        return G[:, 0] + G[:, 1] + G[:, 2], A.sum(1)
    if mode == ATTR_ABS:
        return G[:, 0].abs() + G[:, 1].abs() + G[:, 2].abs(), A.sum(1)
    raise ValueError(mode)


def fold_path(dpatch, B, m, T, size, P, frame_rows, row_offset, w, mode, x=None, baseline=None):
    """gava_unpatchify_path in dpatch's dtype -> (value, s_abs): dpatch holds the B*m*T frames of the copies (clip b's copy k is
    batch index b*m + k)."""
    g = input_grad_ref.fold(dpatch, B * m, T, size, P, frame_rows, row_offset).view(B, m, 3, T, size, size)
    return reduce_path(g, w, mode, x, baseline)


def fold_bound(m, s_abs):
    """m roundings of the chain, the subtraction, the product, the channel sums (or the squares and the root): (m + 8) u."""
    return (m + 8) * U * s_abs


def delta(attr, logits, target, m, k_lo, k_hi):
    """-> (sum64 [B], f_diff64 [B], sum of |a| [B]) in float64; a target outside [0, C) gives NaN in the first two."""
    B, C = attr.shape[0], logits.shape[1]
    a = attr.double().reshape(B, -1)
    lg = logits.double().view(B, m, C)
    ok = (target >= 0) & (target < C)
    safe = target.clamp(0, C - 1)
    f = lg[torch.arange(B), k_hi, safe] - lg[torch.arange(B), k_lo, safe]
    s = a.sum(1)
    s[~ok] = float("nan")
    f[~ok] = float("nan")
    return s, f, a.abs().sum(1)
