"""CPU reference of the faithfulness-curve helpers (gava_patch_ranks, gava_blur_clips, gava_perturb_clips, gava_perturb_scores):
the table of cases, the value regimes and the bounds.  test_perturbation_host.py checks the reference against the definitions
on the CPU, test_gpu_perturbation.py the kernels against the reference.  Nothing here touches a device or the library.

Ordering rule (include/gava_hip.h): unit j is BEFORE unit i when s_j > s_i, or s_j == s_i (-0 == +0) and j < i; every NaN is
after -inf, NaNs among themselves by index.  rank_i = #{j : j before i}.
"""
import math

import numpy as np
import torch

MAX_UNITS = 65536
U = 2.0 ** -24           # fp32 unit roundoff


# ---- ranks ------------------------------------------------------------------------------------------------------------
def ranks_1d(s):
    """Ranks of one ranking by a stable sort: primary key NaN-ness (NaNs last), then the value descending (-0 and +0 are the
    same float64 key after adding 0.0), ties kept in index order by the sort's stability."""
    s = np.asarray(s, dtype=np.float64)
    nan = np.isnan(s)
    v = np.where(nan, 0.0, s) + 0.0                      # -0.0 + 0.0 = +0.0
    order = np.lexsort((np.arange(s.size), -v, nan))     # last key first: NaN-ness, then -value, then index
    r = np.empty(s.size, dtype=np.int32)
    r[order] = np.arange(s.size, dtype=np.int32)
    return r


def ranks_by_counting(s):
    """The O(n^2) definition itself."""
    s = [float(v) for v in s]
    n = len(s)

    def before(j, i):
        a, b = s[j], s[i]
        if math.isnan(a) or math.isnan(b):
            return (not math.isnan(a) and math.isnan(b)) or (math.isnan(a) and math.isnan(b) and j < i)
        return a > b or (a == b and j < i)
    return np.array([sum(before(j, i) for j in range(n)) for i in range(n)], dtype=np.int32)


def pool_pixels(scores, P):
    """[B, T, S, S] -> [B, T, g, g]: the sum over each P x P patch.  Exact in float64 for the integer-valued scores the tests
    use (|v| <= 1024, at most 256 per patch: every partial sum is an integer below 2^24, so fp32 gets the same value in any
    order)."""
    B, T, S, _ = scores.shape
    g = S // P
    return scores.double().view(B, T, g, P, g, P).sum((3, 5))


def ranks(scores, scope="clip", patch=None):
    """scores fp32 [B, T, g, g] / [B, T, S, S] with patch=P / [B, T] -> int32 [B, units] as gava_patch_ranks writes them."""
    if scores.dim() == 4 and patch is not None:
        scores = pool_pixels(scores, patch)
    B = scores.shape[0]
    flat = scores.reshape(B, -1).double().numpy()
    if scope == "clip":
        return torch.from_numpy(np.stack([ranks_1d(row) for row in flat]))
    assert scores.dim() == 4
    T, gg = scores.shape[1], scores.shape[2] * scores.shape[3]
    return torch.from_numpy(np.stack([np.concatenate([ranks_1d(row[t * gg:(t + 1) * gg]) for t in range(T)]) for row in flat]))


REGIMES = ("randn", "equal", "half_zero", "ascending", "descending", "special")


def regime_scores(shape, regime, seed):
    """fp32 scores of `shape` in one of the value regimes."""
    gen = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    if regime == "randn":
        s = torch.randn(n, generator=gen)
    elif regime == "equal":
        s = torch.full((n,), 0.37)
    elif regime == "half_zero":                          # what relevance's positive part produces: exact zeros among positives
        s = torch.randn(n, generator=gen).clamp_(min=0)
    elif regime == "ascending":
        s = torch.arange(n, dtype=torch.float32) * 0.25 - 3.0
    elif regime == "descending":
        s = -(torch.arange(n, dtype=torch.float32) * 0.25 - 3.0)
    elif regime == "special":                            # duplicates, +-0, +-inf, NaNs
        pool = torch.tensor([0.0, -0.0, 1.5, 1.5, -2.0, float("inf"), float("-inf"), float("nan"), float("nan"), 3e38, -3e38, 1e-45])
        s = pool[torch.randint(0, pool.numel(), (n,), generator=gen)]
    else:
        raise ValueError(regime)
    return s.view(shape).contiguous()


def integer_pixels(B, T, S, seed):
    """Integer-valued pixel scores, |v| <= 1024: every summation order pools to the same fp32 value."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, (B, T, S, S), generator=gen).float()


# (B, T, g) of the patch-layout rank cases; every one runs in both scopes
RANK_PATCH_CASES = [(2, 4, 4), (2, 8, 14)]
RANK_FRAME_T = [1, 320]
RANK_PIXEL_CASES = [(2, 4, 64, 16), (2, 3, 28, 14)]      # (B, T, S, P)


# ---- thresholds -------------------------------------------------------------------------------------------------------
def thresholds(n, fractions):
    return [int(math.floor(float(f) * n + 0.5)) for f in fractions]


def linspace_fractions(steps):
    return [s / steps for s in range(steps + 1)]


# ---- perturbed clips ----------------------------------------------------------------------------------------------------
def unit_ranks_per_pixel(rk, T, S, P):
    """ranks [B, T*g*g] or [B, T] -> the rank of every pixel's unit, [B, 1, T, S, S] (frame units when the row is T long and
    patch units would not be)."""
    B, g = rk.shape[0], S // P
    if rk.shape[1] == T * g * g:
        r = rk.view(B, T, g, 1, g, 1).expand(B, T, g, P, g, P).reshape(B, T, S, S)
    else:
        r = rk.view(B, T, 1, 1).expand(B, T, S, S)
    return r.unsqueeze(1)


def perturb(x, rk, ks, P, mode, baseline=None):
    """-> [B, S1, 3, T, S, S]: torch.where only, so every word is x's or the baseline's."""
    B, _, T, S, _ = x.shape
    r = unit_ranks_per_pixel(rk, T, S, P)
    if baseline is None:
        base = torch.zeros_like(x)
    elif baseline.dim() == 1:
        base = baseline.view(1, 3, 1, 1, 1).expand_as(x)
    else:
        base = baseline
    out = []
    for k in ks:
        hit = (r < k).expand_as(x)
        out.append(torch.where(hit, base, x) if mode == "deletion" else torch.where(hit, x, base))
    return torch.stack(out, 1).contiguous()


# (B, T, S, P, S1, frame units)
PERTURB_CASES = [(2, 4, 64, 16, 11, False), (1, 3, 28, 14, 1, False), (1, 3, 28, 14, 4, False), (1, 8, 224, 16, 3, False),
                 (2, 4, 64, 16, 5, True)]


def perturb_case_thresholds(n, S1):
    """S1 thresholds from 0 to n; with four or more the second one is repeated (repeats are allowed)."""
    if S1 == 1:
        return [n // 2]
    ks = thresholds(n, linspace_fractions(S1 - 1))
    if S1 >= 4:
        ks[2] = ks[1]
    return ks


# ---- blur ---------------------------------------------------------------------------------------------------------------
def gaussian_taps(sigma):
    r = int(math.ceil(3.0 * sigma))
    w = torch.exp(-torch.arange(-r, r + 1, dtype=torch.float64) ** 2 / (2.0 * sigma * sigma))
    return (w / w.sum()).float()


def blur(x, taps, dtype=torch.float64):
    """Separable convolution with replicate padding on the given fp32 taps, along x then along y, in `dtype`."""
    r = taps.numel() // 2
    S = x.shape[-1]
    w = taps.to(dtype)
    idx = (torch.arange(S).view(S, 1) + torch.arange(-r, r + 1).view(1, -1)).clamp_(0, S - 1)       # [S, 2r+1]
    v = x.to(dtype)
    if dtype == torch.float32:                           # one product and one sum per tap, in tap order
        h = torch.zeros_like(v)
        for i in range(2 * r + 1):
            h = h + w[i] * v[..., idx[:, i]]
        o = torch.zeros_like(v)
        for i in range(2 * r + 1):
            o = o + w[i] * h[..., idx[:, i], :]
        return o
    h = (v[..., idx] * w).sum(-1)                        # [..., S(y), S(x)]
    return (h[..., idx, :] * w.view(1, -1, 1)).sum(-2)


def blur_bound(taps, x):
    """|d| <= 2 (2r + 2) 2^-24 max|x|: two passes of 2r + 1 products and sums in fp32."""
    return 2 * (taps.numel() + 1) * U * float(x.abs().max())


BLUR_CASES = [(1, 2, 28, 5.0), (1, 2, 64, 1.0), (1, 2, 64, 5.0)]     # (B, T, S, sigma); one 224^2 plane is cut from a [1, 3, 1] clip


# ---- scores ---------------------------------------------------------------------------------------------------------------
def scores_ref(logits, S1, fractions, target, ref_step):
    """logits fp32 [nb * S1, C] -> dict in float64 / int64; fractions are used as the fp32 values the kernel gets.
    target None: the argmax of each clip's row ref_step, lowest class on ties (np.argmax returns the first maximum)."""
    nb, C = logits.shape[0] // S1, logits.shape[1]
    lg = logits.double().view(nb, S1, C)
    top1 = torch.from_numpy(np.argmax(lg.numpy(), axis=2))
    tgt = top1[:, ref_step].clone() if target is None else target.clone()
    ok = (tgt >= 0) & (tgt < C)
    safe = tgt.clamp(0, C - 1)
    logit = lg.gather(2, safe.view(nb, 1, 1).expand(nb, S1, 1)).squeeze(2)
    prob = lg.softmax(-1).gather(2, safe.view(nb, 1, 1).expand(nb, S1, 1)).squeeze(2)
    logit[~ok] = float("nan")
    prob[~ok] = float("nan")
    f = torch.tensor(fractions, dtype=torch.float32).double()
    df = (f[1:] - f[:-1]).view(1, -1)
    auc = lambda y: (df * (y[:, 1:] + y[:, :-1]) / 2).sum(1) if S1 > 1 else y[:, 0] * 0.0       # (NaN stays NaN)
    return dict(logit=logit, prob=prob, top1=top1, auc_logit=auc(logit), auc_prob=auc(prob), target=tgt)


PROB_TOL = 1e-5          # tests/test_gpu_views.py: fp32 softmax, u = 2^-24
SCORE_CASES = [(3, 1), (3, 11), (400, 1), (400, 11)]     # (C, S1)


def auc_logit_bound(S1, logits):
    return (S1 + 2) * U * float(logits.abs().max())
