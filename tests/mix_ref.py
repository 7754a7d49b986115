"""fp64 restatement, in numpy, of the mix of the clips, the soft targets and the criterion for targets of the logits' shape with
its closed-form gradient (include/gava_hip.h: gava_mix_clips, gava_mix_targets, gava_soft_criterion).

The criterion is pinned to the reference by tests/test_mix_host.py: it reproduces tests/golden/soft_loss_ref.npz, which
tools/gen_golden_soft_loss.py wrote from the reference's own training/loss_utils.py and torch.nn.CrossEntropyLoss (class
probabilities) under autograd in fp64.  The GPU tests then measure the kernels against this file at any shape.

Per sample with logits z, targets t and tau = sum_c t_c:
    p = softmax(z),  ce = sum_c t_c (logsumexp(z) - z_c),  k = argmax z,  y* = argmax t (the lowest index on ties)
    w = scale * (fl(beta * fl(|y* - k| / (C - 1))) * tau + alpha * sum_c t_c (1 - p_c)^gamma),  l = ce * w (or ce),  loss = mean l
    Q = sum_c t_c (1 - p_c)^(gamma - 1) p_c
    d loss / d z_c = (w (tau p_c - t_c) + ce scale alpha gamma p_c (Q - t_c (1 - p_c)^(gamma - 1))) * g / B
fl(): the reference casts the ordinal fraction to fp32 whatever the logits' type and multiplies it by beta in that type
(loss_utils.py:38,42), as tests/loss_ref.py notes.  The ordinal term has no gradient.  Unweighted: w = 1 and no second term.
"""
import numpy as np


def mix_clips(x, partner, lam, box):
    """x [B, planes, H, W] (any float type; computed in fp64 on those values), partner int [B], lam [B] (used as given: pass
    the fp32 values the kernel reads), box int [B, 4] as (y0, y1, x0, x1).
    -> (out float64, exact bool: where out must equal a or b bit for bit, scale float64: lam |a| + (1 - lam) |b| elsewhere)."""
    x = np.asarray(x)
    x64 = x.astype(np.float64)
    B = x.shape[0]
    out, exact, scale = x64.copy(), np.ones(x.shape, dtype=bool), np.zeros(x.shape)
    for i in range(B):
        j = int(partner[i])
        y0, y1, x0, x1 = (int(v) for v in box[i])
        if j == i:
            continue
        if y1 > y0 and x1 > x0:
            out[i, :, y0:y1, x0:x1] = x64[j, :, y0:y1, x0:x1]
            continue
        l = float(lam[i])
        if l == 1.0:
            continue
        if l == 0.0:
            out[i] = x64[j]
            continue
        out[i] = l * x64[i] + (1.0 - l) * x64[j]
        exact[i] = False
        scale[i] = l * np.abs(x64[i]) + (1.0 - l) * np.abs(x64[j])
    return out, exact, scale


def mix_targets(labels, partner, lam, C, smoothing):
    """-> targets float64 [B, C]; labels clamped to [0, C); a clip that is its own partner keeps its smoothed label."""
    y = np.clip(np.asarray(labels, dtype=np.int64), 0, C - 1)
    B = y.shape[0]
    s = np.full((B, C), smoothing / C)
    s[np.arange(B), y] += 1.0 - smoothing
    partner = np.asarray(partner, dtype=np.int64)
    l = np.where(partner == np.arange(B), 1.0, np.asarray(lam, dtype=np.float64))[:, None]
    return l * s + (1.0 - l) * s[partner]


def soft_criterion(logits, targets, *, weighted, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, g=1.0):
    """-> dict(loss, per_sample [B], weight [B], top1 [B], target1 [B], hits, conf [C, C], dlogits [B, C]), float64 / int64."""
    z = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    B, C = z.shape
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    omp = (s - e) / s                                # 1 - p_c without the cancellation at p_c -> 1
    lse = m + np.log(s)
    tau = t.sum(axis=1)
    ce = (t * (lse - z)).sum(axis=1)
    top1, target1 = z.argmax(axis=1), t.argmax(axis=1)          # numpy, like torch, returns the first maximum
    if weighted:
        ordinal = (np.float32(beta) * (np.abs(target1 - top1) / (C - 1)).astype(np.float32)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            pg = np.where(t != 0, t * omp ** gamma, 0.0)
            pg1 = np.where(t != 0, t * omp ** (gamma - 1.0), 0.0)
        w = scale * (ordinal * tau + alpha * pg.sum(axis=1))
        q = (pg1 * p).sum(axis=1)
        per = ce * w
        d = w[:, None] * (tau[:, None] * p - t) + (ce * scale * alpha * gamma)[:, None] * p * (q[:, None] - pg1)
    else:
        w, per = np.ones(B), ce
        d = tau[:, None] * p - t
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (target1, top1), 1)
    return dict(loss=per.mean(), per_sample=per, weight=w, top1=top1, target1=target1, hits=int((top1 == target1).sum()), conf=conf,
                dlogits=d * (g / B))
