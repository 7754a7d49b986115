"""fp64 restatement of the training criterion (include/gava_hip.h, gava_train_criterion) and its closed-form gradient, in numpy.

Pinned to the reference by tests/test_train_criterion_host.py: it reproduces tests/golden/loss_ref.npz, which
tools/gen_golden_loss.py wrote from the reference's own training/loss_utils.py and torch.nn.CrossEntropyLoss under autograd in
fp64.  The GPU tests then measure the kernels against this file at any shape.

Per sample i with label y:  p = softmax(z_i),  ce = logsumexp(z_i) - z_iy,  k = argmax_c z_ic (the lowest class on ties),
    w = scale * (fl(beta * fl(|y - k| / (C - 1))) + alpha * (1 - p_y)^gamma),  l = ce * w  (or ce, unweighted),   loss = mean l
    d loss / d z_ic = (w + ce * scale * alpha * gamma * (1 - p_y)^(gamma - 1) * p_y) * (p_c - [c == y]) * g / B
fl(): the reference casts the ordinal fraction to fp32 whatever the logits' type (`.float()`, loss_utils.py:38) and multiplies
it by beta in that type (:42) before the sum with the focal factor promotes it, so its fp64 run carries those two roundings too.  The ordinal term has no gradient (the argmax passes none); the bracket is 1 unweighted.
"""
import numpy as np


def criterion(logits, labels, *, weighted, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, g=1.0):
    """-> dict(loss, per_sample [B], weight [B], top1 [B], hits, conf [C, C], dlogits [B, C]), all float64 / int64."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    B, C = z.shape
    rows = np.arange(B)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    ce = (m[:, 0] + np.log(s[:, 0])) - z[rows, y]
    top1 = z.argmax(axis=1)                         # numpy, like torch, returns the first maximum
    py = p[rows, y]
    omp = (e.sum(axis=1) - e[rows, y]) / s[:, 0]    # 1 - p_y without the cancellation at p_y -> 1
    if weighted:
        ordinal = (np.float32(beta) * (np.abs(y - top1) / (C - 1)).astype(np.float32)).astype(np.float64)
        w = scale * (ordinal + alpha * omp ** gamma)
        a = w + ce * scale * alpha * gamma * omp ** (gamma - 1.0) * py
        per = ce * w
    else:
        w, a, per = np.ones(B), np.ones(B), ce
    onehot = np.zeros((B, C))
    onehot[rows, y] = 1.0
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (y, top1), 1)
    return dict(loss=per.mean(), per_sample=per, weight=w, top1=top1, hits=int((top1 == y).sum()), conf=conf,
                dlogits=a[:, None] * (p - onehot) * (g / B))
