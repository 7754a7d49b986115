"""Restatements of the auxiliary heads and their loss terms (include/gava_hip.h, gava_nte_head / gava_memory_head /
gava_sigmoid_criterion / gava_nte_diag_loss), in a form of their own: what the GPU tests measure the kernels against, at any
shape and in any dtype (fp64 on the CPU as the reference, fp32 on the GPU as "what torch ops give").

Pinned two ways.  sigmoid_loss reproduces tests/golden/aux_loss_ref.npz, which tools/gen_golden_aux_loss.py wrote from the
reference's own training/loss_utils.py under autograd in fp64 (tests/test_aux_heads_host.py: values 1e-12, gradients 1e-10).
The heads are pinned through the model: tests/test_gpu_aux_heads.py runs the kernels inside VitaCLIP against
tests/golden/tiny_aux_grads.npz, the reference model's outputs and gradients.

sigmoid_loss, per sample with t = +1 at the label and -1 elsewhere:  ce = softplus(-t x),  q = sigmoid(-t x) = 1 - p_t,
    term = ce                         d term / dx = -t q
    term = alpha_t q^gamma ce         d term / dx = -t alpha_t q^gamma (gamma (1 - q) ce + q)         (use_focal)
    per_sample = scale * sum_c term,  loss = mean,  alpha_t = fl(alpha) at the label, fl(1 - alpha) elsewhere
fl(): the reference builds alpha_t from the fp32 one-hot labels (`y_true.float()`, loss_utils.py:151,158), so its fp64 run carries
alpha and 1 - alpha rounded to fp32.
"""
import numpy as np
import torch


def sigmoid_loss(logits, labels, *, use_focal=False, alpha=0.25, gamma=2.0, scale=1.0, g=1.0):
    """-> dict(loss, per_sample [M], dlogits [M, C]) in float64."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    M, C = x.shape
    pos = np.arange(C)[None, :] == y[:, None]
    t = np.where(pos, 1.0, -1.0)
    v = -t * x
    ce = np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))
    e = np.exp(-np.abs(v))
    q = np.where(v >= 0, 1.0, e) / (1.0 + e)              # sigmoid(v)
    omq = np.where(v >= 0, e, 1.0) / (1.0 + e)            # sigmoid(-v) = 1 - q without the cancellation
    if use_focal:
        a_t = np.where(pos, np.float64(np.float32(alpha)), np.float64(np.float32(1.0 - alpha)))      # fl(), see above
        term = a_t * q ** gamma * ce
        d = -t * a_t * q ** gamma * (gamma * omq * ce + q)
    else:
        term, d = ce, -t * q
    per = term.sum(axis=1) * scale
    return dict(loss=per.mean(), per_sample=per, dlogits=d * (scale * g / M))


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def nte_head(summary, weight, bias, video_nte, scale):
    """logits_vm [B, B] in the mean-of-unit-rows form (the reference's mean over the K products, by linearity)."""
    sp = unit(summary @ weight.t() + bias)
    valid = (video_nte.sum(dim=(1, 2)) != 0).to(summary.dtype)
    sim = sp @ unit(video_nte).mean(dim=1).t()
    lm = scale * (sim * (valid[:, None] * valid[None, :]))
    return torch.log_softmax(lm, dim=-1) + torch.log_softmax(lm, dim=-2)


def memory_head(memory, text_features, tf_params, mem_params, scale, bias=None):
    """logits_mt [M, C]; tf_params = (W1 [H1, E], b1, W2 [H2, H1], b2), mem_params the same four stacked over the classes
    ([C, H1, E], [C, H1], [C, H2, H1], [C, H2]): one batched product over the classes per layer."""
    w1, b1, w2, b2 = tf_params
    u = unit(torch.tanh(text_features @ w1.t() + b1) @ w2.t() + b2)                                   # [C, H2]
    W1, B1, W2, B2 = mem_params
    mm = memory.mean(dim=1)                                                                           # [M, E]
    h = torch.tanh(torch.einsum("me,che->cmh", mm, W1) + B1[:, None, :])
    z = unit(torch.einsum("cmh,ckh->cmk", h, W2) + B2[:, None, :])                                    # [C, M, H2]
    out = torch.log_softmax(scale * torch.einsum("cmk,ck->mc", z, u), dim=-1)
    return out if bias is None else out + bias


def nte_diag(logits_vm, weight):
    return -weight * torch.diagonal(logits_vm).mean()
