"""fp64 numpy restatement of one AdamW step as gava_adamw_step defines it (include/gava_hip.h): torch.optim.AdamW with
amsgrad = False, maximize = False, plus GradScaler's grad_scale / found_inf and torch's handling of a missing gradient.
tests/test_fused_adamw_host.py pins it against torch.optim.AdamW on float64 tensors; the GPU tests measure the kernel against it."""
import numpy as np


def adamw_step(params, grads, state, groups, group_of, grad_scale=None, found_inf=None):
    """In place on `params` (list of float64 arrays) and `state` (list of dicts step / exp_avg / exp_avg_sq, {} before the first
    step).  grads[i] is None for a parameter without a gradient: it is skipped entirely.  groups: list of dicts lr, betas, eps,
    weight_decay; group_of[i] indexes it.  A non-zero found_inf skips the whole step."""
    if found_inf is not None and float(found_inf) != 0.0:
        return
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        h = groups[group_of[i]]
        st = state[i]
        if not st:
            st.update(step=0.0, exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
        g = np.asarray(g, dtype=np.float64)
        if grad_scale is not None:
            g = g * (1.0 / float(grad_scale))
        b1, b2 = h["betas"]
        t = st["step"] + 1.0
        p *= 1.0 - h["lr"] * h["weight_decay"]
        st["exp_avg"] += (g - st["exp_avg"]) * (1.0 - b1)
        st["exp_avg_sq"] *= b2
        st["exp_avg_sq"] += (1.0 - b2) * g * g
        denom = np.sqrt(st["exp_avg_sq"]) / np.sqrt(1.0 - b2 ** t) + h["eps"]
        p -= (h["lr"] / (1.0 - b1 ** t)) * (st["exp_avg"] / denom)
        st["step"] = t
