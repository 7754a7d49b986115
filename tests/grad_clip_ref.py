"""fp64 numpy restatement of clipping by global norm as gava_grad_norm / gava_adamw_step_clipped define it (include/gava_hip.h):
torch's GradScaler.unscale_ + clip_grad_norm_(norm_type=2) + AdamW step, with one deviation: a non-finite norm skips the step
where torch would scale every gradient by NaN.  The step itself is tests/optim_ref.py::adamw_step, called, not copied.
tests/test_grad_clip_host.py pins this file against torch on float64 tensors; the GPU tests measure the kernels against it."""
import numpy as np

from optim_ref import adamw_step


def unscaled(grads, grad_scale=None, fp32_product=False):
    """The gradients the norm is taken of: g * (1 / grad_scale).  fp32_product=True rounds the reciprocal and every product to
    fp32 first, as the kernels do (x_i = fl32(g_i * inv_scale)); the sums that follow are fp64 either way."""
    if grad_scale is None:
        return [None if g is None else np.asarray(g, dtype=np.float64) for g in grads]
    if fp32_product:
        inv = np.float32(1.0) / np.float32(grad_scale)
        return [None if g is None else (np.asarray(g, dtype=np.float32) * inv).astype(np.float64) for g in grads]
    inv = 1.0 / float(grad_scale)
    return [None if g is None else np.asarray(g, dtype=np.float64) * inv for g in grads]


def grad_norm(grads, max_norm, grad_scale=None, fp32_product=False):
    """(tensor_norm, norm, coef, nonfinite): per-tensor norms (0 where grads[i] is None), the global norm, the coefficient
    min(1, max_norm / (norm + 1e-6)) and the skip flag.  nonfinite: the sum of squares is inf or NaN; the coefficient is then 1."""
    with np.errstate(over="ignore", invalid="ignore"):
        sums = [0.0 if g is None else float(np.sum(np.square(g), dtype=np.float64)) for g in unscaled(grads, grad_scale, fp32_product)]
        total = float(np.sum(np.asarray(sums, dtype=np.float64))) if sums else 0.0
        norm = float(np.sqrt(total))
        nonfinite = not np.isfinite(total)
        coef = 1.0 if nonfinite else min(1.0, float(max_norm) / (norm + 1e-6))
        return [float(np.sqrt(s)) for s in sums], norm, coef, nonfinite


def clipped_adamw_step(params, grads, state, groups, group_of, max_norm, grad_scale=None, found_inf=None):
    """One clipped step, in place like adamw_step; returns what grad_norm returns.  The stats do not depend on found_inf; the
    step is skipped when found_inf != 0 or the norm is not finite."""
    tn, norm, coef, nonfinite = grad_norm(grads, max_norm, grad_scale)
    if not nonfinite:
        clipped = [None if g is None else g * coef for g in unscaled(grads, grad_scale)]
        adamw_step(params, clipped, state, groups, group_of, found_inf=found_inf)
    return tn, norm, coef, nonfinite
