#!/usr/bin/env python
"""Generate tests/golden/tiny_path_grads.npz: the REFERENCE's path-mean and noise-mean gradients with respect to the input clip.

Runs only in the build container, where the reference checkout is (tools/gen_golden.py's REF), like tools/gen_golden_input_grad.py.
It builds the reference's ``VitaCLIP`` at the TINY shape with the synthetic weights (tools/gen_golden.py's own builders), takes
``x = synth_clip(2, 4, 64)`` and the targets [1, 2], and differentiates the target's raw logit under fp32 torch autograd.  Nothing
of the model is restated here.

(a) integrated gradients: the 8 trapezoid interpolants alpha_k x from the zero baseline (alpha_k = k / 7, end weights halved) ->
    ig_mean_grad [2, 3, 4, 64, 64] = sum_k w_k grad_k, ig_sum_attr [2] = sum(x * mean grad), ig_f_x / ig_f_x0 [2] (the target's logit
    at both ends), ig_logits_x / ig_logits_x0 [2, 3].
(b) SmoothGrad: 4 noisy copies x + sigma_b z, sigma_b = 0.15 (max - min) of clip b, z from tests/path_grad_ref.py's generator
    (seed 7, clip b, copy k) -> sg_mean_grad [2, 3, 4, 64, 64], sg_sigma [2].

The file holds data only, ~0.8 MB.

    python tools/gen_golden_path_grad.py
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

sys.path.insert(0, os.path.join(gg.REPO, "tests"))
import path_grad_ref as ref  # noqa: E402

from gava_clip_amd import synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402

TARGET = [1, 2]
STEPS, SAMPLES, SEED, SIGMA = 8, 4, 7, 0.15


def grads_of(model, clips, target):
    """clips [N, 3, T, S, S], target [N] -> (logits [N, C], d logits[n, target_n] / d clips[n])."""
    xs = clips.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, lmt, lvm = model(xs)
    assert lmt is None and lvm is None
    logits.gather(1, target.view(-1, 1)).sum().backward()
    assert xs.grad is not None and bool(torch.isfinite(xs.grad).all())
    return logits.detach(), xs.grad


def main():
    torch.set_num_threads(8)
    mod, _ = gg.import_reference()
    assert mod.__file__.startswith(gg.REF)
    model = gg.build_reference(mod, TINY, os.path.join(gg.CLASSES, "updrs_3cls_classes.txt"))
    gg.load_synth(model, TINY, 3)
    model.train()
    x = torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size))
    B = x.shape[0]
    target = torch.tensor(TARGET)
    # (a) the trapezoid path from zero; copy k of clip b is batch index b * STEPS + k
    alpha, w = ref.trapezoid(STEPS)
    pts = ref.line(x, None, alpha).float().reshape(B * STEPS, *x.shape[1:])
    assert torch.equal(pts.view(B, STEPS, *x.shape[1:])[:, -1], x) and not pts.view(B, STEPS, -1)[:, 0].any()
    logits, g = grads_of(model, pts, target.repeat_interleave(STEPS))
    w64 = torch.tensor(w, dtype=torch.float64).view(1, STEPS, 1, 1, 1, 1)
    mean = (w64 * g.double().view(B, STEPS, *x.shape[1:])).sum(1)
    lg = logits.view(B, STEPS, -1)
    f = lg.gather(2, target.view(B, 1, 1).expand(B, STEPS, 1)).squeeze(2)
    out = dict(target=target.numpy(), ig_alpha=np.array(alpha), ig_w=np.array(w), ig_mean_grad=mean.float().numpy(),
               ig_sum_attr=(x.double() * mean).reshape(B, -1).sum(1).numpy(), ig_f_x=f[:, -1].numpy(), ig_f_x0=f[:, 0].numpy(),
               ig_logits_x=lg[:, -1].numpy(), ig_logits_x0=lg[:, 0].numpy())
    # (b) the noisy copies
    flat = x.reshape(B, -1)
    sigma = torch.tensor(SIGMA, dtype=torch.float32) * (flat.amax(1) - flat.amin(1))
    z = ref.noise(SEED, 0, B, SAMPLES, flat.shape[1])
    noisy = (flat.double().unsqueeze(1) + sigma.double().view(B, 1, 1) * z).float().reshape(B * SAMPLES, *x.shape[1:])
    _, g = grads_of(model, noisy, target.repeat_interleave(SAMPLES))
    out.update(sg_sigma=sigma.numpy(), sg_mean_grad=g.double().view(B, SAMPLES, *x.shape[1:]).mean(1).float().numpy())
    path = os.path.join(gg.REPO, "tests", "golden", "tiny_path_grads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; sum_attr", out["ig_sum_attr"], "f_x - f_x0", out["ig_f_x"] - out["ig_f_x0"],
          "|sg| =", float(np.linalg.norm(out["sg_mean_grad"])))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
