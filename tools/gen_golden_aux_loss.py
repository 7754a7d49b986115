#!/usr/bin/env python
"""Generate tests/golden/aux_loss_ref.npz: the REFERENCE's sigmoid_focal_loss on a handful of (logits, labels) sets.

Runs only where /root/reference exists (never on the GPU box), like tools/gen_golden_loss.py.  It imports the reference's
``training/loss_utils.py`` and evaluates, in fp64 under torch autograd, what training/train.py:365,459-462 does with it:
``sigmoid_focal_loss(alpha, gamma, use_focal, scale)(logits, labels)`` per sample, then ``.mean()``; ``loss.backward()`` gives
dlogits.  Nothing of the criterion is restated here.

The file holds data only.  Per set s: logits_s [M, C] float64, labels_s [M] int64, params_s = (use_focal, alpha, gamma, scale),
per_sample_s, loss_s, dlogits_s.  The sets cover C = 1, 3, 4 and M = 1, 7, both use_focal values, entries of |x| ~ 30 of either
sign at and off the label, labels 0 and C - 1, gamma 1 and 2, and a scale other than 1.

    python tools/gen_golden_aux_loss.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True


def make_sets():
    rng = np.random.default_rng(2718)
    sets = []
    for s, (M, C, focal, alpha, gamma, scale) in enumerate([(7, 3, 0, 0.25, 2.0, 1.0), (7, 3, 1, 0.25, 2.0, 1.0), (1, 3, 0, 0.25, 2.0, 1.0),
                                                            (1, 3, 1, 0.25, 2.0, 0.5), (7, 4, 0, 0.25, 2.0, 2.25), (7, 4, 1, 0.4, 1.0, 3.0),
                                                            (7, 1, 1, 0.25, 2.0, 1.0), (1, 1, 0, 0.25, 2.0, 1.0), (1, 4, 1, 0.25, 3.5, 1.0)]):
        z = rng.standard_normal((M, C)) * 3.0 - 1.0
        y = rng.integers(0, C, M)
        y[0] = C - 1
        if M == 7:
            y[1], y[2] = 0, C - 1                           # labels at both ends
            z[1, 0] = 30.25                                 # sure and right: softplus(-30) ~ 7e-14
            z[2, C - 1] = -29.5                             # sure and wrong at the label
            z[3, 0] = 31.0                                  # sure and wrong off the label (when y[3] != 0)
            z[4, C - 1] = -30.75
        sets.append((z, y.astype(np.int64), (float(focal), alpha, gamma, scale)))
    return sets


def main():
    sys.path.insert(0, os.path.join(REF, "training"))
    import loss_utils
    assert loss_utils.__file__.startswith(REF)
    out = {}
    sets = make_sets()
    out["n_sets"] = np.array(len(sets))
    for s, (z, y, params) in enumerate(sets):
        focal, alpha, gamma, scale = params
        logits = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        per = loss_utils.sigmoid_focal_loss(alpha=alpha, gamma=gamma, use_focal=bool(focal), scale=scale)(logits, torch.tensor(y))
        loss = per.mean()
        loss.backward()
        out[f"logits_{s}"], out[f"labels_{s}"], out[f"params_{s}"] = z, y, np.array(params)
        out[f"per_sample_{s}"], out[f"loss_{s}"], out[f"dlogits_{s}"] = per.detach().numpy(), loss.detach().numpy(), logits.grad.numpy()
        print("set", s, z.shape, params, "loss", float(loss.detach()))
    path = os.path.join(REPO, "tests", "golden", "aux_loss_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
