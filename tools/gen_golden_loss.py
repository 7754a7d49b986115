#!/usr/bin/env python
"""Generate tests/golden/loss_ref.npz: the REFERENCE's training criterion on a handful of (logits, labels) sets.

Runs only where /root/reference exists (never on the GPU box), like tools/gen_golden_views.py.  It imports the reference's
``training/loss_utils.py`` and evaluates, in fp64 under torch autograd, exactly what training/train.py:446-452 does:
``torch.nn.CrossEntropyLoss(reduction='none')`` per sample, times ``categorical_ordinal_focal_weight(...)`` when the set is
weighted, then ``.mean()``; ``loss.backward()`` gives dlogits.  Nothing of the criterion is restated here.

The file holds data only.  Per set s: logits_s [B, C] float64, labels_s [B] int64, params_s = (weighted, alpha, gamma, beta,
scale), per_sample_s, weight_s, loss_s, dlogits_s.  The sets cover C = 3, 4, 400 and B = 1, 7, a row whose two largest logits
are exactly equal, a row with p_label within 1e-6 of 1, a row whose label is C - 1 away from the argmax, beta = 0 and 0.2,
and one unweighted set.

    python tools/gen_golden_loss.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True


def make_sets():
    rng = np.random.default_rng(4711)
    sets = []
    for s, (B, C, weighted, beta) in enumerate([(7, 3, 1, 0.2), (7, 3, 1, 0.0), (1, 3, 1, 0.2), (7, 4, 1, 0.2), (7, 400, 1, 0.2),
                                                 (1, 400, 1, 0.0), (7, 4, 0, 0.0), (7, 3, 1, 0.2)]):
        z = rng.standard_normal((B, C)) * 3.0
        y = rng.integers(0, C, B)
        if B == 7:
            z[0, 1] = z[0, 2] = z[0].max() + 0.5            # exact tie of the two largest: argmax is class 1
            y[0] = 2
            z[1, :] = -8.0 + rng.standard_normal(C) * 0.1   # p_label within 1e-6 of 1
            z[1, 0] = 12.0 if C < 100 else 16.0
            y[1] = 0
            z[2, C - 1] = z[2].max() + 2.0                  # label at ordinal distance C - 1 from the argmax
            y[2] = 0
        gamma, alpha, scale = (2.0, 0.25, 1.0) if s != 7 else (1.0, 0.5, 3.0)
        sets.append((z, y.astype(np.int64), (float(weighted), alpha, gamma, beta, scale)))
    return sets


def main():
    sys.path.insert(0, os.path.join(REF, "training"))
    import loss_utils
    assert loss_utils.__file__.startswith(REF)
    out = {}
    sets = make_sets()
    out["n_sets"] = np.array(len(sets))
    for s, (z, y, params) in enumerate(sets):
        weighted, alpha, gamma, beta, scale = params
        logits = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        labels = torch.tensor(y)
        loss = torch.nn.CrossEntropyLoss(reduction='none')(logits, labels)
        weights = torch.ones_like(loss)
        if weighted:
            weights = loss_utils.categorical_ordinal_focal_weight(gamma=gamma, alpha=alpha, beta=beta, scale=scale)(logits, labels)
            loss = loss * weights
        per = loss.detach().clone()
        loss = loss.mean()
        loss.backward()
        p = logits.detach().softmax(-1)
        if z.shape[0] == 7:
            top = torch.sort(logits.detach()[0]).values
            assert top[-1] == top[-2] and float(1 - p[1, y[1]]) < 1e-6 and abs(int(y[2]) - int(p[2].argmax())) == z.shape[1] - 1
        out[f"logits_{s}"], out[f"labels_{s}"], out[f"params_{s}"] = z, y, np.array(params)
        out[f"per_sample_{s}"], out[f"weight_{s}"] = per.numpy(), weights.detach().numpy().astype(np.float64)
        out[f"loss_{s}"], out[f"dlogits_{s}"] = loss.detach().numpy(), logits.grad.numpy()
        print("set", s, z.shape, params, "loss", float(loss.detach()))
    path = os.path.join(REPO, "tests", "golden", "loss_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
