#!/usr/bin/env python
"""Generate tests/golden/soft_loss_ref.npz: the REFERENCE's criterion on targets of the logits' shape (soft / mixed labels).

Runs only where the reference checkout exists (never on the GPU box), like tools/gen_golden_loss.py.  It imports the
reference's ``training/loss_utils.py`` and evaluates, in fp64 under torch autograd, what training/train.py:446-452 does when
the labels are not integers: ``torch.nn.CrossEntropyLoss(reduction='none')`` with class probabilities per sample, times
``categorical_ordinal_focal_weight(...)`` (whose y_true then has the logits' shape, loss_utils.py:32-44) when the set is
weighted, then ``.mean()``; ``loss.backward()`` gives dlogits.  Nothing of the criterion is restated here.

The file holds data only.  Per set s: logits_s [B, C] float64, targets_s [B, C] float64, params_s = (weighted, alpha, gamma,
beta, scale), per_sample_s, weight_s, loss_s, dlogits_s.  The sets cover C = 3, 4, 65 and B = 1, 3, 5, 7; rows with one-hot
targets, smoothed and mixed targets, targets that do not sum to 1, two equal largest targets, an all-zero target row, two
equal largest logits and a confident row; beta = 0 and 0.2, gamma = 1 and 2, and one unweighted set.

    python tools/gen_golden_soft_loss.py <path of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAVA_REFERENCE", "")
sys.dont_write_bytecode = True


def make_sets():
    rng = np.random.default_rng(1207)
    sets = []
    for s, (B, C, weighted, alpha, gamma, beta, scale) in enumerate([(5, 4, 1, 0.25, 2.0, 0.2, 1.0), (7, 3, 1, 0.25, 2.0, 0.2, 1.0),
                                                                     (3, 65, 1, 0.25, 2.0, 0.2, 1.0), (7, 3, 1, 0.5, 1.0, 0.0, 3.0),
                                                                     (5, 4, 0, 0.25, 2.0, 0.0, 1.0), (1, 3, 1, 0.25, 2.0, 0.2, 1.0)]):
        z = rng.standard_normal((B, C)) * 3.0
        ya, yb = rng.integers(0, C, B), rng.integers(0, C, B)
        lam = rng.beta(0.8, 0.8, B)
        eps = 0.1
        t = np.full((B, C), eps / C)
        for i in range(B):                                          # smoothed, mixed targets
            t[i, ya[i]] += lam[i] * (1 - eps)
            t[i, yb[i]] += (1 - lam[i]) * (1 - eps)
        t[0] = 0.0
        t[0, ya[0]] = 1.0                                           # one-hot
        if B >= 3:
            t[1] *= 1.7                                             # does not sum to 1
            t[2] = 0.0
            t[2, 0] = t[2, C - 1] = 0.5                             # two equal largest targets: class 0 is the target's argmax
            z[2, C - 1] = z[2].max() + 2.0                          # ... at ordinal distance C - 1 from the logits' argmax
        if B >= 5:
            z[3, 1] = z[3, 2] = z[3].max() + 0.5                    # two equal largest logits: class 1 is the argmax
            t[4] = 0.0                                              # all-zero targets: no loss, no gradient
        if B >= 7:
            z[5, :] = -8.0 + rng.standard_normal(C) * 0.1           # a confident row
            z[5, 0] = 12.0
        sets.append((z, t, (float(weighted), alpha, gamma, beta, scale)))
    return sets


def main():
    if not os.path.isfile(os.path.join(REF, "training", "loss_utils.py")):
        raise SystemExit("usage: gen_golden_soft_loss.py <path of the reference checkout>   (or GAVA_REFERENCE)")
    sys.path.insert(0, os.path.join(REF, "training"))
    import loss_utils
    assert os.path.abspath(loss_utils.__file__).startswith(os.path.abspath(REF))
    out = {}
    sets = make_sets()
    out["n_sets"] = np.array(len(sets))
    for s, (z, t, params) in enumerate(sets):
        weighted, alpha, gamma, beta, scale = params
        logits = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        targets = torch.tensor(t, dtype=torch.float64)
        loss = torch.nn.CrossEntropyLoss(reduction='none')(logits, targets)
        weights = torch.ones_like(loss)
        if weighted:
            weights = loss_utils.categorical_ordinal_focal_weight(gamma=gamma, alpha=alpha, beta=beta, scale=scale)(logits, targets)
            loss = loss * weights
        per = loss.detach().clone()
        loss = loss.mean()
        loss.backward()
        out[f"logits_{s}"], out[f"targets_{s}"], out[f"params_{s}"] = z, t, np.array(params)
        out[f"per_sample_{s}"], out[f"weight_{s}"] = per.numpy(), weights.detach().numpy().astype(np.float64)
        out[f"loss_{s}"], out[f"dlogits_{s}"] = loss.detach().numpy(), logits.grad.numpy()
        print("set", s, z.shape, params, "loss", float(loss.detach()))
    path = os.path.join(REPO, "tests", "golden", "soft_loss_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
