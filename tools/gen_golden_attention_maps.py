#!/usr/bin/env python
"""Generate tests/golden/tiny_attention_maps.npz: the REFERENCE's own attention probabilities and their rollout.

Runs only in the build container, where the reference checkout is (tools/gen_golden.py's REF), like
tools/gen_golden_input_grad.py.  It builds the reference's ``VitaCLIP`` at the TINY shape with the synthetic weights
(tools/gen_golden.py's builders), feeds it ``x = synth_clip(2, 4, 64)`` in eval mode and reads, through forward hooks on
every block's ``attn.q_proj`` / ``attn.k_proj``, the projected queries and keys the block's softmax sees.  From those (fp32,
as the reference produced them) the probabilities are formed in fp64 exactly as Attention.forward does - q / sqrt(64) . k,
softmax over the keys, per head.  Nothing of the model is restated here.

The reference orders a block's tokens (cls, local prompts, global prompts, patches, summary); the fixture uses this
project's order (cls, patches | global | local | summary).  The file holds data only, a few KB:
    logits    [2, 3]               the reference's logits of the same forward
    cls       [L, B*T, H, n_all]   the CLS row of every block and head over all its keys, float32
    rollout   [B*T, n]             row 0 of A^_L ... A^_1, A^_l = (I + mean_h A_l,h) / 2 with A_l,h restricted to (cls, patches)
                                   and renormalised per row - by the matrix products, in fp64, stored float32

    python tools/gen_golden_attention_maps.py
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

from gava_clip_amd import synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402


def main():
    torch.set_num_threads(8)
    cfg = TINY
    mod, _ = gg.import_reference()
    assert mod.__file__.startswith(gg.REF)
    model = gg.build_reference(mod, cfg, os.path.join(gg.CLASSES, "updrs_3cls_classes.txt"))
    gg.load_synth(model, cfg, 3)
    model.eval()
    taken = {}
    hooks = []
    for i, blk in enumerate(model.visual.blocks):
        for name in ("q_proj", "k_proj"):
            hooks.append(getattr(blk.attn, name).register_forward_hook(
                lambda m, inp, out, key=(i, name): taken.__setitem__(key, out.detach().double())))
    x = torch.from_numpy(synth.synth_clip(2, cfg.num_frames, cfg.input_size))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits = model(x)[0]
    for h in hooks:
        h.remove()
    L, H, T, G = cfg.num_layers, cfg.num_heads, cfg.num_frames, cfg.num_global_prompts
    n = (cfg.input_size // cfg.patch_size) ** 2 + 1
    n_all = n + G + T + 1
    # reference order (cls, local T, global G, patches, summary) -> (cls, patches, global, local, summary)
    order = [0] + list(range(1 + T + G, T + G + n)) + list(range(1 + T, 1 + T + G)) + list(range(1, 1 + T)) + [n_all - 1]
    assert sorted(order) == list(range(n_all))
    cls, A = [], []
    for i in range(L):
        q, k = taken[(i, "q_proj")], taken[(i, "k_proj")]
        BT, Lt, D = q.shape
        assert Lt == n_all and k.shape == q.shape
        dh = D // H
        qh, kh = q.view(BT, Lt, H, dh), k.view(BT, Lt, H, dh)
        aff = torch.einsum("nqhc,nkhc->nhqk", qh / dh ** 0.5, kh)[:, :, order][:, :, :, order]
        cls.append(aff[:, :, 0].softmax(-1))
        A.append(aff[:, :, :n, :n].softmax(-1).mean(1))          # restricted to the frame's own tokens, renormalised; head mean
    eye = torch.eye(n, dtype=torch.float64)
    M = eye.expand(A[0].shape[0], n, n)
    for a in A:
        M = (0.5 * (eye + a)) @ M
    rollout = M[:, 0]
    assert float((rollout.sum(-1) - 1).abs().max()) < 1e-12
    path = os.path.join(gg.REPO, "tests", "golden", "tiny_attention_maps.npz")
    np.savez_compressed(path, logits=logits.numpy(), cls=torch.stack(cls).float().numpy(), rollout=rollout.float().numpy())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
