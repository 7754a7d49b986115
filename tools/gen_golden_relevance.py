#!/usr/bin/env python
"""Generate tests/golden/tiny_relevance.npz and tests/golden/c1_relevance.npz: the REFERENCE's own gradient-weighted attention
relevance (Chefer et al., "Generic Attention-model Explainability", the self-attention rule).

Runs only in the build container, where the reference checkout is (tools/gen_golden.py's REF), like
tools/gen_golden_attention_maps.py.  It builds the reference's ``VitaCLIP`` with the synthetic weights (tools/gen_golden.py's
builders) at two shapes,
    tiny   TINY, x = synth_clip(2, 4, 64, seed=1234)                       (the model and clip of tiny.npz)
    c1     ViT-B/16, T = 8, 12 blocks, x = synth_clip(2, 8, 224, seed=1234) (the model and clip of c1_b16.npz),
and runs the reference itself, in eval mode, with hooks only: forward hooks on every block's ``attn.q_proj`` / ``k_proj`` /
``v_proj`` read the projected queries, keys and values, a forward pre-hook on ``attn.out_proj`` reads its input and puts a
tensor hook on it that captures the gradient dO.  ``backward()`` runs on  s = sum_b logits[b, target_b]  with the target the
reference's own top-1.  Nothing of the model is restated here.  From what the hooks took (fp32, as the reference produced it),
in fp64 and per head:
    A = softmax(q / sqrt(64) . k) over all keys,   grad A = dO . v^T,   A-_l = mean_h max(0, A * grad A) on (cls, patches),
    relevance = row 0 of (I + A-_L) ... (I + A-_1), by the matrix products.
The reference orders a block's tokens (cls, local prompts, global prompts, patches, summary); the fixtures use this project's
order (cls, patches).  The files hold data only, a few KB each:
    logits    [2, 3]      the reference's logits of the same forward
    target    [2]         int64, their argmax
    relevance [B*T, n]    float32 (the values were formed in fp64)

    python tools/gen_golden_relevance.py
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
from gava_clip_amd.config import TINY, VIT_B16_T8  # noqa: E402


def run(mod, cfg, name, xseed):
    model = gg.build_reference(mod, cfg, os.path.join(gg.CLASSES, "updrs_3cls_classes.txt"))
    gg.load_synth(model, cfg, 3)
    model.eval()
    taken, hooks = {}, []
    for i, blk in enumerate(model.visual.blocks):
        for nm in ("q_proj", "k_proj", "v_proj"):
            hooks.append(getattr(blk.attn, nm).register_forward_hook(
                lambda m, inp, out, key=(i, nm): taken.__setitem__(key, out.detach().double())))

        def pre(m, inp, i=i):
            inp[0].register_hook(lambda g, i=i: taken.__setitem__((i, "dO"), g.detach().double()))
        hooks.append(blk.attn.out_proj.register_forward_pre_hook(pre))
    x = torch.from_numpy(synth.synth_clip(2, cfg.num_frames, cfg.input_size, seed=xseed)).requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits = model(x)[0]
    target = logits.detach().argmax(1)
    logits.gather(1, target.view(-1, 1)).sum().backward()
    for h in hooks:
        h.remove()
    L, H, T, G = cfg.num_layers, cfg.num_heads, cfg.num_frames, cfg.num_global_prompts
    n = (cfg.input_size // cfg.patch_size) ** 2 + 1
    own = [0] + list(range(1 + T + G, T + G + n))            # reference order (cls, local T, global G, patches, summary)
    eye = torch.eye(n, dtype=torch.float64)
    M = None
    for i in range(L):
        q, k, v, dO = (taken[(i, nm)] for nm in ("q_proj", "k_proj", "v_proj", "dO"))
        BT, Lt, D = q.shape
        assert Lt == n + G + T + 1 and k.shape == v.shape == q.shape and dO.shape == q.shape
        dh = D // H
        heads = lambda t: t.view(BT, Lt, H, dh)
        A = torch.einsum("nqhc,nkhc->nhqk", heads(q) / dh ** 0.5, heads(k)).softmax(-1)
        dA = torch.einsum("nqhc,nkhc->nhqk", heads(dO), heads(v))
        Abar = (A * dA).clamp(min=0)[:, :, own][:, :, :, own].mean(1)
        M = (eye + Abar) if M is None else (eye + Abar) @ M
    rel = M[:, 0]
    assert rel.shape == (2 * T, n) and bool(torch.isfinite(rel).all()) and bool((rel[:, 0] >= 1).all()) and bool((rel >= 0).all())
    path = os.path.join(gg.REPO, "tests", "golden", f"{name}_relevance.npz")
    np.savez_compressed(path, logits=logits.detach().numpy(), target=target.numpy(), relevance=rel.float().numpy())
    print("wrote", path, os.path.getsize(path), "bytes; patch relevance per frame:", rel[:, 1:].sum(-1).tolist())


def main():
    torch.set_num_threads(8)
    mod, _ = gg.import_reference()
    assert mod.__file__.startswith(gg.REF)
    run(mod, TINY, "tiny", 1234)
    run(mod, VIT_B16_T8, "c1", 1234)


if __name__ == "__main__":
    main()
