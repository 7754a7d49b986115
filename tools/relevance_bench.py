#!/usr/bin/env python
"""What VitaCLIP.relevance_maps costs, at BASELINE config c2's shape (ViT-B/16, T = 8, 224 px) for B = 8 and B = 64 (a batch that
does not fit is halved until it does; the B that ran is recorded).  In ONE process, alternating the variants round by round
after a warm-up (the measuring guide's A/B recipe), each call timed between device synchronisations:

    saliency            saliency(x, target, reduce="absmax"): the grad-enabled forward, the whole vision backward, the fold
    relevance           relevance_maps(x, target): the same forward, the backward up to block 0's d mix, one
                        gava_attention_relevance per block

and gava_attention_relevance on its own per form on the model's shapes (the qkv rows of a block, 214 keys, fp16 activations under
bf16 gradients as on the kept route), next to gava_attention_mass's chain step for scale: the median time of `--kernel-reps`
launches between events.  Nothing here is gated.  Writes profiles/relevance_bench.json.

    python tools/relevance_bench.py [--batches 8 64] [--rounds 7] [--warmup 2] [--kernel-reps 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from gava_clip_amd import VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def model_times(m, x, rounds, warmup):
    target = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    variants = {"saliency": lambda: m.saliency(x, target=target, reduce="absmax"),
                "relevance": lambda: m.relevance_maps(x, target=target)}
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():
            ms = timed(fn)
            if r >= warmup:
                times[k].append(ms)
    res = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
    res["relevance"]["over_saliency_pct"] = round(100 * (res["relevance"]["median_ms"] / res["saliency"]["median_ms"] - 1), 1)
    return res


def kernel_times(B, cfg, act, reps):
    T, D, H, G = cfg.num_frames, cfg.feature_dim, cfg.num_heads, cfg.num_global_prompts
    n1 = (cfg.input_size // cfg.patch_size) ** 2 + 1
    BT = B * T
    dt = hip.h16_dtype(act)
    qkv = (torch.randn(BT * n1, 3 * D, device="cuda") * 0.5).to(dt)
    qkv[:, :D] *= 0.125
    side = (torch.randn(G + 2 * BT, 2 * D, device="cuda") * 0.5).to(dt)
    dmix = torch.randn(BT * n1, D, device="cuda").bfloat16()
    last_q = qkv.view(BT, n1, 3 * D)[:, 0, :D].contiguous()
    last_d = dmix.view(BT, n1, D)[:, 0].contiguous()
    w = torch.rand(BT, n1, device="cuda").contiguous()
    keys = dict(batch=BT, heads=H, n_kmain=n1, side_k=side[:, :D], n_g=G, T=T, has_summary=True)
    rel = dict(k=qkv[:, D:2 * D], v=qkv[:, 2 * D:], prec=hip.PREC_BF16, act_prec=act, **keys)
    forms = {"relevance cls step (n_q = 1)": lambda: hip.attention_relevance(last_q, dout=last_d, n_q=1, q_batch_rows=1, **rel),
             "relevance chain step (n_q = n, w)": lambda: hip.attention_relevance(qkv[:, :D], dout=dmix, n_q=n1, w=w, **rel),
             "mass chain step (n_q = n, w, renorm)": lambda: hip.attention_mass(qkv[:, :D], qkv[:, D:2 * D], n_q=n1, w=w, renorm=True, prec=act, **keys)}
    out = {}
    for name, run in forms.items():
        run()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name] = dict(median_us=round(statistics.median(ms) * 1e3, 1), min_us=round(min(ms) * 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relevance_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relevance_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    m = m.cuda().eval()
    out = dict(device=torch.cuda.get_device_name(0), config="VIT_B16_T8", T=cfg.num_frames, rounds=args.rounds, batches={})
    for B in args.batches:
        asked = B
        while True:
            try:
                x = torch.from_numpy(synth.synth_clip(B, cfg.num_frames, cfg.input_size, seed=21)).cuda()
                res = model_times(m, x, args.rounds, args.warmup)
                break
            except torch.OutOfMemoryError:
                if B == 1:
                    raise
                B //= 2
                torch.cuda.empty_cache()
        out["batches"][str(asked)] = dict(B=B, model=res, kernels=kernel_times(B, cfg, m.prec, args.kernel_reps))
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
