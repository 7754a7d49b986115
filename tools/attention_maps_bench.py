#!/usr/bin/env python
"""What VitaCLIP.attention_maps costs, at BASELINE config c2's shape (ViT-B/16, T = 8, 224 px) for B = 8 and B = 64 (a batch that
does not fit is halved).  One process, alternating rounds - every round runs each variant once, the figure is the median over
the rounds (host clock around work that ends in a device synchronisation):

    kept_forward        encode_video(x, kept=...) alone: the activation-keeping forward every map starts from, the yardstick
    rollout             attention_maps(x, mode="rollout"): that forward + one gava_attention_mass per block + the head
    cls                 attention_maps(x, mode="cls", layer=-1, heads=None)

and gava_attention_mass on its own per form on the model's operands (the qkv rows of a block, 214 keys): the median time of
--kernel-reps launches between device events.  The cost is reported against the kept forward of the same process; nothing is
gated.  Writes profiles/attention_maps_bench.json.

    python tools/attention_maps_bench.py [--batches 8 64] [--rounds 7] [--warmup 2] [--kernel-reps 20]"""
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
from gava_clip_amd import VitaCLIP, hip, synth, training  # noqa: E402
from gava_clip_amd.config import VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def model_times(m, x, rounds, warmup):
    B, T = x.shape[0], x.shape[2]
    kept = training.alloc_kept(m, B, T, x.device)

    def kept_forward():
        with torch.no_grad():
            m.encode_video(x, kept=kept)

    variants = {"kept_forward": kept_forward,
                "rollout": lambda: m.attention_maps(x, mode="rollout"),
                "cls": lambda: m.attention_maps(x, mode="cls", layer=-1, heads=None)}
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():
            ms = timed(fn)
            if r >= warmup:
                times[k].append(ms)
    res = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
    base = res["kept_forward"]["median_ms"]
    for k in ("rollout", "cls"):
        res[k]["over_kept_forward_ms"] = round(res[k]["median_ms"] - base, 3)
        res[k]["over_kept_forward_pct"] = round(100 * (res[k]["median_ms"] - base) / base, 1)
    return res


def kernel_times(B, cfg, prec, reps):
    T, D, H, G = cfg.num_frames, cfg.feature_dim, cfg.num_heads, cfg.num_global_prompts
    n1 = (cfg.input_size // cfg.patch_size) ** 2 + 1
    BT = B * T
    dt = hip.h16_dtype(prec)
    qkv = (torch.randn(BT * n1, 3 * D, device="cuda") * 0.5).to(dt)
    qkv[:, :D] *= 0.125
    side = (torch.randn(G + 2 * BT, 2 * D, device="cuda") * 0.5).to(dt)
    last_q = qkv.view(BT, n1, 3 * D)[:, 0, :D].contiguous()
    w = torch.rand(BT, n1, device="cuda").softmax(-1).contiguous()
    common = dict(k=qkv[:, D:2 * D], batch=BT, heads=H, n_kmain=n1, prec=prec, side_k=side[:, :D], n_g=G, T=T, has_summary=True)
    forms = {"cls_row (n_q = 1, all keys)": lambda: hip.attention_mass(last_q, n_q=1, q_batch_rows=1, **common),
             "cls_row_renorm (n_q = 1)": lambda: hip.attention_mass(last_q, n_q=1, q_batch_rows=1, renorm=True, **common),
             "chain_step (n_q = n, w, renorm)": lambda: hip.attention_mass(qkv[:, :D], n_q=n1, w=w, renorm=True, **common),
             "mass (n_q = n, all keys)": lambda: hip.attention_mass(qkv[:, :D], n_q=n1, **common)}
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_maps_bench needs the GPU: nothing here is measured without one")
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
        out["batches"][str(asked)] = dict(B=B, model=res, attention_mass=kernel_times(B, cfg, m.prec, args.kernel_reps))
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "attention_maps_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
