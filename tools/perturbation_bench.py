#!/usr/bin/env python
"""What VitaCLIP.perturbation_curves costs, at BASELINE config c2's shape (ViT-B/16, T = 8, 224 px) for a small B and the default
eleven steps.  One process, alternating rounds - every round runs each variant once, the figure is the median over the rounds
(host clock around work that ends in a device synchronisation):

    curves              perturbation_curves(x, scores, mode="deletion") as a whole
    forwards            the plain forward of the same B * S1 perturbed clips alone (built once, outside the clock)
    torch_build         the same perturbed clips from torch ops: the ranks' mask upsampled to pixels, torch.where per step

and the helper kernels on their own, the median time of --kernel-reps launches between device events: gava_patch_ranks (patch
and pixel layout), gava_blur_clips (sigma = 5), gava_perturb_clips (zero and tensor baseline), gava_perturb_scores.  Nothing is
gated.  Writes profiles/perturbation_bench.json.

    python tools/perturbation_bench.py [--batch 4] [--steps 10] [--rounds 7] [--warmup 2] [--kernel-reps 20]"""
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


def event_us(run, reps):
    run()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_us=round(statistics.median(ms) * 1e3, 1), min_us=round(min(ms) * 1e3, 1))


def torch_build(x, ranks, ks, g, P):
    """The deletion clips from torch ops alone -> [B, S1, 3, T, S, S]."""
    B, _, T, S, _ = x.shape
    r = ranks.view(B, 1, T, g, g).repeat_interleave(P, 3).repeat_interleave(P, 4)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    return torch.stack([torch.where(r < k, zero, x) for k in ks], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perturbation_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    m = m.cuda().eval()
    B, T, S, P = args.batch, cfg.num_frames, cfg.input_size, cfg.patch_size
    g, S1 = S // P, args.steps + 1
    x = torch.from_numpy(synth.synth_clip(B, T, S, seed=21)).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    scores = torch.rand(B, T, g, g, generator=gen, device="cuda")
    pixels = torch.rand(B, T, S, S, generator=gen, device="cuda")
    fr, ks = hip.perturb_thresholds(T * g * g, args.steps)
    ranks = hip.patch_ranks(scores)
    blurred = hip.blur_clips(x, hip.gaussian_taps(5.0))
    xp = hip.perturb_clips(x, ranks, ks, patch=P, mode="deletion")
    assert torch.equal(torch_build(x, ranks, ks, g, P), xp)
    flat = xp.view(B * S1, 3, T, S, S)
    with torch.no_grad():
        logits = m(flat)[0]
        variants = {"curves": lambda: m.perturbation_curves(x, scores, mode="deletion", steps=args.steps),
                    "forwards": lambda: m(flat),
                    "torch_build": lambda: torch_build(x, ranks, ks, g, P)}
        times = {k: [] for k in variants}
        for r in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                ms = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
    model = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
    taps = hip.gaussian_taps(5.0).cuda()
    tmp = torch.empty_like(x)
    kernels = {"patch_ranks (patch layout, n = %d)" % (T * g * g): lambda: hip.patch_ranks(scores),
               "patch_ranks (pixel layout)": lambda: hip.patch_ranks(pixels, patch=P),
               "blur_clips (sigma = 5, r = 15)": lambda: hip.blur_clips(x, taps, out=tmp),
               "perturb_clips (zero baseline)": lambda: hip.perturb_clips(x, ranks, ks, patch=P, mode="deletion", out=xp),
               "perturb_clips (tensor baseline)": lambda: hip.perturb_clips(x, ranks, ks, patch=P, mode="insertion", baseline=blurred, out=xp),
               "perturb_scores": lambda: hip.perturb_scores(logits, fr, ref_step=0)}
    kern = {k: event_us(fn, args.kernel_reps) for k, fn in kernels.items()}
    moved = (1 + S1) * x.numel() * 4
    pc = kern["perturb_clips (zero baseline)"]["median_us"]
    helpers_us = kern["patch_ranks (patch layout, n = %d)" % (T * g * g)]["median_us"] + pc + kern["perturb_scores"]["median_us"]
    out = dict(device=torch.cuda.get_device_name(0), config="VIT_B16_T8", B=B, T=T, S1=S1, rounds=args.rounds, model=model, kernels=kern,
               perturb_clips_bytes=moved, perturb_clips_gb_per_s=round(moved / pc / 1e3, 1),
               helpers_us=round(helpers_us, 1), helpers_pct_of_curves=round(100 * helpers_us / (model["curves"]["median_ms"] * 1e3), 3),
               curves_over_forwards_ms=round(model["curves"]["median_ms"] - model["forwards"]["median_ms"], 3),
               torch_build_over_perturb_clips=round(model["torch_build"]["median_ms"] * 1e3 / pc, 2))
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "perturbation_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
