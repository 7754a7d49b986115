#!/usr/bin/env python
"""What VitaCLIP.integrated_gradients and smooth_grad cost, at BASELINE config c2's shape (ViT-B/16, T = 8, 224 px) for B = 4 clips
and m = 16 copies.  One process, alternating rounds - every round runs each variant once, the figure is the median over the rounds
(host clock around work that ends in a device synchronisation):

    integrated_gradients    integrated_gradients(x, target, steps=m) as a whole (reduce="sum", the completeness residual included)
    smooth_grad             smooth_grad(x, target, samples=m) as a whole (the plain forward of x and gava_clip_range included)
    saliency_torch_ig       what the library could do before: the B*m interpolants from torch ops, ONE saliency(reduce=None) call on
                            them (B*m full-size fp32 gradients in memory), and the torch reduction (x - x0) * sum_k w_k g_k, summed over channels
    saliency_torch_sg       the same for SmoothGrad: torch.randn noise, the same saliency call, mean and absmax in torch

and the helper kernels on their own, the median time of --kernel-reps launches between device events, with the bytes they move and the
HBM bandwidth that makes: gava_path_clips (line and noise), gava_clip_range, gava_unpatchify_path (GRAD, ATTR_SUM; next to
gava_unpatchify on the same B*m frames), gava_path_delta.  Nothing is gated.  Writes profiles/path_grad_bench.json.

    python tools/path_grad_bench.py [--batch 4] [--m 16] [--rounds 5] [--warmup 2] [--kernel-reps 20]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("path_grad_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    model = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    model.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    model = model.cuda().eval()
    B, m, T, S, P = args.batch, args.m, cfg.num_frames, cfg.input_size, cfg.patch_size
    x = torch.from_numpy(synth.synth_clip(B, T, S, seed=21)).cuda()
    target = torch.arange(B, device="cuda") % 3
    alpha, w = hip.path_rule("trapezoid", m)
    a_t = torch.tensor(alpha, dtype=torch.float32, device="cuda").view(1, m, 1, 1, 1, 1)
    w_t = torch.tensor(w, dtype=torch.float32, device="cuda").view(1, m, 1, 1, 1, 1)
    tgt_m = target.repeat_interleave(m)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def saliency_torch_ig():
        pts = (a_t * x.unsqueeze(1)).view(B * m, 3, T, S, S)
        g = model.saliency(pts, target=tgt_m, reduce=None)[0].view(B, m, 3, T, S, S)
        return (x * (w_t * g).sum(1)).sum(1)

    def saliency_torch_sg():
        flat = x.view(B, -1)
        sigma = 0.15 * (flat.amax(1) - flat.amin(1))
        noisy = (x.unsqueeze(1) + sigma.view(B, 1, 1, 1, 1, 1) * torch.randn(B, m, 3, T, S, S, generator=gen, device="cuda")).view(B * m, 3, T, S, S)
        g = model.saliency(noisy, target=tgt_m, reduce=None)[0].view(B, m, 3, T, S, S)
        return g.mean(1).abs().amax(1)

    with torch.no_grad():
        variants = {"integrated_gradients": lambda: model.integrated_gradients(x, target=target, steps=m, max_clips=B * m),
                    "smooth_grad": lambda: model.smooth_grad(x, target=target, samples=m, max_clips=B * m),
                    "saliency_torch_ig": saliency_torch_ig,
                    "saliency_torch_sg": saliency_torch_sg}
        times, peak = {k: [] for k in variants}, {}
        for r in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms = timed(fn)
                peak[k] = torch.cuda.max_memory_allocated() - base
                if r >= args.warmup:
                    times[k].append(ms)
    calls = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                     peak_extra_mib=round(peak[k] / 2 ** 20, 1)) for k, v in times.items()}
    # the helper kernels alone
    g, n1 = S // P, (S // P) ** 2 + 1
    clip_bytes = 3 * T * S * S * 4
    copies = torch.empty(B, m, 3, T, S, S, device="cuda")
    sigma = hip.clip_range(x, 0.15)[2]
    dpatch = torch.randn(B * m * T * n1, 3 * P * P, device="cuda")
    full, one = torch.empty(B, 3, T, S, S, device="cuda"), torch.empty(B, T, S, S, device="cuda")
    every = torch.empty(B * m, 3, T, S, S, device="cuda")
    logits = torch.randn(B * m, 3, device="cuda")
    geo = dict(T=T, size=S, patch=P, frame_rows=n1, row_offset=1)
    rows_bytes = B * m * T * g * g * 3 * P * P * 4          # the patch rows a fold reads
    kernels = {
        "path_clips line": (lambda: hip.path_clips(x, patch=P, alpha=alpha, out=copies), (1 + m) * B * clip_bytes),
        "path_clips noise": (lambda: hip.path_clips(x, patch=P, sigma=sigma, samples=m, out=copies), (1 + m) * B * clip_bytes),
        "clip_range": (lambda: hip.clip_range(x, 0.15), B * clip_bytes),
        "unpatchify_path GRAD": (lambda: hip.unpatchify_path(dpatch, full, B=B, mode=hip.PATH_GRAD, w=w, **geo), rows_bytes + B * clip_bytes),
        "unpatchify_path ATTR_SUM": (lambda: hip.unpatchify_path(dpatch, one, B=B, mode=hip.PATH_ATTR_SUM, w=w, x=x, **geo),
                                     rows_bytes + B * clip_bytes + B * clip_bytes // 3),
        "unpatchify GRAD of the B*m clips": (lambda: hip.unpatchify(dpatch, every, B=B * m, mode=hip.UNPATCH_GRAD, **geo), 2 * rows_bytes),
        "path_delta": (lambda: hip.path_delta(one, logits, target, m=m, k_lo=0, k_hi=m - 1), B * clip_bytes // 3),
    }
    kern = {}
    for k, (fn, moved) in kernels.items():
        kern[k] = event_us(fn, args.kernel_reps)
        kern[k].update(bytes=moved, gb_per_s=round(moved / kern[k]["median_us"] / 1e3, 1))
    out = dict(device=torch.cuda.get_device_name(0), config="VIT_B16_T8", B=B, m=m, T=T, rounds=args.rounds, calls=calls, kernels=kern,
               ig_over_saliency_torch=round(calls["integrated_gradients"]["median_ms"] / calls["saliency_torch_ig"]["median_ms"], 3),
               sg_over_saliency_torch=round(calls["smooth_grad"]["median_ms"] / calls["saliency_torch_sg"]["median_ms"], 3))
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "path_grad_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
