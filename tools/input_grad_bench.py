#!/usr/bin/env python
"""What the gradient with respect to the input clip costs, at BASELINE config c2's training shape (ViT-B/16, B = 64, T = 8, 224 px;
the batch is halved until it fits).  One process, alternating rounds - every round runs each variant once, the figure is the
median over the rounds:

    backward            loss.backward() with x.requires_grad = False: the parent's behaviour, the baseline
    backward_dx         loss.backward() with x.requires_grad = True (the dgrad GEMM through the patch projection + gava_unpatchify)
    saliency_absmax     model.saliency(x, target, reduce="absmax") as a whole call: forward, head, backward, the map
    saliency_grad       model.saliency(x, target, reduce=None): the same with the full-size gradient

(host clock around work that ends in a device synchronisation; the forward of the two backward variants is outside the window),
and gava_unpatchify on its own per mode on the model's operand (rows of 3 P^2 floats behind each frame's CLS row): the
median time of --kernel-reps launches between device events, and the bytes the pass has to move, computed from the shapes.
Writes profiles/input_grad_bench.json.

    python tools/input_grad_bench.py [--batch 64] [--rounds 7] [--warmup 2] [--kernel-reps 20]"""
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
    B = x.shape[0]
    w = torch.randn(B, 3, generator=torch.Generator().manual_seed(4)).cuda()
    target = torch.arange(B, device="cuda") % 3

    def backward(want_dx):
        for p in m.parameters():
            p.grad = None
        xin = x.detach().requires_grad_(want_dx)
        loss = (m(xin)[0] * w).sum()
        return timed(loss.backward)

    variants = {"backward": lambda: backward(False), "backward_dx": lambda: backward(True),
                "saliency_absmax": lambda: timed(lambda: m.saliency(x, target=target, reduce="absmax")),
                "saliency_grad": lambda: timed(lambda: m.saliency(x, target=target, reduce=None))}
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():
            ms = fn()
            if r >= warmup:
                times[k].append(ms)
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}


def kernel_times(B, T, size, P, reps):
    n = (size // P) ** 2
    ld = -(-3 * P * P // 128) * 128
    dp = torch.randn(B * T, n + 1, ld, device="cuda")
    x = torch.randn(B, 3, T, size, size, device="cuda")
    pix = B * T * size * size
    out = {}
    for name, mode in (("grad", hip.UNPATCH_GRAD), ("absmax", hip.UNPATCH_ABSMAX), ("l2", hip.UNPATCH_L2), ("grad_x_input", hip.UNPATCH_GRAD_X_INPUT)):
        o = torch.empty((B, 3, T, size, size) if mode == hip.UNPATCH_GRAD else (B, T, size, size), device="cuda")
        run = lambda: hip.unpatchify(dp, o, B=B, T=T, size=size, patch=P, mode=mode, frame_rows=n + 1, row_offset=1,
                                     x=x if mode == hip.UNPATCH_GRAD_X_INPUT else None)
        run()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        # 3 gradient floats read per pixel (+ 3 of x), 3 or 1 written
        nbytes = 4 * pix * (3 + (3 if mode == hip.UNPATCH_GRAD_X_INPUT else 0) + (3 if mode == hip.UNPATCH_GRAD else 1))
        med = statistics.median(ms)
        out[name] = dict(median_us=round(med * 1e3, 1), bytes=nbytes, gb_per_s=round(nbytes / med / 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    m = m.cuda().train()
    B = args.batch
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
    out = dict(device=torch.cuda.get_device_name(0), config="VIT_B16_T8", B=B, T=cfg.num_frames, rounds=args.rounds, model=res,
               unpatchify=kernel_times(B, cfg.num_frames, cfg.input_size, cfg.patch_size, args.kernel_reps))
    base, dx = res["backward"]["median_ms"], res["backward_dx"]["median_ms"]
    out["input_grad_stage_ms"] = round(dx - base, 3)
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "input_grad_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
