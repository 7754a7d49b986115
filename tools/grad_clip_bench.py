#!/usr/bin/env python
"""What clipping by global norm inside the fused AdamW step costs, at BASELINE config c2's trainable set (ViT-B/16, T = 8, 224 px:
28.5 M fp32 elements), with the gradients of one real backward.

1. gava_grad_norm alone over the optimizer's own table and chunk list.  `bytes` is what it has to read, 4 bytes per gradient
   element; gb_per_s that over the median time, hbm_peak_fraction that over the data sheet's 8.0 TB/s (a float4 copy reaches
   about 6.3 TB/s).  Measured twice: right after a pass of torch ops over the same gradients ("warm": what the 256 MiB Infinity
   Cache may still hold) and after 1 GiB of unrelated traffic ("cold").
2. FusedAdamW.step() plain and with max_grad_norm.
3. With a GradScaler: scaler.step(FusedAdamW(max_grad_norm=...)) against the torch sequence scaler.unscale_(opt) +
   clip_grad_norm_ + scaler.step(opt), the latter with FusedAdamW and with torch.optim.AdamW.  The scaled gradients are restored
   from a master copy before every timed call (unscale_ and clip_grad_norm_ rewrite them); the restore is outside the window.
4. A c2 training step (forward + backward + FusedAdamW.step()), B = --batch, with and without max_grad_norm: host clock around
   a step that ends in a device synchronisation.  The base row is THIS tree's step without max_grad_norm, not a build of the
   tree before clipping existed (its update kernel has the same floating-point instructions, but the source was refactored);
   the JSON says so and carries the whole-step medians that profiles/fused_adamw_bench.json recorded for that earlier tree.

1 - 3: device events around one call, --reps calls per round, the variants alternating in one process, the first --warmup
rounds dropped; medians.  Nothing is gated.  Writes profiles/grad_clip_bench.json (or --out).

    python tools/grad_clip_bench.py [--batch 64] [--rounds 5] [--warmup 2] [--reps 10] [--step-rounds 12] [--no-step] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from gava_clip_amd import FusedAdamW, VitaCLIP, hip  # noqa: E402
from gava_clip_amd.config import VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, the data sheet's figure
HYPER = dict(lr=4e-4, weight_decay=0.2)      # the recipe's (training/train.py)


def event_ms(run, before=None, after=None):
    """Device time of run(); before() and after() are outside the window."""
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    if after is not None:
        after()
    return e0.elapsed_time(e1)


def alternate(variants, rounds, warmup, reps):
    """variants: {name: (run, before or None[, after])}.  Every round times every variant `reps` times, in turn."""
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, (run, *around) in variants.items():
            ms = [event_ms(run, *around) for _ in range(reps)]
            if r >= warmup:
                times[k] += ms
    return {k: dict(median_us=round(statistics.median(v) * 1e3, 1), min_us=round(min(v) * 1e3, 1), calls=len(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_clip_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_clip_bench.py measures on the device: none found")
    cfg, B = VIT_B16_T8, args.batch
    torch.manual_seed(0)
    model = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    model.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    model = model.cuda().train()
    x = torch.randn(B, 3, cfg.num_frames, cfg.input_size, cfg.input_size, device="cuda")
    y = torch.arange(B, device="cuda") % 3
    torch.nn.functional.cross_entropy(model(x)[0], y).backward()
    params = [p for p in model.parameters() if p.grad is not None]
    n_elem = sum(p.numel() for p in params)
    master = [p.grad.clone() for p in params]                      # the unscaled gradients of that backward
    total = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.double()) for g in master])))
    max_norm = 0.3 * total                                         # the coefficient is well below 1: the clip does its work
    out = dict(device=torch.cuda.get_device_name(0), batch=B, trainable_tensors=len(params), trainable_elements=n_elem,
               largest_tensor_elements=max(p.numel() for p in params), grad_norm_of_the_backward=total, max_grad_norm=max_norm,
               rounds=args.rounds, warmup=args.warmup, reps=args.reps, hbm_peak_tb_per_s=HBM_PEAK / 1e12)

    plain, clip = FusedAdamW(model, **HYPER), FusedAdamW(model, max_grad_norm=max_norm, **HYPER)
    theirs = torch.optim.AdamW(params, **HYPER)
    plain.step(); clip.step(); theirs.step()
    assert abs(float(clip.last["grad_norm"]) - total) <= 1e-6 * total and float(clip.last["clip_coef"]) < 0.31

    # 1. the norm alone, over clip's table
    tab, dev, n_chunks, tbytes = clip._table
    ws, tensor_norm, stats, _ps = clip._clip
    n = hip.GradNormArgs()
    n.table, n.table_host, n.chunks = dev.data_ptr(), tab, dev.data_ptr() + tbytes
    n.n_tensors, n.n_chunks, n.n_groups, n.max_norm = len(tab), n_chunks, len(clip.param_groups), max_norm
    n.workspace, n.tensor_norm, n.stats = ws.data_ptr(), tensor_norm.data_ptr(), stats.data_ptr()
    lib = hip.load()
    scratch = torch.empty(2 ** 28, device="cuda")                  # 1 GiB

    def run_norm():
        hip.check(lib.gava_grad_norm(C.byref(n), hip.stream_ptr()), "gava_grad_norm")
    live = [p.grad for p in params]
    rows = alternate({"warm": (run_norm, lambda: torch._foreach_mul_(live, 1.0)),          # rewrites every gradient, as a backward does
                      "cold": (run_norm, lambda: scratch.fill_(1.0))}, args.rounds, args.warmup, args.reps)
    moved = 4 * n_elem
    for r in rows.values():
        r.update(bytes=moved, gb_per_s=round(moved / r["median_us"] / 1e3, 1), hbm_peak_fraction=round(moved / (r["median_us"] * 1e-6) / HBM_PEAK, 3))
    out["grad_norm"] = dict(chunks=n_chunks, launches=2, **rows)
    del scratch
    torch.cuda.empty_cache()

    # 2. the step, plain and clipped
    out["fused_step"] = alternate({"plain": (plain.step, None), "max_grad_norm": (clip.step, None)}, args.rounds, args.warmup, args.reps)
    out["fused_step"]["clipped_over_plain"] = round(out["fused_step"]["max_grad_norm"]["median_us"] / out["fused_step"]["plain"]["median_us"], 3)

    # 3. under a GradScaler
    scale = 2.0 ** 16
    scaled = [g * scale for g in master]
    grads = [p.grad for p in params]

    def restore():
        torch._foreach_copy_(grads, scaled)

    scalers = {k: torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=10 ** 9) for k in ("clip", "plain", "theirs")}

    def fused_clipped():
        scalers["clip"].step(clip)

    def torch_sequence(key, opt):
        def run():
            s = scalers[key]
            s.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            s.step(opt)
        return run

    def update(key):       # GradScaler allows one step per update
        return scalers[key].update

    variants = {"scaler.step(FusedAdamW(max_grad_norm))": (fused_clipped, restore, update("clip")),
                "unscale_ + clip_grad_norm_ + scaler.step(FusedAdamW)": (torch_sequence("plain", plain), restore, update("plain")),
                "unscale_ + clip_grad_norm_ + scaler.step(torch.optim.AdamW)": (torch_sequence("theirs", theirs), restore, update("theirs"))}
    for s in scalers.values():                                     # a scaler must have scaled something before its first step
        s.scale(torch.zeros((), device="cuda"))
    out["scaler_step"] = alternate(variants, args.rounds, args.warmup, args.reps)
    base = out["scaler_step"]["scaler.step(FusedAdamW(max_grad_norm))"]["median_us"]
    out["scaler_step"]["torch_sequence_fused_over_clipped"] = round(out["scaler_step"]["unscale_ + clip_grad_norm_ + scaler.step(FusedAdamW)"]["median_us"] / base, 3)
    out["scaler_step"]["torch_sequence_torch_adamw_over_clipped"] = round(out["scaler_step"]["unscale_ + clip_grad_norm_ + scaler.step(torch.optim.AdamW)"]["median_us"] / base, 3)

    # 4. a c2 training step with and without the clip
    if not args.no_step:
        def step_with(opt):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.zero_grad(set_to_none=True)
                torch.nn.functional.cross_entropy(model(x)[0], y).backward()
                opt.step()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            return run
        steps = {"plain": step_with(plain), "max_grad_norm": step_with(clip)}
        times = {k: [] for k in steps}
        for r in range(args.warmup + args.step_rounds):
            for k, fn in steps.items():
                ms = fn()
                if r >= args.warmup:
                    times[k].append(ms)
        out["train_step_c2"] = {k: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), steps=len(v))
                                for k, v in times.items()}
        out["train_step_c2"]["base"] = "this tree's FusedAdamW.step() without max_grad_norm (not a build of the tree before clipping)"
        earlier = os.path.join(REPO, "profiles", "fused_adamw_bench.json")
        if os.path.exists(earlier):
            with open(earlier) as f:
                runs = json.load(f).get("runs", [])
            out["train_step_c2"]["recorded_before_clipping_fused_whole_step_ms"] = [round(r["whole_step_ms"], 2) for r in runs if r.get("optimizer") == "fused"]
        out["train_step_c2"]["clipped_over_plain"] = round(out["train_step_c2"]["max_grad_norm"]["median_ms"] /
                                                           out["train_step_c2"]["plain"]["median_ms"], 4)
    print(json.dumps(out, indent=1))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
