#!/usr/bin/env python
"""What the mix and the soft-target criterion cost, at BASELINE config c2's clip shape (ViT-B/16, T = 8, 224 px) for B = 64 clips.

1. gava_mix_clips alone - in place and out of place, Mixup and CutMix, one draw for the batch ("batch") and one per clip
   ("elem": half the pairs Mixup, half CutMix, every lam and box its own) - next to the same mix from torch ops
   (x * lam + x.flip(0) * (1 - lam), slice assignment from x.flip(0)).  Median time of --kernel-reps runs between device events;
   `bytes` is the least traffic the mix needs (every input byte that is used read once, every output byte that changes or is
   new written once), gb_per_s that over the median time and hbm_peak_fraction that over the 8.0 TB/s of the data sheet (a
   float4 copy reaches about 6.3 TB/s).  The torch rows are charged the same bytes, so the columns compare.
2. SoftTargetCriterion forward + backward against the same expression in torch ops (forward + backward), at (64, 3) and
   (64, 400): median host-clock time per call of --criterion-reps calls that end in one device synchronisation.
3. A c2 training step (forward + backward + torch AdamW on the trainable subset, as bench.py's train_step) with integer labels
   and cross-entropy, and with ClipMixer + SoftTargetCriterion in front of it: one process, alternating rounds, the median.

Nothing is gated.  Writes profiles/mix_bench.json.

    python tools/mix_bench.py [--batch 64] [--rounds 5] [--warmup 2] [--kernel-reps 20] [--criterion-reps 200] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from gava_clip_amd import ClipMixer, SoftTargetCriterion, VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, the data sheet's figure


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


def plans(B, S):
    rev = (B - 1 - np.arange(B)).astype(np.int32)
    none = np.zeros((B, 4), dtype=np.int32)
    half = (S // 8, S // 8 + int(S * 0.7071), S // 5, S // 5 + int(S * 0.7071))         # lam = 0.5: half the image
    rng = np.random.default_rng(3)
    lam_e = rng.uniform(0.1, 0.9, B).astype(np.float32)
    box_e = none.copy()
    for i in range(B // 4, B - B // 4):                                                 # the inner pairs CutMix, the outer Mixup
        side = int(S * np.sqrt(1 - lam_e[i]))
        y0, x0 = int(rng.integers(0, S - side + 1)), int(rng.integers(0, S - side + 1))
        box_e[i] = (y0, y0 + side, x0, x0 + side)
    return {"mixup batch": dict(partner=rev, lam=np.full(B, 0.3, dtype=np.float32), box=none),
            "cutmix batch": dict(partner=rev, lam=np.full(B, 0.5, dtype=np.float32), box=np.tile(np.array(half, dtype=np.int32), (B, 1))),
            "elem": dict(partner=rev, lam=lam_e, box=box_e)}


def least_bytes(plan, clip_bytes, H, W, inplace):
    """Read every input byte that is used once, write every output byte that is new or changes once."""
    B = len(plan["partner"])
    box = plan["box"]
    frac = np.where((box[:, 1] > box[:, 0]) & (box[:, 3] > box[:, 2]), (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2]) / float(H * W),
                    (plan["lam"] != 1).astype(np.float64))
    frac = np.where(plan["partner"] == np.arange(B), 0.0, frac)
    if not inplace:
        return int(2 * B * clip_bytes)
    pair = np.maximum(frac, frac[plan["partner"]])          # a position is read in both clips when either member changes there
    return int((pair.sum() + frac.sum()) * clip_bytes)


def torch_mix(x, plan, inplace):
    B = x.shape[0]
    lam, box = plan["lam"], plan["box"]
    uniform = (lam == lam[0]).all() and (box == box[0]).all()
    y0, y1, x0, x1 = (int(v) for v in box[0])
    if uniform and y1 > y0:
        out = x if inplace else x.clone()
        out[..., y0:y1, x0:x1] = x.flip(0)[..., y0:y1, x0:x1]
        return out
    if uniform:
        out = x * float(lam[0]) + x.flip(0) * (1.0 - float(lam[0]))
        return x.copy_(out) if inplace else out
    src = x.clone() if inplace else x                       # per clip: the partner's original pixels are needed
    out = x if inplace else torch.empty_like(x)
    for i in range(B):
        j = int(plan["partner"][i])
        y0, y1, x0, x1 = (int(v) for v in box[i])
        if y1 > y0 and x1 > x0:
            if not inplace:
                out[i] = src[i]
            out[i, ..., y0:y1, x0:x1] = src[j, ..., y0:y1, x0:x1]
        else:
            torch.add(src[i] * float(lam[i]), src[j], alpha=1.0 - float(lam[i]), out=out[i])
    return out


def torch_soft_criterion(logits, targets, *, alpha, gamma, beta, scale):
    ce = torch.nn.functional.cross_entropy(logits, targets, reduction="none")
    C = logits.shape[-1]
    p = logits.softmax(-1)
    frac = ((targets.argmax(-1) - p.argmax(-1)).abs() / (C - 1)).float()
    w = ((beta * frac.unsqueeze(-1) + alpha * (1 - p) ** gamma) * targets).sum(-1) * scale
    return (ce * w).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--criterion-reps", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    B, T, S = args.batch, cfg.num_frames, cfg.input_size
    x = torch.from_numpy(synth.synth_clip(B, T, S, seed=21)).cuda()
    clip_bytes = 3 * T * S * S * 4
    out = dict(device=torch.cuda.get_device_name(0), config="VIT_B16_T8", B=B, T=T, size=S, clip_mib=round(clip_bytes / 2 ** 20, 2),
               hbm_peak_tb_per_s=HBM_PEAK / 1e12)

    # 1. the mix alone
    mixes = {}
    work, dst = x.clone(), torch.empty_like(x)
    with torch.no_grad():
        for name, plan in plans(B, S).items():
            desc = hip.mix_descriptors(plan, S, S)
            ref = hip.mix_clips(x, desc)
            assert torch.allclose(torch_mix(x, plan, False), ref, rtol=1e-6, atol=1e-6), name       # the two routes mix the same
            for inplace in (False, True):
                moved = least_bytes(plan, clip_bytes, S, S, inplace)
                # in place the data changes from run to run (a mix of a mix): the traffic does not
                runs = {"hip": (lambda: hip.mix_clips(work, desc, out=work)) if inplace else (lambda: hip.mix_clips(x, desc, out=dst)),
                        "torch": (lambda: torch_mix(work, plan, True)) if inplace else (lambda: torch_mix(x, plan, False))}
                for route, fn in runs.items():
                    r = event_us(fn, args.kernel_reps)
                    r.update(bytes=moved, gb_per_s=round(moved / r["median_us"] / 1e3, 1),
                             hbm_peak_fraction=round(moved / (r["median_us"] * 1e-6) / HBM_PEAK, 3))
                    mixes[f"{name}, {'in place' if inplace else 'out of place'}, {route}"] = r
                work.copy_(x)
    out["mix_clips"] = mixes
    del work, dst
    torch.cuda.empty_cache()

    # 2. the criterion, forward + backward
    crit_rows = {}
    kw = dict(alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)
    for Bc, C in ((64, 3), (64, 400)):
        g = torch.Generator().manual_seed(C)
        z = (torch.randn(Bc, C, generator=g) * 2.5).cuda().requires_grad_()
        t = torch.softmax(torch.randn(Bc, C, generator=g) * 3, -1).cuda()
        crit = SoftTargetCriterion(focal_ordinal=True, **kw)

        def run_hip():
            z.grad = None
            crit(z, t).backward()

        def run_torch():
            z.grad = None
            torch_soft_criterion(z, t, **kw).backward()
        run_hip()
        g_hip = z.grad.clone()
        run_torch()
        assert torch.allclose(g_hip, z.grad, rtol=1e-3, atol=1e-6)
        row = {}
        for r in range(args.warmup + args.rounds):
            for route, fn in (("hip", run_hip), ("torch", run_torch)):
                ms = timed(lambda: [fn() for _ in range(args.criterion_reps)])
                if r >= args.warmup:
                    row.setdefault(route, []).append(ms / args.criterion_reps * 1e3)
        crit_rows[f"{Bc}x{C}"] = {route: dict(median_us_per_call=round(statistics.median(v), 1), min_us_per_call=round(min(v), 1))
                                  for route, v in row.items()}
    out["soft_criterion_fwd_bwd"] = crit_rows

    # 3. a c2 training step with and without the mixer
    if not args.no_step:
        model = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
        model.load_state_dict(synth_torch_state(cfg, 3), strict=True)
        model = model.cuda().train()
        y = torch.arange(B, device="cuda") % 3
        opt = torch.optim.AdamW([q for q in model.parameters() if q.requires_grad], lr=1e-5)
        mixer, soft = ClipMixer(3, mode="elem", seed=0), SoftTargetCriterion(focal_ordinal=True, beta=0.2)

        def step_labels():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(x)[0], y).backward()
            opt.step()

        def step_mixed():
            opt.zero_grad(set_to_none=True)
            xm, t = mixer(x, y)
            soft(model(xm)[0], t).backward()
            opt.step()
        steps = {"labels_cross_entropy": step_labels, "mixer_soft_criterion": step_mixed}
        times = {k: [] for k in steps}
        for r in range(args.warmup + args.rounds):
            for k, fn in steps.items():
                ms = timed(fn)
                if r >= args.warmup:
                    times[k].append(ms)
        out["train_step_c2"] = {k: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2))
                                for k, v in times.items()}
        out["train_step_c2"]["mixed_over_labels"] = round(out["train_step_c2"]["mixer_soft_criterion"]["median_ms"] /
                                                          out["train_step_c2"]["labels_cross_entropy"]["median_ms"], 4)
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "mix_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
