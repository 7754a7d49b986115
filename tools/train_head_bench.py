#!/usr/bin/env python
"""Time and count the launches of a training step's tail - head + criterion + their backward - on both routes:

    hip    training.HeadFn + gava_clip_amd.TrainCriterion (gava_train_head*, gava_train_criterion*)
    torch  the traced torch ops of VitaCLIP._train_head + the criterion written out in torch ops, hits read with .item()

at a c2-shaped tail (B = 64, C = 3) and a c3-shaped one (B = 32, C = 400), E = 512, one prompt per class.  Launches are counted
with torch.profiler (device kernels of one step); times are the mean of --steps steps after --warmup, host clock around a
device synchronisation.  Writes profiles/train_head_bench.json.

    python tools/train_head_bench.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gava_clip_amd import TrainCriterion  # noqa: E402
from gava_clip_amd.training import HeadFn  # noqa: E402


def torch_tail(video, text, ls, labels, beta=0.2, alpha=0.25, gamma=2.0):
    vf = video / video.norm(dim=-1, keepdim=True)
    tf = text / text.norm(dim=-1, keepdim=True)
    logits = ls.exp() * vf @ tf.t()
    C = logits.shape[-1]
    ce = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    p = logits.softmax(-1)
    onehot = torch.nn.functional.one_hot(labels, C)
    frac = ((labels - p.argmax(-1)).abs() / (C - 1)).float()
    w = ((beta * frac.unsqueeze(-1) + alpha * (1 - p) ** gamma) * onehot).sum(-1)
    loss = (ce * w).mean()
    loss.backward()
    return loss.item(), (logits.topk(1, dim=1)[1] == labels.view(-1, 1)).sum().item()      # training/train.py:478-479


def hip_tail(video, text, ls, labels, off, crit):
    logits, _ = HeadFn.apply(video, text, ls, None, off)
    loss = crit(logits, labels)
    loss.backward()
    return loss, crit.last["hits"]                                                          # device tensors: no host wait


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "cases": {}}
    for name, B, C in (("c2_tail", 64, 3), ("c3_tail", 32, 400)):
        g = torch.Generator().manual_seed(B + C)
        E = 512
        video = torch.randn(B, E, generator=g).cuda().requires_grad_()
        text = torch.randn(C, E, generator=g).cuda().requires_grad_()
        ls = torch.tensor(2.0, device="cuda", requires_grad=True)
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        off = torch.arange(C + 1, dtype=torch.int32, device="cuda")
        crit = TrainCriterion(focal_ordinal=True, beta=0.2)
        routes = {"hip": lambda: hip_tail(video, text, ls, labels, off, crit), "torch": lambda: torch_tail(video, text, ls, labels)}
        res = {}
        for route, fn in routes.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
                fn()
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name]
            res[route] = {"ms_per_step": round(ms, 4), "device_kernels": len(kernels),
                          "device_us": round(sum(e.device_time for e in kernels), 2)}
        out["cases"][name] = dict(B=B, C=C, E=E, **res)
        print(name, json.dumps(res))
    path = os.path.join(REPO, "profiles", "train_head_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
