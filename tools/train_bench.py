#!/usr/bin/env python
"""One training step (forward + loss.backward()) of the drop-in model at c2-like sizes: ms per phase, worst gradient sanity.
    python tools/train_bench.py [--B 64] [--iters 3] [--optimizer {torch,fused}] [--whole 20] [--json out.json]
--optimizer fused: gava_clip_amd.FusedAdamW built from the model (one kernel; it also writes the packed 16-bit copies of the summary
projections, so their refresh leaves the forward and backward columns).  --whole N: N more steps timed as a whole, one
synchronisation per step, after the per-phase ones; --json: medians of all columns, the optimizer's device time included."""
import argparse, json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import torch
import gava_clip_amd.config as C
from gava_clip_amd import VitaCLIP
from helpers import model_kwargs

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=64)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--optimizer", choices=("torch", "fused"), default="torch")
ap.add_argument("--whole", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()
cfg = C.VIT_B16_T8
cls_path = os.path.join(REPO, "gava_clip_amd", "data", "classes", "updrs_3cls_classes.txt")
torch.manual_seed(0)
model = VitaCLIP(**model_kwargs(cfg, cls_path)).cuda().train()
x = torch.randn(a.B, 3, cfg.num_frames, cfg.input_size, cfg.input_size, device="cuda")
y = torch.randint(0, 3, (a.B,), device="cuda")
if a.optimizer == "fused":
    from gava_clip_amd import FusedAdamW
    opt = FusedAdamW(model, lr=1e-4)
else:
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def step():
    t0 = time.perf_counter()
    logits = model(x)[0]
    loss = torch.nn.functional.cross_entropy(logits, y)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize(); t2 = time.perf_counter()
    ev0.record()
    opt.step()
    ev1.record()
    torch.cuda.synchronize(); t3 = time.perf_counter()
    return float(loss), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def whole_step():
    t0 = time.perf_counter()
    loss = torch.nn.functional.cross_entropy(model(x)[0], y)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


cols = []
for i in range(a.iters + 1):
    loss, f, b, o = step()
    if i > 0:
        cols.append((f, b, o, ev0.elapsed_time(ev1)))
    print(f"step {i}: loss {loss:.4f}  forward {f:.1f} ms  backward {b:.1f} ms  optimizer {o:.1f} ms  "
          f"-> {a.B / ((f + b + o) / 1e3):.0f} clips/s   peak mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
whole = [whole_step() for _ in range(a.whole)]
if whole:
    print(f"whole step, {a.whole} steps: median {statistics.median(whole):.2f} ms  min {min(whole):.2f} ms", flush=True)
if a.json:
    med = [statistics.median(c) for c in zip(*cols)] if cols else [None] * 4
    with open(a.json, "w") as fh:
        json.dump(dict(optimizer=a.optimizer, B=a.B, iters=a.iters, forward_ms=med[0], backward_ms=med[1], optimizer_ms=med[2],
                       optimizer_device_ms=med[3], whole_step_ms=statistics.median(whole) if whole else None,
                       whole_step_min_ms=min(whole) if whole else None, whole_steps=a.whole,
                       trainable_parameters=sum(p.numel() for p in model.parameters() if p.requires_grad)), fh, indent=1)
        fh.write("\n")
