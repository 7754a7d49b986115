#!/usr/bin/env python
"""Training from decoded uint8 videos: one c2-like training step (forward + loss + backward, ViT-B/16, 3 classes) through
`forward_frames` against the two-step route `model(pre.batch(videos))`, same process, alternating; and the one-launch batch
preprocessing against one launch per clip.  One JSON line per measurement, with the spread of the repeats.

    python tools/train_frames_bench.py [--repeats 7] [--out profiles/r06_train_frames.txt]"""
import argparse, json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import torch
from gava_clip_amd import VitaCLIP
from gava_clip_amd.config import VitaConfig
from gava_clip_amd.preprocess import ClipPreprocessor, TrainClipPreprocessor
from helpers import model_kwargs

HEADER = """# tools/train_frames_bench.py (MI355X, one box, one process; the routes alternate inside every repeat)
# train_step: host wall clock around ONE step, from a device synchronise before the forward to one after the backward -
#   preprocessing or descriptor building, the random-sample branch's host draws, forward, cross-entropy, backward; no optimizer
#   step.  It is what a training loop pays per step.  two_step_launch_per_clip is the parent commit's route (batch() launched
#   one kernel per clip), two_step_one_launch the same route through gava_preprocess_clips.
# preprocess_batch: device events around 20 back-to-back calls, per call; one_launch_batch() includes building and copying
#   the descriptors and allocating the output, one_launch_kernel_only does not.
# all_ms lists every timed repeat in order."""
a = None
d = torch.device("cuda")
lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                all_ms=[round(v, 3) for v in ms])


def per_clip(pre, vids, x):       # what ClipPreprocessor.batch did before the one-launch kernel: one launch per clip
    for b, v in enumerate(vids):
        pre(v, out=x[b])
    return x


def train_case(name, B, T, n_frames):
    cfg = VitaConfig(num_frames=T)
    cls_path = os.path.join(REPO, "gava_clip_amd", "data", "classes", "updrs_3cls_classes.txt")
    torch.manual_seed(0)
    model = VitaCLIP(**model_kwargs(cfg, cls_path)).cuda().train()
    g = torch.Generator(device=d).manual_seed(1)
    vids = [torch.randint(0, 256, (n_frames, 360, 640, 3), dtype=torch.uint8, device=d, generator=g) for _ in range(B)]
    y = torch.randint(0, 3, (B,), device=d, generator=g)
    xbuf = torch.empty(B, 3, T, 224, 224, device=d)
    for pname, pre in (("eval", ClipPreprocessor(num_frames=T, sampling_rate=1, spatial_size=224)),
                       ("random", TrainClipPreprocessor(num_frames=T, sampling_rate=1, spatial_size=224))):
        routes = {"frames": lambda: model.forward_frames(vids, pre)[0],
                  "two_step_one_launch": lambda: model(pre.batch(vids))[0]}
        if pname == "eval":
            routes["two_step_launch_per_clip"] = lambda: model(per_clip(pre, vids, xbuf))[0]

        def step(fn):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            torch.nn.functional.cross_entropy(fn(), y).backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        times = {k: [] for k in routes}
        for r in range(a.warmup + a.repeats):            # alternating, so that drift of the box hits every route alike
            for k, fn in routes.items():
                ms = step(fn)
                if r >= a.warmup:
                    times[k].append(ms)
        for k, ms in times.items():
            emit(what="train_step", case=name, preprocessor=pname, route=k, clips=B, frames=T, video="%dx360x640" % n_frames, **spread(ms))
    del model
    torch.cuda.empty_cache()


def prep_case(B=64, T=8, iters=20):
    g = torch.Generator(device=d).manual_seed(2)
    vids = [torch.randint(0, 256, (32, 360, 640, 3), dtype=torch.uint8, device=d, generator=g) for _ in range(B)]
    pre = ClipPreprocessor(num_frames=T, sampling_rate=2, spatial_size=224)
    x = torch.empty(B, 3, T, 224, 224, device=d)
    from gava_clip_amd import hip
    desc, keep = pre.descriptors(vids)
    lut = pre.lut(d)
    routes = {"launch_per_clip": lambda: per_clip(pre, vids, x),
              "one_launch_kernel_only": lambda: hip.preprocess_clips(desc, x, T=T, size=224, lut=lut),
              "one_launch_batch()": lambda: pre.batch(vids)}
    times = {k: [] for k in routes}
    for r in range(a.warmup + a.repeats):
        for k, fn in routes.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record(); torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) / iters)
    for k, ms in times.items():
        emit(what="preprocess_batch", route=k, clips=B, frames=T, video="32x360x640", **spread(ms))


def main():
    global a
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    print(HEADER, flush=True)
    prep_case()
    train_case("c2", 64, 8, 32)
    train_case("updrs", 4, 70, 80)
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEADER + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
