#!/usr/bin/env python
"""Multi-view evaluation, timed: `forward_views` (8 videos x 3 x 4 views = 96 clips, ViT-B/16, 8 frames) against
`forward_frames` on 96 clips of the same videos, same process, alternating; and `gava_view_scores` alone at (64, 30, 400).
One JSON line per measurement, with the spread of the repeats.

    python tools/views_bench.py [--repeats 9] [--out profiles/r07_multiview.txt]"""
import argparse, json, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import torch
from gava_clip_amd import VitaCLIP, hip
from gava_clip_amd.config import VitaConfig
from gava_clip_amd.preprocess import ClipPreprocessor
from helpers import model_kwargs

HEADER = """# tools/views_bench.py (MI355X, one box, one process; the two forward routes alternate inside every repeat)
# forward: device events around `iters` back-to-back calls after warm-up, per call, host work included (descriptors, launches).
#   views  = forward_views(8 videos of 32x360x640, ClipPreprocessor 3 spatial x 4 temporal views, sampling_rate 2): 96 clips in
#            one launch of the towers + gava_view_scores; the text features are cached by the call.
#   frames = forward_frames on 96 clips (each of the 8 videos 12 times, one view each) with cache_text_features on: the same
#            tower work on other crops, no score fusion.
#   The towers are the same kernels, so the two are expected to agree to within the run-to-run spread.
# view_scores: gava_view_scores alone on [64, 30, 400] logits, per call (its cost is its launch).
# all_ms lists every timed repeat in order."""
lines = []
d = torch.device("cuda")


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def spread(ms, nd=3):
    return dict(median_ms=round(statistics.median(ms), nd), min_ms=round(min(ms), nd), max_ms=round(max(ms), nd),
                all_ms=[round(v, nd) for v in ms])


def timed(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    print(HEADER, flush=True)
    cfg = VitaConfig(num_frames=8)
    torch.manual_seed(0)
    model = VitaCLIP(**model_kwargs(cfg, os.path.join(REPO, "gava_clip_amd", "data", "classes", "updrs_3cls_classes.txt"))).cuda().eval()
    g = torch.Generator(device=d).manual_seed(1)
    vids = [torch.randint(0, 256, (32, 360, 640, 3), dtype=torch.uint8, device=d, generator=g) for _ in range(8)]
    views = ClipPreprocessor(num_frames=8, sampling_rate=2, spatial_size=224, num_spatial_views=3, num_temporal_views=4)
    single = ClipPreprocessor(num_frames=8, sampling_rate=2, spatial_size=224)
    vids96 = [v for v in vids for _ in range(views.num_views)]
    model.cache_text_features = True
    routes = {"views": lambda: model.forward_views(vids, views), "frames": lambda: model.forward_frames(vids96, single)}
    times = {k: [] for k in routes}
    with torch.no_grad():
        for r in range(a.warmup + a.repeats):
            for k, fn in routes.items():
                ms = timed(fn, a.iters)
                if r >= a.warmup:
                    times[k].append(ms)
    for k, ms in times.items():
        emit(what="forward", route=k, clips=96, videos=8, views="3x4", frames=8, video="32x360x640", iters=a.iters, **spread(ms))
    x = torch.randn(64, 30, 400, device=d, generator=g) * 10
    vs = []
    for r in range(a.warmup + a.repeats):
        ms = timed(lambda: hip.view_scores(x), 200)
        if r >= a.warmup:
            vs.append(ms)
    emit(what="view_scores", shape=[64, 30, 400], iters=200, **spread(vs, 5))
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEADER + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
