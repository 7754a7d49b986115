#!/usr/bin/env python
"""What RandAugment on the device costs, at BASELINE config c2's source shape: B = 64 clips of T = 8 frames, 256 x 340 uint8 RGB.

1. Each kind of work alone, one op on every frame of the batch (512 frames): the entry point(s) it needs between device events,
   the descriptor table already on the device.  `bytes` is every frame read once and written once (the histogram pass: read
   once); gb_per_s that over the median time, hbm_peak_fraction that over the data sheet's 8.0 TB/s.
2. RandAugment.apply for the reference recipe "rand-m7-n4-mstd0.5-inc1", plans drawn under a fixed seed: the host clock around
   the whole call ending in a device synchronisation (descriptor tables, pinned copies and launches included), and the draw of
   the 64 plans on its own.
3. The same clips and plans through Pillow on the host, where Pillow is importable: one process, one core, --pil-clips clips
   timed and scaled to the batch.
4. A c2 training step through forward_frames (forward + backward + torch AdamW on the trainable subset) with
   TrainClipPreprocessor and with AugmentedClipPreprocessor: one process, alternating rounds, the median.

Nothing is gated.  Writes profiles/augment_bench.json.

    python tools/augment_bench.py [--batch 64] [--rounds 5] [--warmup 2] [--kernel-reps 20] [--pil-clips 4] [--no-step]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import rand_augment_ref as ref  # noqa: E402
from gava_clip_amd import AugmentedClipPreprocessor, RandAugment, VitaCLIP, hip  # noqa: E402
from gava_clip_amd.config import VIT_B16_T8  # noqa: E402
from gava_clip_amd.preprocess import TrainClipPreprocessor  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, the data sheet's figure
CONFIG = "rand-m7-n4-mstd0.5-inc1"
H, W, N_FRAMES = 256, 340, 16
KINDS = {"table, fixed (Invert)": ("Invert", None, None), "table, blend (Brightness 1.54)": ("Brightness", 1.54, None),
         "table + statistics (Equalize)": ("Equalize", None, None), "table + statistics (AutoContrast)": ("AutoContrast", None, None),
         "table + L statistics (Contrast 1.54)": ("Contrast", 1.54, None), "color (1.54)": ("Color", 1.54, None),
         "sharpness (1.54)": ("Sharpness", 1.54, None), "affine bilinear (Rotate 21)": ("Rotate", 21.0, ref.BILINEAR),
         "affine bicubic (Rotate 21)": ("Rotate", 21.0, ref.BICUBIC), "affine bicubic (TranslateXRel 0.3)": ("TranslateXRel", 0.3, ref.BICUBIC)}


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


def rate(r, moved):
    r.update(bytes=moved, gb_per_s=round(moved / r["median_us"] / 1e3, 1), hbm_peak_fraction=round(moved / (r["median_us"] * 1e-6) / HBM_PEAK, 3))
    return r


def layer_args(videos, idx, layer, arena):
    """one layer over the whole batch as (gava_augment_args, keep-alive): the table on the device, slots per frame"""
    T = len(idx[0])
    tables, off = [], 0
    for v, ix in zip(videos, idx):
        rows = RandAugment._rows(layer, T, H, W)
        frame = H * W * 3
        rows["src"] = np.uint64(v.data_ptr()) + np.asarray(ix, dtype=np.uint64) * np.uint64(frame)
        rows["dst"] = np.uint64(arena.data_ptr() + off) + np.arange(T, dtype=np.uint64) * np.uint64(frame)
        off += T * frame
        tables.append(rows)
    rows = np.concatenate(tables)
    n = rows.shape[0]
    rows["lut_slot"] = rows["hist_slot"] = np.arange(n)
    host = torch.from_numpy(rows.view(np.uint8).copy())
    dev = host.cuda()
    luts = torch.empty(n, 3, 256, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(n, 4, 256, dtype=torch.int32, device="cuda")
    a = hip.AugmentArgs()
    a.desc_host, a.desc, a.hist, a.luts, a.n, a.n_hist, a.n_luts = host.data_ptr(), hip.ptr(dev), hip.ptr(hist), hip.ptr(luts), n, n, n
    return a, (host, dev, luts, hist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--pil-clips", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: nothing here is measured without one")
    cfg = VIT_B16_T8
    B, T = args.batch, cfg.num_frames
    base = [ref.video(N_FRAMES, H, W, 40 + i) for i in range(4)]                 # four distinct videos, repeated over the batch
    videos_cpu = [base[i % 4] for i in range(B)]
    videos = [torch.from_numpy(v).cuda() for v in videos_cpu]
    frames_bytes = B * T * H * W * 3
    out = dict(device=torch.cuda.get_device_name(0), B=B, T=T, H=H, W=W, frames=B * T, frames_mib=round(frames_bytes / 2 ** 20, 1),
               hbm_peak_tb_per_s=HBM_PEAK / 1e12, config=CONFIG)
    lib = hip.load()
    stream = hip.stream_ptr()
    idx = [list(range(1, 1 + 2 * T, 2)) for _ in range(B)]
    arena = torch.empty(frames_bytes, dtype=torch.uint8, device="cuda")

    # 1. every kind alone
    kinds = {}
    for name, (op, arg, filt) in KINDS.items():
        a, keep = layer_args(videos, idx, (op, arg, None if filt is None else [filt] * T), arena)
        needs_hist = op in ("Equalize", "AutoContrast", "Contrast")
        is_table = needs_hist or op in ("Invert", "Brightness")

        def call(stage):
            hip.check(getattr(lib, "gava_augment_" + stage)(C.byref(a), stream), stage)
        row = {}
        if needs_hist:
            row["hist"] = rate(event_us(lambda: call("hist"), args.kernel_reps), frames_bytes)
            keep[3].zero_()
            row["hist + luts"] = event_us(lambda: (call("hist"), call("luts")), args.kernel_reps)
        elif is_table:
            row["luts"] = event_us(lambda: call("luts"), args.kernel_reps)
        row["apply"] = rate(event_us(lambda: call("apply"), args.kernel_reps), 2 * frames_bytes)
        stages = (("hist", "luts") if needs_hist else ("luts",) if is_table else ()) + ("apply",)
        row["layer"] = rate(event_us(lambda: [call(s) for s in stages], args.kernel_reps), (3 if needs_hist else 2) * frames_bytes)
        kinds[name] = row
        # the result is the restatement's, on the first clip's first frame
        torch.cuda.synchronize()
        got = arena[:H * W * 3].view(H, W, 3).cpu().numpy()
        assert np.array_equal(got, ref.apply_op(videos_cpu[0][idx[0][0]], op, arg, filt)), name
        del a, keep
    out["kinds"] = kinds
    del arena

    # 2. the recipe's policy over the batch
    aug = RandAugment(CONFIG)
    random.seed(7)
    np.random.seed(7)
    t0 = time.perf_counter()
    plans = [aug.plan(T, H, W) for _ in range(B)]
    draw_ms = (time.perf_counter() - t0) * 1e3
    counts = {}
    for p in plans:
        for layer in p:
            counts[layer[0]] = counts.get(layer[0], 0) + 1
    ms = []
    for r in range(args.warmup + args.rounds):
        t = timed(lambda: aug.apply(videos, idx, plans))
        if r >= args.warmup:
            ms.append(t)
    dev_us = event_us(lambda: aug.apply(videos, idx, plans), args.kernel_reps)
    out["policy"] = dict(draw_64_plans_ms=round(draw_ms, 3), applied_ops=sum(len(p) for p in plans), ops=counts,
                         clips_without_op=sum(not p for p in plans),
                         apply_host_clock_ms=dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3)),
                         apply_between_events_us=dev_us)

    # 3. Pillow on the host
    try:
        import PIL
        n = max(1, min(args.pil_clips, B))
        t0 = time.perf_counter()
        for v, ix, plan in list(zip(videos_cpu, idx, plans))[:n]:
            frames = [v[i] for i in ix]
            for name, arg, filters in plan:
                frames = [ref.pillow_op(f, name, arg, None if filters is None else filters[k]) for k, f in enumerate(frames)]
        per_clip = (time.perf_counter() - t0) * 1e3 / n
        out["pillow_host"] = dict(version=PIL.__version__, clips_timed=n, ms_per_clip_one_core=round(per_clip, 2),
                                  ms_per_batch_one_core=round(per_clip * B, 1))
    except ImportError:
        out["pillow_host"] = "Pillow is not importable here: not measured"

    # 4. a c2 training step from decoded videos, with and without the augmentation
    if not args.no_step:
        model = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
        model.load_state_dict(synth_torch_state(cfg, 3), strict=True)
        model = model.cuda().train()
        y = torch.arange(B, device="cuda") % 3
        opt = torch.optim.AdamW([q for q in model.parameters() if q.requires_grad], lr=1e-5)
        pres = {"plain": TrainClipPreprocessor(num_frames=T, sampling_rate=2, spatial_size=cfg.input_size),
                "augmented": AugmentedClipPreprocessor(CONFIG, num_frames=T, sampling_rate=2, spatial_size=cfg.input_size)}

        def step(pre):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model.forward_frames(videos, pre)[0], y).backward()
            opt.step()
        times = {k: [] for k in pres}
        for r in range(args.warmup + args.rounds):
            for k, pre in pres.items():
                t = timed(lambda: step(pre))
                if r >= args.warmup:
                    times[k].append(t)
        out["train_step_c2_frames"] = {k: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2))
                                       for k, v in times.items()}
        out["train_step_c2_frames"]["augmented_over_plain"] = round(
            out["train_step_c2_frames"]["augmented"]["median_ms"] / out["train_step_c2_frames"]["plain"]["median_ms"], 4)
    print(json.dumps(out, indent=1))
    path = os.path.join(REPO, "profiles", "augment_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
