#!/usr/bin/env python
"""Stand-alone timing of the key-streaming attention kernels against the single-pass 320-key class, and end-to-end
forward time of VitaCLIP at long-clip shapes.  One JSON line per measurement.

    python tools/long_attn_bench.py [--e2e]

Kernels: ViT-L/14 layout (257 frame rows, G = 8, 16 heads, 512 frames): T = 32 (298 keys, single-pass kernel) against
T = 64 (330 keys, streaming kernel); forward TF/s count 4 * n_q * n_keys * 64 flops per (frame, head).  Backward: the same
two shapes through gava_attention_backward (dQ + dK/dV kernels), 10 * n_q * n_keys * 64 flops per (frame, head)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gava_clip_amd import hip  # noqa: E402


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels(BT=512, heads=16, n=257, G=8):
    D = heads * 64
    for T in (32, 64):
        keys = n + G + T + 1
        g = torch.Generator().manual_seed(T)
        qkv = (torch.randn(BT * n, 3 * D, generator=g) * 0.5).cuda().half()
        side = torch.randn(G + 2 * BT, 2 * D, generator=g).cuda().half()
        out = torch.empty(BT * n, D, dtype=torch.float16, device="cuda")
        f = lambda: hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=BT, heads=heads, n_q=n, n_kmain=n,
                                  prec=hip.PREC_F16, side_k=side[:, :D], side_v=side[:, D:], n_g=G, T=T, has_summary=True)
        ms = timed(f)
        fl = 4.0 * n * keys * 64 * BT * heads
        print(json.dumps(dict(what="attention_fwd", keys=keys, n_q=n, frames=BT, heads=heads,
                              kernel="streaming" if keys > 320 else "single-pass", ms=round(ms, 4), tflops=round(fl / ms / 1e9, 1))))
        qb, sb = qkv.bfloat16(), side.bfloat16()
        do = torch.randn(BT * n, D, generator=g).cuda().bfloat16()
        dqkv = torch.empty(BT * n, 3 * D, dtype=torch.bfloat16, device="cuda")
        part = torch.empty(BT * (G + T + 1), 2 * D, dtype=torch.float32, device="cuda")
        fb = lambda: hip.attention_backward(qb[:, :D], qb[:, D:2 * D], qb[:, 2 * D:], do, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                                            batch=BT, heads=heads, n=n, prec=hip.PREC_BF16, q_scale=0.125, side_k=sb[:, :D], side_v=sb[:, D:],
                                            dside_k=part[:, :D], dside_v=part[:, D:], n_g=G, T=T, has_summary=True)
        ms = timed(fb, reps=10)
        fl = 10.0 * n * keys * 64 * BT * heads
        print(json.dumps(dict(what="attention_bwd", keys=keys, n_q=n, frames=BT, heads=heads,
                              kernel="streaming dQ" if keys > 320 else "single-pass", ms=round(ms, 4), tflops=round(fl / ms / 1e9, 1))))


def e2e():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from helpers import CLASSES_3, model_kwargs, synth_torch_state
    from gava_clip_amd import VitaCLIP, synth
    from gava_clip_amd.config import VIT_B16_T8, VIT_B16_T128, VIT_L14_T32, VIT_L14_T64
    for name, cfg, B in (("vit_b16_t8", VIT_B16_T8, 64), ("vit_b16_t128", VIT_B16_T128, 4),
                         ("vit_l14_t32", VIT_L14_T32, 4), ("vit_l14_t64", VIT_L14_T64, 2)):
        m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
        m.load_state_dict(synth_torch_state(cfg, 3, 0), strict=True)
        m = m.cuda().eval()
        x = torch.from_numpy(synth.synth_clip(B, cfg.num_frames, cfg.input_size, seed=1)).cuda()
        with torch.no_grad():
            ms = timed(lambda: m(x), reps=5, warm=2)
        print(json.dumps(dict(what="forward", config=name, clips=B, frames=B * cfg.num_frames, keys=cfg.attn_keys(),
                              ms=round(ms, 3), clips_per_s=round(1000 * B / ms, 1))))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    kernels()
    if "--e2e" in sys.argv:
        e2e()
