"""TEST INFRASTRUCTURE ONLY - CPU restatement, in torch, of the reference's random-sample data path
(video_dataset/dataset.py:93-114 with auto_augment=None, transform.py:503-577).

`preprocess_clip` index-selects the drawn frames, normalises with the reference's expression, slices the box out of the
(C, T, H, W) view and calls F.interpolate(bilinear, align_corners=False).  `draw` restates the parameter draw - written
independently of gava_clip_amd.preprocess.TrainClipPreprocessor.sample, so that the two check each other.  PINNED:
tests/golden/preprocess_train_ref.npz holds what the reference's own VideoDataset.__getitem__ returns for eleven seeded
synthetic videos (tools/gen_golden_train_preprocess.py); tests/test_train_preprocess.py requires this file to reproduce
them bit for bit.  Imported by tests/ only.
"""
import math
import random

import numpy as np
import torch


def video(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8))


def draw_frames(n_frames, T, rate):
    """dataset.py:202-217"""
    if rate < 0:                                             # TSN
        bounds = [round((n_frames - 1) / T * k) for k in range(T + 1)]
        return [int(np.random.randint(lo, hi + 1)) for lo, hi in zip(bounds[:-1], bounds[1:])]
    if rate * (T - 1) + 1 >= n_frames:                       # short video
        last = ((n_frames - 1) // rate) * rate               # the largest multiple of rate below n_frames
        return [min(k * rate, last) for k in range(T)]
    first = int(np.random.randint(n_frames - rate * (T - 1)))
    return list(range(first, first + rate * T, rate))


def draw_box(height, width, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """transform.py:503-542 with its defaults (log_scale=True, switch_hw=False, ten attempts)"""
    attempt = 0
    while attempt < 10:
        attempt += 1
        a = random.uniform(scale[0], scale[1]) * (height * width)
        r = math.exp(random.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(a * r))), int(round(math.sqrt(a / r)))
        np.random.uniform()                                  # the left operand of upstream's `... < 0.5 and switch_hw`
        if w < 1 or h < 1 or w > width or h > height:
            continue
        top = random.randint(0, height - h)
        left = random.randint(0, width - w)
        return top, left, h, w
    whr = float(width) / float(height)
    h, w = height, width
    if whr < min(ratio):
        h = int(round(w / min(ratio)))
    elif whr > max(ratio):
        w = int(round(h * max(ratio)))
    return (height - h) // 2, (width - w) // 2, h, w


def draw(n_frames, height, width, T, rate):
    idx = draw_frames(n_frames, T, rate)
    return (idx, *draw_box(height, width))


def preprocess_clip(frames_u8, idx, i, j, h, w, size, mean, std):
    """uint8 [n, H, W, 3] -> fp32 [3, T, size, size]"""
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    frames = torch.as_tensor(frames_u8).index_select(0, torch.as_tensor(list(idx), dtype=torch.long))
    frames = frames.float() / 255.                                          # dataset.py:96
    frames = (frames - mean) / std                                          # :110
    frames = frames.permute(3, 0, 1, 2)                                     # :111  C, T, H, W
    cropped = frames[:, :, i:i + h, j:j + w]                                # transform.py:571
    return torch.nn.functional.interpolate(cropped, size=(size, size), mode="bilinear", align_corners=False).contiguous()
