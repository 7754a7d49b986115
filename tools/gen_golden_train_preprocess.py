#!/usr/bin/env python
"""Generate tests/golden/preprocess_train_ref.npz by running the REFERENCE's random-sample data path in the build container.

Runs only where /root/reference exists (never on the GPU box), like tools/gen_golden.py.  The reference's
``video_dataset.dataset`` is imported with the ``av`` stand-in of gen_golden.run_preprocess_cases (a container that yields
frames carrying synthetic uint8 arrays: decoding is out of scope) and, this time, its REAL ``video_dataset.transform``:
``torchvision`` / ``torchvision.transforms`` / ``torchvision.transforms.functional`` are empty stand-in modules (nothing of
them is touched with auto_augment=None), PIL is installed.  Everything from ``to_rgb().to_ndarray()`` on is upstream's
code: ``VideoDataset(random_sample=True, auto_augment=None, is_train=False)[0]`` (dataset.py:93-114) under seeded
``random`` / ``np.random``.

Per case the file holds data only: the case tuple (n_frames, H, W, T, sampling_rate, size, seed, video seed), the drawn
(idx, i, j, h, w) captured by wrapping the two reference functions, whether the central fallback was taken, the next draw
of both generators after the item (pins their state), the sha256 of the fp32 output and a 4096-value strided sample (the
format of preprocess_ref.npz).

    python tools/gen_golden_train_preprocess.py
"""
import hashlib
import importlib
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

# (n_frames, H, W, T, sampling_rate, size, first seed tried, property the draw must have)
#   any       whatever the seed gives
#   up / down the box upsamples (h, w < size) / downsamples (h, w > size)
#   fallback  all ten attempts fail, the central crop is taken (an elongated frame fails each attempt with p ~ 0.9)
#   corner    the box touches the frame's bottom-right corner (the clamp at the box edge)
CASES = [
    (20, 240, 320, 8, 2, 224, 100, "any"),        # landscape, random start
    (40, 320, 240, 16, 1, 224, 200, "any"),       # portrait, 16 frames
    (12, 256, 256, 8, 1, 224, 300, "any"),        # square
    (10, 120, 160, 8, 1, 224, 400, "up"),         # every box is smaller than 224: upsampling
    (80, 360, 640, 70, 1, 224, 500, "down"),      # the UPDRS shape: 70 frames of 360 x 640, downsampling
    (10, 181, 333, 8, 1, 32, 600, "any"),         # a small crop size, odd frame sizes
    (5, 200, 300, 8, 2, 224, 700, "any"),         # shorter than the segment: the last index repeats, no frame draw
    (37, 240, 320, 8, -1, 224, 800, "any"),       # TSN
    (9, 64, 512, 8, 1, 64, 900, "fallback"),      # elongated: central fallback
    (9, 48, 64, 8, 1, 32, 1000, "corner"),        # box flush with the bottom-right corner
    (30, 512, 64, 16, -1, 96, 1100, "fallback"),  # TSN + fallback, portrait
]


class _CountingRandom:
    """`random` as video_dataset.transform sees it, counting the draws of the box search"""

    def __init__(self):
        self.uniform_calls = self.randint_calls = 0

    def uniform(self, a, b):
        self.uniform_calls += 1
        return random.uniform(a, b)

    def randint(self, a, b):
        self.randint_calls += 1
        return random.randint(a, b)

    def __getattr__(self, name):
        return getattr(random, name)


def import_reference(videos):
    class _Frame:
        def __init__(self, arr, pts):
            self.arr, self.pts = arr, pts

        def to_rgb(self):
            return self

        def to_ndarray(self):
            return self.arr

    class _Container:
        def __init__(self, path):
            self.frames = videos[os.path.basename(path)]

        def decode(self, video=0):
            for i in range(self.frames.shape[0] - 1, -1, -1):      # out of order on purpose: the reference sorts by pts
                yield _Frame(self.frames[i], 40 * i)

        def close(self):
            pass

    av = types.ModuleType("av")
    av.open = lambda path: _Container(path)
    sys.modules["av"] = av
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    sys.modules["torchvision.transforms.functional"] = tv.transforms.functional
    pkg = types.ModuleType("video_dataset")
    pkg.__path__ = [os.path.join(REF, "video_dataset")]
    sys.modules["video_dataset"] = pkg
    ds_mod = importlib.import_module("video_dataset.dataset")
    tr_mod = importlib.import_module("video_dataset.transform")
    assert ds_mod.__file__.startswith(REF) and tr_mod.__file__.startswith(REF)
    assert ds_mod.random_resized_crop is tr_mod.random_resized_crop
    return ds_mod, tr_mod


def main():
    videos = {}
    ds_mod, tr_mod = import_reference(videos)
    counter = _CountingRandom()
    tr_mod.random = counter
    drawn = {}
    box_fn, idx_fn = tr_mod._get_param_spatial_crop, ds_mod.VideoDataset._random_sample_frame_idx

    def box_wrapped(*a, **k):
        drawn["box"] = box_fn(*a, **k)
        return drawn["box"]

    def idx_wrapped(self, n):
        drawn["idx"] = idx_fn(self, n)
        return drawn["idx"]

    tr_mod._get_param_spatial_crop = box_wrapped
    ds_mod.VideoDataset._random_sample_frame_idx = idx_wrapped

    mean, std = torch.tensor(MEAN), torch.tensor(STD)
    out, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for c, (n, h, w, T, rate, size, seed0, want) in enumerate(CASES):
            vseed = 7000 + c
            videos[f"v{c}.mp4"] = np.random.default_rng(vseed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
            lst = os.path.join(tmp, f"list{c}.csv")
            with open(lst, "w") as f:
                f.write(f"v{c}.mp4,{c % 3}\n")
            ds = ds_mod.VideoDataset(list_path=lst, data_root=tmp, num_spatial_views=1, num_temporal_views=1, random_sample=True,
                                     num_frames=T, sampling_rate=rate, spatial_size=size, mean=mean, std=std,
                                     auto_augment=None, is_train=False)
            for seed in range(seed0, seed0 + 400):      # a seed search for the wanted property: the draw alone, no pixels
                random.seed(seed)
                np.random.seed(seed)
                counter.uniform_calls = counter.randint_calls = 0
                ds._random_sample_frame_idx(n)
                i, j, bh, bw = tr_mod._get_param_spatial_crop((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), h, w)
                fallback = counter.randint_calls == 0
                if {"any": not fallback, "up": bh < size and bw < size and not fallback,
                    "down": bh > size and bw > size and not fallback, "fallback": fallback,
                    "corner": i + bh == h and j + bw == w and (bh < h or bw < w) and not fallback}[want]:
                    break
            else:
                raise SystemExit(f"case {c}: no seed in [{seed0}, {seed0 + 400}) gives '{want}'")
            random.seed(seed)
            np.random.seed(seed)
            counter.uniform_calls = counter.randint_calls = 0
            drawn.clear()
            frames, label, name = ds[0]                                   # the reference's own __getitem__
            nxt = np.array([random.random(), np.random.random()])        # the state both generators are left in
            fallback = counter.randint_calls == 0
            if want == "fallback":
                assert fallback and counter.uniform_calls == 20, "the central fallback was not taken"
            assert tuple(frames.shape) == (3, T, size, size) and label == c % 3 and name == f"v{c}"
            idx, (i, j, bh, bw) = drawn["idx"], drawn["box"]
            a = frames.contiguous().numpy()
            cases.append((n, h, w, T, rate, size, seed, vseed))
            out[f"idx_{c}"] = np.array(idx, dtype=np.int64)
            out[f"box_{c}"] = np.array([i, j, bh, bw], dtype=np.int64)
            out[f"fallback_{c}"] = np.array(int(fallback))
            out[f"next_{c}"] = nxt
            out[f"sha256_{c}"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out[f"sample_{c}"] = a.reshape(-1)[::max(1, a.size // 4096)][:4096].copy()
            print("case", c, cases[-1], want, "idx", idx, "box", (i, j, bh, bw), "fallback", fallback,
                  hashlib.sha256(a.tobytes()).hexdigest()[:16])
    out["cases"] = np.array(cases, dtype=np.int64)
    path = os.path.join(REPO, "tests", "golden", "preprocess_train_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
