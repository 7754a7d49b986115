#!/usr/bin/env python
"""Generate tests/golden/preprocess_views_ref.npz: EVERY spatial x temporal evaluation crop the REFERENCE builds.

Runs only where /root/reference exists (never on the GPU box), like tools/gen_golden_train_preprocess.py, and imports the
reference's ``video_dataset.dataset`` with the same stand-ins (``av``: a container that yields frames carrying synthetic
uint8 arrays; ``torchvision`` and the augmentation module: empty, the evaluation branch never touches them).  Per case the
reference's own ``VideoDataset.__getitem__`` runs (dataset.py:117-139); it keeps only ``frames[0]``, so the dataset's own
``_generate_temporal_crops`` is wrapped to record every list it returns: their concatenation, in call order, is the list of
:135-136 (spatial-major).  Nothing of the pixel path is restated here.

The file holds data only: the case table (n_frames, H, W, T, sampling_rate, size, spatial views, temporal views) and, per
view, the sha256 of the fp32 bytes and a strided sample of at most 1024 values.  The video of case i is
``rng.integers(0, 256, (n, H, W, 3), uint8)`` with ``np.random.default_rng(9000 + i)`` (tests/views_ref.py::video).

    python tools/gen_golden_views.py
"""
import hashlib
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
from views_ref import MEAN, STD, VIDEO_SEED, sample, video   # noqa: E402  (seed, sample format and statistics only)

# (n_frames, H, W, T, sampling_rate, size, spatial views, temporal views)
CASES = [
    (13, 40, 56, 4, 2, 32, 3, 3),       # landscape; slide_len 6
    (9, 56, 40, 4, 1, 32, 3, 2),        # portrait: the crops move along H
    (12, 48, 48, 4, 2, 32, 3, 4),       # square: three equal spatial views; slide_len 5 over 4 views, steps of 5/3
    (3, 40, 56, 4, 2, 32, 1, 5),        # shorter than seg_len: every temporal view is the padded clip
    (12, 40, 57, 4, 2, 32, 1, 3),       # slide_len 5, step 2.5: round(2.5) == 2
    (30, 240, 320, 8, 2, 224, 3, 10),   # the loader's default counts, one full-size case
]


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
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    pkg = types.ModuleType("video_dataset")
    pkg.__path__ = [os.path.join(REF, "video_dataset")]
    sys.modules["video_dataset"] = pkg
    tr = types.ModuleType("video_dataset.transform")
    tr.create_random_augment = tr.random_resized_crop = None
    sys.modules["video_dataset.transform"] = tr
    ds_mod = importlib.import_module("video_dataset.dataset")
    assert ds_mod.__file__.startswith(REF)
    return ds_mod


def main():
    videos = {}
    ds_mod = import_reference(videos)
    mean, std = torch.tensor(MEAN), torch.tensor(STD)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        for c, (n, h, w, T, rate, size, sv, tvw) in enumerate(CASES):
            videos[f"v{c}.mp4"] = video(n, h, w, VIDEO_SEED + c).numpy()
            lst = os.path.join(tmp, f"list{c}.csv")
            with open(lst, "w") as f:
                f.write(f"v{c}.mp4,{c % 3}\n")
            ds = ds_mod.VideoDataset(list_path=lst, data_root=tmp, num_spatial_views=sv, num_temporal_views=tvw, random_sample=False,
                                     num_frames=T, sampling_rate=rate, spatial_size=size, mean=mean, std=std, is_train=False)
            views, temporal = [], ds._generate_temporal_crops

            def recording(x):
                crops = temporal(x)
                views.extend(crops)
                return crops

            ds._generate_temporal_crops = recording
            first, label, name = ds[0]                              # the reference's own __getitem__
            assert len(views) == sv * tvw and label == c % 3 and name == f"v{c}"
            assert torch.equal(first, views[0])                     # what upstream returns is view 0 of the list
            digests, samples = [], []
            for v in views:
                assert tuple(v.shape) == (3, T, size, size)
                a = v.contiguous().numpy()
                digests.append(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8))
                samples.append(sample(a).copy())
            out[f"sha256_{c}"] = np.stack(digests)
            out[f"sample_{c}"] = np.stack(samples)
            print("case", c, CASES[c], len(views), "views", hashlib.sha256(out[f"sha256_{c}"].tobytes()).hexdigest()[:16])
    path = os.path.join(REPO, "tests", "golden", "preprocess_views_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
