#!/usr/bin/env python
"""Generate tests/golden/rand_augment_ref.npz by running the REFERENCE's RandAugment step under Pillow in the build container.

Runs only where /root/reference exists (never on the GPU box), like tools/gen_golden_train_preprocess.py, whose ``av`` /
``torchvision`` stand-ins it uses; on top of them ``torchvision.transforms`` gets three few-line stand-ins (ToPILImage, ToTensor,
Compose: what dataset.py:105-107 and transform.py:655 touch).  ``video_dataset.rand_augment`` needs only Pillow, which is
installed, and is the reference's own file.

Two kinds of case, data only:
  op      one AugmentOp(name, prob=1, magnitude, hparams as create_random_augment builds them) on T = 3 frames: every op of
          both lists, both filters, both signs, flat channels, tiny frames, factors inside and outside [0, 1], a magnitude the
          clip to [0, 10] catches
  policy  VideoDataset(random_sample=True, auto_augment=config, interpolation=...)[0] itself under seeded generators
Per case: the case numbers and strings, the plan as it was applied (op names, level arguments, the filter of every frame -
captured by wrapping AugmentOp.__call__, the op functions and _interpolation), the next draw of both generators, the sha256 and a
4096-value strided sample of the augmented uint8 frames, and for policy cases the drawn (idx, box) and the same for the fp32
clip.  The Pillow version is recorded.

    python tools/gen_golden_rand_augment.py
"""
import hashlib
import importlib
import os
import random
import sys
import tempfile

import numpy as np
import PIL
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rand_augment_ref as ref                               # noqa: E402  (the video generator only)
from gen_golden_train_preprocess import MEAN, STD, import_reference      # noqa: E402

T_OP = 3
# (name, magnitude, mstd, interpolation, H, W, first seed tried, sign wanted (+1, -1, 0 = whatever), flat channel or None)
OP_CASES = []
for _name in ref.RAND + [n for n in ref.RAND_INC if n not in ref.RAND]:
    if _name in ref.GEOMETRIC:
        for _interp in ("bilinear", "bicubic"):
            for _sign in (1, -1):
                OP_CASES.append((_name, 7, 0, _interp, 37, 53, 100, _sign, None))
    elif _name.endswith("Increasing") and "Posterize" not in _name and "Solarize" not in _name:
        OP_CASES += [(_name, 6, 0, "bicubic", 37, 53, 200, 1, None), (_name, 6, 0, "bicubic", 37, 53, 200, -1, None)]     # 1.54, 0.46
    else:
        OP_CASES.append((_name, 7, 0, "bicubic", 37, 53, 300, 0, None))
OP_CASES += [
    ("AutoContrast", 5, 0, "bicubic", 37, 53, 400, 0, 1),         # a flat channel: hi == lo, the identity for it
    ("Equalize", 5, 0, "bicubic", 37, 53, 401, 0, 2),             # a flat channel: one non-empty bin
    ("Contrast", 9, 0, "bicubic", 37, 53, 402, 0, 0),
    ("Equalize", 5, 0, "bicubic", 5, 7, 403, 0, None),            # 35 pixels: step == 0
    ("AutoContrast", 5, 0, "bicubic", 5, 7, 404, 0, None),
    ("Sharpness", 2, 0, "bicubic", 2, 5, 405, 0, None),           # no interior for the 3 x 3 filter
    ("Sharpness", 10, 0, "bicubic", 3, 3, 406, 0, None),          # one interior pixel, factor 1.9
    ("Color", 2, 0, "bicubic", 3, 3, 407, 0, None),               # factor 0.46
    ("Brightness", 5, 0, "bicubic", 37, 53, 408, 0, None),        # factor 1.0 exactly
    ("Rotate", 0, 5, "bicubic", 37, 53, 409, -2, None),           # gauss(0, 5) < 0: clipped to 0, Rotate by 0 is a copy
    ("Rotate", 10, 0, "random", 37, 53, 410, 0, None),            # a filter drawn per frame
    ("ShearX", 10, 0, "bicubic", 2, 5, 411, -1, None),
    ("Rotate", 10, 0, "bilinear", 1, 7, 412, 1, None),
    ("TranslateYRel", 10, 0, "bilinear", 64, 64, 413, -1, None),
    ("PosterizeIncreasing", 10, 0, "bicubic", 37, 53, 414, 0, None),      # 0 bits: everything goes to 0
    ("Posterize", 10, 0, "bicubic", 37, 53, 415, 0, None),                # 4 bits
    ("Solarize", 10, 0, "bicubic", 37, 53, 416, 0, None),                 # threshold 256: the identity
    ("SolarizeIncreasing", 10, 0, "bicubic", 37, 53, 417, 0, None),       # threshold 0: the inverse
]
# (config, interpolation, n_frames, H, W, T, sampling_rate, size, first seed tried, property wanted)
POLICY_CASES = [
    ("rand-m7-n4-mstd0.5-inc1", "bicubic", 12, 60, 80, 4, 2, 32, 1000, "full"),       # all four ops applied
    ("rand-m7-n4-mstd0.5-inc1", "bicubic", 9, 37, 53, 3, 1, 96, 1100, "any"),
    ("rand-m9-n2", "bilinear", 12, 60, 80, 4, 2, 32, 1200, "any"),
    ("rand-m9-n2", "bicubic", 12, 60, 80, 4, 2, 32, 1300, "none"),                    # both ops skipped
    ("rand-m5-n3-mstd1-w0", "bicubic", 10, 48, 64, 4, -1, 32, 1400, "any"),           # weighted choice, TSN
    ("rand-m9-n3-mstd0.5-inc0", "random", 12, 60, 80, 4, 2, 32, 1500, "geometric"),   # inc0 switches the list on; drawn filters
]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def sample(a):
    return np.ascontiguousarray(a).reshape(-1)[::max(1, a.size // 4096)][:4096].copy()


def install_transforms():
    tv = sys.modules["torchvision.transforms"]

    class ToPILImage:
        def __call__(self, t):                               # float CHW in [0, 1] -> mul(255).byte(), as torchvision does
            return Image.fromarray(t.mul(255).byte().permute(1, 2, 0).contiguous().numpy())

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            TRACE["frames"] = np.stack([np.asarray(im) for im in x])
            return x

    tv.ToPILImage, tv.ToTensor, tv.Compose = ToPILImage, ToTensor, Compose


TRACE = {"layers": [], "fresh": False, "op": None, "frames": None}


def instrument(ra):
    """record what is applied: the op's name and level arguments at its first frame, the filter of every frame"""
    init, call, interp = ra.AugmentOp.__init__, ra.AugmentOp.__call__, ra._interpolation

    def init_named(self, name, *a, **k):
        init(self, name, *a, **k)
        self.name = name

    def call_traced(self, img_list):
        TRACE["fresh"], TRACE["op"] = True, self
        return call(self, img_list)

    def interp_traced(kwargs):
        f = interp(kwargs)
        TRACE["layers"][-1][2].append(int(f))
        return f

    def wrap(fn):
        def traced(img, *level_args, **kwargs):
            if TRACE["fresh"]:
                TRACE["layers"].append([TRACE["op"].name, level_args[0] if level_args else None, []])
                TRACE["fresh"] = False
            return fn(img, *level_args, **kwargs)
        return traced

    ra.AugmentOp.__init__, ra.AugmentOp.__call__, ra._interpolation = init_named, call_traced, interp_traced
    for k in list(ra.NAME_TO_OP):
        ra.NAME_TO_OP[k] = wrap(ra.NAME_TO_OP[k])


def store_plan(out, c, T):
    layers = TRACE["layers"]
    out[f"plan_names_{c}"] = np.array([l[0] for l in layers], dtype="U24")
    out[f"plan_args_{c}"] = np.array([np.nan if l[1] is None else float(l[1]) for l in layers], dtype=np.float64)
    out[f"plan_filters_{c}"] = np.array([l[2] if l[2] else [-1] * T for l in layers], dtype=np.int64).reshape(len(layers), T)


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def main():
    videos = {}
    ds_mod, tr_mod = import_reference(videos)
    install_transforms()
    ra = importlib.import_module("video_dataset.rand_augment")
    assert ra.__file__.startswith("/root/reference") and tr_mod.rand_augment_transform is ra.rand_augment_transform
    instrument(ra)
    out, c = {"pillow": np.array(PIL.__version__)}, 0

    for name, mag, mstd, interp, H, W, seed0, sign, flat in OP_CASES:
        hparams = {"translate_const": int(min(H, W) * 0.45)}
        if interp != "random":
            hparams["interpolation"] = tr_mod._pil_interp(interp)
        if mstd:
            hparams["magnitude_std"] = mstd
        op = ra.AugmentOp(name, prob=1.0, magnitude=mag, hparams=hparams)
        vseed = 9000 + c
        frames = ref.video(T_OP, H, W, vseed, flat)
        imgs = [Image.fromarray(f) for f in frames]
        for seed in range(seed0, seed0 + 400):
            seed_all(seed)
            TRACE["layers"].clear()
            res = op(list(imgs))
            arg = TRACE["layers"][0][1]
            if sign == 0 or (sign == -2 and arg == 0) or (sign in (1, -1) and arg is not None and
                                                          math_sign(arg if "Increasing" not in name else arg - 1.0) == sign):
                break
        else:
            raise SystemExit(f"op case {c} ({name}): no seed gives the wanted sign")
        nxt = np.array([random.random(), np.random.random()])
        got = np.stack([np.asarray(im) for im in res])
        out[f"case_{c}"] = np.array([0, T_OP, H, W, T_OP, 1, 0, seed, vseed, -1 if flat is None else flat], dtype=np.int64)
        out[f"cfg_{c}"] = np.array([name, interp], dtype="U32")
        out[f"mag_{c}"] = np.array([mag, mstd], dtype=np.float64)
        store_plan(out, c, T_OP)
        out[f"next_{c}"], out[f"sha256_{c}"], out[f"sample_{c}"] = nxt, sha(got), sample(got)
        print("op", c, name, mag, mstd, interp, (H, W), "seed", seed, "arg", arg, TRACE["layers"][0][2],
              "changed", int((got != frames).sum()))
        c += 1

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
    with tempfile.TemporaryDirectory() as tmp:
        for cfg, interp, n, H, W, T, rate, size, seed0, want in POLICY_CASES:
            vseed = 9000 + c
            videos[f"v{c}.mp4"] = ref.video(n, H, W, vseed)
            lst = os.path.join(tmp, f"list{c}.csv")
            with open(lst, "w") as f:
                f.write(f"v{c}.mp4,{c % 3}\n")
            ds = ds_mod.VideoDataset(list_path=lst, data_root=tmp, num_spatial_views=1, num_temporal_views=1, random_sample=True,
                                     num_frames=T, sampling_rate=rate, spatial_size=size, mean=mean, std=std,
                                     auto_augment=cfg, interpolation=interp, is_train=False)
            for seed in range(seed0, seed0 + 400):
                seed_all(seed)
                TRACE["layers"].clear()
                clip, label, name = ds[0]
                nxt = np.array([random.random(), np.random.random()])
                names = [l[0] for l in TRACE["layers"]]
                if {"any": len(names) >= 1, "none": len(names) == 0, "full": len(names) == 4,
                    "geometric": sum(nm in ref.GEOMETRIC for nm in names) >= 2}[want]:
                    break
            else:
                raise SystemExit(f"policy case {c}: no seed gives '{want}'")
            assert tuple(clip.shape) == (3, T, size, size)
            a = clip.contiguous().numpy()
            out[f"case_{c}"] = np.array([1, n, H, W, T, rate, size, seed, vseed, -1], dtype=np.int64)
            out[f"cfg_{c}"] = np.array([cfg, interp], dtype="U32")
            out[f"mag_{c}"] = np.array([np.nan, np.nan])
            store_plan(out, c, T)
            out[f"idx_{c}"] = np.array(drawn["idx"], dtype=np.int64)
            out[f"box_{c}"] = np.array(drawn["box"], dtype=np.int64)
            out[f"next_{c}"], out[f"sha256_{c}"], out[f"sample_{c}"] = nxt, sha(TRACE["frames"]), sample(TRACE["frames"])
            out[f"clip_sha256_{c}"], out[f"clip_sample_{c}"] = sha(a), sample(a)
            print("policy", c, cfg, interp, "seed", seed, "idx", drawn["idx"], "box", drawn["box"],
                  [(l[0], l[1], l[2]) for l in TRACE["layers"]])
            c += 1
    out["n_cases"] = np.array(c)
    path = os.path.join(REPO, "tests", "golden", "rand_augment_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


def math_sign(v):
    return 1 if v > 0 else (-1 if v < 0 else 0)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
