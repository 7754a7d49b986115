"""RandAugment on the device: the reference's auto_augment step (video_dataset/dataset.py:98-108, transform.py:625-658,
rand_augment.py), which upstream runs through Pillow on the host between the frame draw and random_resized_crop.

RandAugment parses the config string and draws a video's policy on the host with the generator calls the reference makes, in
its order, so seeding `random` and `np.random` reproduces a reference run; the pixels are the work of gava_augment_hist /
gava_augment_luts / gava_augment_apply (csrc/augment.hip): uint8 [T, H, W, 3] in, uint8 [T, H, W, 3] out, Pillow's bytes.
AugmentedClipPreprocessor is TrainClipPreprocessor with that step in front: its clip descriptors point at the augmented
frames, so batch(), __call__ and VitaCLIP.forward_frames work as they do without augmentation.

Nothing here imports Pillow, and nothing waits for the device.
"""
import math
import random
import re

import numpy as np
import torch

from . import hip
from .preprocess import CLIP_MEAN, CLIP_STD, TrainClipPreprocessor

BILINEAR, BICUBIC = 2, 3            # Pillow's filter codes, as a plan records them
_MAX_LEVEL = 10.0

_RAND = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
         "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
_INCREASING = {"Posterize", "Solarize", "Color", "Contrast", "Brightness", "Sharpness"}
_RAND_INCREASING = tuple(n + "Increasing" if n in _INCREASING else n for n in _RAND)
# rand_augment.py:430-446, in _RAND's order
_WEIGHTS_0 = (0.025, 0.005, 0, 0.3, 0, 0.005, 0.005, 0.025, 0.005, 0.005, 0.025, 0.2, 0.2, 0.1, 0.1)
_GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "TranslateX", "TranslateY")
_TABLE_OPS = {"Invert": hip.AUG_INVERT, "Posterize": hip.AUG_POSTERIZE, "Solarize": hip.AUG_SOLARIZE,
              "SolarizeAdd": hip.AUG_SOLARIZE_ADD, "Brightness": hip.AUG_BRIGHTNESS, "Contrast": hip.AUG_CONTRAST,
              "AutoContrast": hip.AUG_AUTOCONTRAST, "Equalize": hip.AUG_EQUALIZE}
_STATS_OPS = (hip.AUG_CONTRAST, hip.AUG_AUTOCONTRAST, hip.AUG_EQUALIZE)


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def _level_arg(name, level, translate_const):
    """the level functions of rand_augment.py:205-311; the sign is drawn where the reference draws it"""
    if name in ("AutoContrast", "Equalize", "Invert"):
        return None
    frac = level / _MAX_LEVEL
    if name == "Rotate":
        return _randomly_negate(frac * 30.0)
    if name in ("ShearX", "ShearY"):
        return _randomly_negate(frac * 0.3)
    if name in ("TranslateXRel", "TranslateYRel"):
        return _randomly_negate(frac * 0.45)
    if name in ("TranslateX", "TranslateY"):
        return _randomly_negate(frac * float(translate_const))
    if name == "Posterize":
        return int(frac * 4)
    if name == "PosterizeIncreasing":
        return 4 - int(frac * 4)
    if name == "Solarize":
        return int(frac * 256)
    if name == "SolarizeIncreasing":
        return 256 - int(frac * 256)
    if name == "SolarizeAdd":
        return int(frac * 110)
    if name.endswith("Increasing"):                 # Color, Contrast, Brightness, Sharpness: away from 1.0
        return 1.0 + _randomly_negate(frac * 0.9)
    return frac * 1.8 + 0.1


def _rotate_matrix(degrees, W, H):
    """Image.rotate's inverse matrix about the centre; None for the copy it returns at a zero angle"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _matrix(name, arg, W, H):
    if name == "Rotate":
        return _rotate_matrix(arg, W, H)
    if name == "ShearX":
        return (1, arg, 0, 0, 1, 0)
    if name == "ShearY":
        return (1, 0, 0, arg, 1, 0)
    if name in ("TranslateXRel", "TranslateX"):
        return (1, 0, arg * W if name.endswith("Rel") else arg, 0, 1, 0)
    return (1, 0, 0, 0, 1, arg * H if name.endswith("Rel") else arg)


class RandAugment:
    """rand_augment_transform(config_str, hparams) as create_random_augment sets it up (transform.py:625-658): fill colour
    (128, 128, 128), `interpolation` "bicubic" (upstream's default), "bilinear" (and any other name but the refused ones, as
    upstream's _pil_interp maps them) or "random" (every frame of every geometric op draws one of the two).

    Config sections after "rand", in any order: m<int> magnitude, n<int> layers, mstd<float> magnitude noise, inc<x> the
    increasing-severity op list (any value switches it on, "inc0" too: upstream tests bool() of the string), w<int> the choice
    weights (only 0 exists).  Sections with other keys are ignored, as upstream ignores them."""

    def __init__(self, config_str, interpolation="bicubic"):
        if interpolation in ("lanczos", "hamming"):
            raise ValueError(f"interpolation {interpolation!r}: Pillow's Image.transform refuses that filter (use bicubic, bilinear or random)")
        if not isinstance(config_str, str) or config_str.split("-")[0] != "rand":
            raise ValueError(f"auto_augment {config_str!r}: only 'rand-...' policies exist upstream")
        self.config_str, self.interpolation = config_str, interpolation
        self.magnitude, self.num_layers, self.magnitude_std, self.weight_idx = _MAX_LEVEL, 2, None, None
        self.names = _RAND
        for section in config_str.split("-")[1:]:
            cs = re.split(r"(\d.*)", section)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            try:
                if key == "mstd":
                    self.magnitude_std = float(val) if self.magnitude_std is None else self.magnitude_std     # setdefault
                elif key == "inc":
                    self.names = _RAND_INCREASING
                elif key == "m":
                    self.magnitude = int(val)
                elif key == "n":
                    self.num_layers = int(val)
                elif key == "w":
                    self.weight_idx = int(val)
            except ValueError:
                raise ValueError(f"auto_augment {config_str!r}: cannot read the number in section {section!r}") from None
        if self.weight_idx not in (None, 0):
            raise ValueError(f"auto_augment {config_str!r}: only the choice weights w0 exist")
        if self.num_layers < 0:
            raise ValueError(f"auto_augment {config_str!r}: n must not be negative")
        self.choice_weights = None
        if self.weight_idx is not None:
            p = list(_WEIGHTS_0)
            self.choice_weights = p / np.sum(p)
            if self.num_layers > np.count_nonzero(self.choice_weights):
                raise ValueError(f"auto_augment {config_str!r}: weighted choice is without replacement, n is past the ops with a weight")

    # ---- the draw (host) -------------------------------------------------------------------------
    def _draw_op(self, name, T, translate_const, prob=0.5):
        """AugmentOp.__call__ (rand_augment.py:369-387): skip, magnitude noise, level (sign), then per frame the filter"""
        if prob < 1.0 and random.random() > prob:
            return None
        magnitude = self.magnitude
        if self.magnitude_std and self.magnitude_std > 0:
            magnitude = random.gauss(magnitude, self.magnitude_std)
        magnitude = min(_MAX_LEVEL, max(0, magnitude))
        arg = _level_arg(name, magnitude, translate_const)
        filters = None
        if name in _GEOMETRIC:
            if self.interpolation == "random":
                filters = [random.choice((BILINEAR, BICUBIC)) for _ in range(T)]
            else:
                filters = [BICUBIC if self.interpolation == "bicubic" else BILINEAR] * T
        return name, arg, filters

    def plan(self, T, H, W):
        """One video's policy -> list of applied layers (name, arg, filters): the reference's op name, its level argument
        (None where it takes none), and for geometric ops one Pillow filter code per frame (else None).  Ops the draw
        skipped are not in the list."""
        picked = np.random.choice(np.arange(len(self.names)), self.num_layers, replace=self.choice_weights is None, p=self.choice_weights)
        translate_const = int(min(H, W) * 0.45)
        layers = [self._draw_op(self.names[int(k)], T, translate_const) for k in picked]
        return [layer for layer in layers if layer is not None]

    # ---- the pixels (device) ---------------------------------------------------------------------
    @staticmethod
    def _rows(layer, T, H, W):
        """a layer as T gava_augment_desc rows without pointers and slots; None where the layer copies the frames"""
        name, arg, filters = layer
        base = name.replace("Increasing", "")
        rows = np.zeros(T, dtype=hip.augment_desc_dtype())
        rows["H"], rows["W"], rows["lut_slot"], rows["hist_slot"] = H, W, -1, -1
        if base in _GEOMETRIC:
            m = _matrix(base, arg, W, H)
            if m is None:
                return None
            if filters is None or len(filters) != T or any(f not in (BILINEAR, BICUBIC) for f in filters):
                raise ValueError(f"{name}: a geometric layer needs one filter code (2 bilinear, 3 bicubic) per frame")
            rows["kind"], rows["m"] = hip.AUG_AFFINE, np.asarray(m, dtype=np.float64)
            rows["filter"] = [hip.AUG_BICUBIC if f == BICUBIC else hip.AUG_BILINEAR for f in filters]
        elif base in _TABLE_OPS:
            if base == "Posterize" and arg >= 8:
                return None
            rows["kind"], rows["op"] = hip.AUG_TABLE, _TABLE_OPS[base]
            if base in ("Posterize", "Solarize", "SolarizeAdd"):
                rows["iarg"] = int(arg)
            elif base in ("Brightness", "Contrast"):
                rows["factor"] = np.float32(arg)
        elif base in ("Color", "Sharpness"):
            rows["kind"], rows["factor"] = hip.AUG_COLOR if base == "Color" else hip.AUG_SHARPNESS, np.float32(arg)
        else:
            raise ValueError(f"unknown augmentation op {name!r}")
        return rows

    def _run(self, videos, idx, plans):
        """-> one entry per video: the augmented uint8 [T, H, W, 3] tensor, or None where no layer changes the clip (the
        source video with its frame indices is then the result, and nothing was copied).  Layer 1 reads the source frames
        at their indices; later layers go back and forth between two arenas; every layer is at most three launches for the
        whole batch."""
        if not (len(videos) == len(idx) == len(plans)):
            raise ValueError("apply takes one frame index list and one plan per video")
        dev = videos[0].device
        clips, total = [], 0
        for b, (v, ix, plan) in enumerate(zip(videos, idx, plans)):
            if not v.is_cuda or v.device != dev:
                raise hip.GavaError("RandAugment takes device tensors on one device (no CPU fallback)")
            if v.dtype != torch.uint8 or v.dim() != 4 or v.shape[-1] != 3 or 0 in v.shape or not v.is_contiguous():
                raise ValueError("videos must be contiguous uint8 [n_frames, H, W, 3]")
            n, H, W = v.shape[:3]
            ix = [int(i) for i in ix]
            if any(i < 0 or i >= n for i in ix) or not ix:
                raise ValueError("a frame index lies outside its video")
            layers = [r for r in (self._rows(layer, len(ix), H, W) for layer in plan) if r is not None]
            if layers:
                clips.append((b, v, ix, layers, total))
                total += (len(ix) * H * W * 3 + 15) // 16 * 16
        out = [None] * len(videos)
        if not clips:
            return out
        depth = max(len(c[3]) for c in clips)
        arenas = [torch.empty(total, dtype=torch.uint8, device=dev) for _ in range(min(depth, 2))]
        per_layer = [[c for c in clips if len(c[3]) > l] for l in range(depth)]
        n_luts = max(sum(len(c[2]) for c in cs if c[3][l]["kind"][0] == hip.AUG_TABLE) for l, cs in enumerate(per_layer))
        n_hist = max(sum(len(c[2]) for c in cs if c[3][l]["kind"][0] == hip.AUG_TABLE and c[3][l]["op"][0] in _STATS_OPS)
                     for l, cs in enumerate(per_layer))
        luts = torch.empty(n_luts, 3, 256, dtype=torch.uint8, device=dev) if n_luts else None
        hist = torch.zeros(n_hist, 4, 256, dtype=torch.int32, device=dev) if n_hist else None
        for l, cs in enumerate(per_layer):
            tables, lut_slot, hist_slot = [], 0, 0
            for b, v, ix, layers, off in cs:
                rows, T = layers[l], len(ix)
                frame = v.shape[1] * v.shape[2] * 3
                steps = np.arange(T, dtype=np.uint64) * np.uint64(frame)
                if l == 0:
                    rows["src"] = np.uint64(v.data_ptr()) + np.asarray(ix, dtype=np.uint64) * np.uint64(frame)
                else:
                    rows["src"] = np.uint64(arenas[(l - 1) % 2].data_ptr() + off) + steps
                rows["dst"] = np.uint64(arenas[l % 2].data_ptr() + off) + steps
                if rows["kind"][0] == hip.AUG_TABLE:
                    rows["lut_slot"] = np.arange(lut_slot, lut_slot + T)
                    lut_slot += T
                    if rows["op"][0] in _STATS_OPS:
                        rows["hist_slot"] = np.arange(hist_slot, hist_slot + T)
                        hist_slot += T
                tables.append(rows)
            hip.augment_layer(np.concatenate(tables), hist, luts, dev)
        for b, v, ix, layers, off in clips:
            T, H, W = len(ix), v.shape[1], v.shape[2]
            out[b] = arenas[(len(layers) - 1) % 2][off:off + T * H * W * 3].view(T, H, W, 3)
        return out

    def apply(self, videos, idx, plans):
        """videos: list of contiguous uint8 device tensors [n_i, H_i, W_i, 3]; idx: the T drawn frame indices of each; plans:
        one plan() per video -> list of uint8 [T, H_i, W_i, 3] device tensors, the frames after their video's policy."""
        out = self._run(videos, idx, plans)
        for b, (v, ix) in enumerate(zip(videos, idx)):
            if out[b] is None:          # no layer changed this clip: its frames as they are
                out[b] = v.index_select(0, torch.as_tensor([int(i) for i in ix], dtype=torch.long, device=v.device))
        return out


class AugmentedClipPreprocessor(TrainClipPreprocessor):
    """Mirror of VideoDataset(random_sample=True, auto_augment=<config>, ...) (dataset.py:93-114): TrainClipPreprocessor with
    the reference's RandAugment step between the frame draw and the crop, on the device.  sample() draws in the reference's
    order - frame indices, the policy, the crop box - so seeding `random` and `np.random` reproduces a reference item."""

    def __init__(self, auto_augment, num_frames=8, sampling_rate=1, spatial_size=224, mean=CLIP_MEAN, std=CLIP_STD,
                 interpolation="bicubic", mirror=False):
        if auto_augment is None:
            raise ValueError("AugmentedClipPreprocessor needs an auto_augment config string (TrainClipPreprocessor is the same "
                             "data path without augmentation)")
        super().__init__(num_frames=num_frames, sampling_rate=sampling_rate, spatial_size=spatial_size, mean=mean, std=std,
                         interpolation=interpolation, mirror=mirror)
        self.augment = RandAugment(auto_augment, interpolation)
        self.auto_augment = auto_augment

    def sample(self, n_frames, height, width):
        """One draw -> (idx, i, j, h, w, plan)"""
        idx = self._frame_indices(n_frames)
        plan = self.augment.plan(len(idx), height, width)
        return (idx, *self._box(height, width), plan)

    def descriptors(self, videos, draws=None):
        """Runs the augmentation, then -> (device array of gava_clip_desc over the augmented frames, keep-alive list).  draws:
        one (idx, i, j, h, w, plan) per video, default: sample() per video, in batch order.  A clip whose plan changes
        nothing keeps pointing at its source video with its frame table."""
        if draws is None:
            draws = [self.sample(v.shape[0], v.shape[1], v.shape[2]) for v in videos]
        if len(draws) != len(videos) or any(len(d) != 6 or len(d[0]) != self.num_frames for d in draws):
            raise ValueError("draws must hold one (idx, i, j, h, w, plan) per video, each with num_frames frame indices")
        augmented = self.augment._run(videos, [d[0] for d in draws], [d[5] for d in draws])
        frames = [v if a is None else a for v, a in zip(videos, augmented)]
        boxes = [(d[0] if a is None else range(self.num_frames), *d[1:5]) for d, a in zip(draws, augmented)]
        return hip.clip_descriptors_box(frames, boxes, size=self.spatial_size)
