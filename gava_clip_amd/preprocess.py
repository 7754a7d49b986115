"""GPU clip preprocessing: both branches of the reference's VideoDataset.__getitem__ (video_dataset/dataset.py:93-139) from
decoded uint8 frames to the model input, on the device.

ClipPreprocessor is the `random_sample=False` branch (:117-139).  The reference uses it for evaluation AND for training: its
train loader builds the dataset with random_sample=False (video_dataset/dataloader.py:89-102).  On the CPU, inside DataLoader
workers, that branch converts EVERY decoded frame to float, normalises and resizes all of them, centre-crops, and only then
keeps T frames.  Here the uint8 frames go to the GPU as they are (4x fewer PCIe / HBM bytes than fp32) and one HBM-bound
kernel produces the (3, T, size, size) clips of a batch, touching only the T frames the temporal crop keeps.

TrainClipPreprocessor is the `random_sample=True` branch of the upstream Vita-CLIP recipe (:93-114) with auto_augment=None:
random temporal sampling (TSN included) and random_resized_crop (transform.py:503-577).  The random draws are index
arithmetic on the host; normalisation and the bilinear resize of the drawn box run in the same kernels.

Decoding (PyAV) stays on the host.  The recipe's auto-augment step (dataset.py:98-108, Pillow upstream) is
gava_clip_amd.augment.AugmentedClipPreprocessor, a TrainClipPreprocessor with RandAugment on the device in front.
"""
import math
import random

import numpy as np
import torch

from . import hip

# the statistics every eval/train script passes (eval_scripts/eval_updrs.sh:9-10, k400_eval.sh:14-15)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class ClipPreprocessor:
    """Mirror of VideoDataset(random_sample=False, ...) (the evaluation branch, any view counts upstream accepts).

    Same argument names as the reference constructor (dataset.py:23-33) for the ones that matter here.
    """

    def __init__(self, num_frames=8, sampling_rate=1, spatial_size=224, mean=CLIP_MEAN, std=CLIP_STD,
                 num_spatial_views=1, num_temporal_views=1):
        if num_spatial_views not in (1, 3):
            raise NotImplementedError()          # dataset.py:201-202
        # upstream builds all num_spatial_views x num_temporal_views crops but returns only the first one
        # (`frames = frames[0]`, dataset.py:134-139): the top/left spatial crop and the temporal crop starting at frame 0.
        # __call__, batch and descriptors serve that one; view_descriptors / batch_views serve all of them.
        self.num_spatial_views, self.num_temporal_views = num_spatial_views, num_temporal_views
        self.num_frames, self.sampling_rate, self.spatial_size = num_frames, sampling_rate, spatial_size
        self.mean = tuple(float(v) for v in torch.as_tensor(mean).flatten().tolist())
        self.std = tuple(float(v) for v in torch.as_tensor(std).flatten().tolist())
        self._lut = {}

    def lut(self, device):
        """(v/255 - mean) / std for the 256 byte values per channel, the reference's expression evaluated once on the host"""
        if device not in self._lut:
            self._lut[device] = hip.clip_lut(self.mean, self.std, device)
        return self._lut[device]

    def check(self, videos):
        for v in videos:
            self._check(v)

    def _check(self, frames):
        if not frames.is_cuda:
            raise hip.GavaError("ClipPreprocessor takes device tensors (no CPU fallback)")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [n_frames, H, W, 3] (to_rgb().to_ndarray() order)")
        h, w = frames.shape[1], frames.shape[2]
        s = self.spatial_size
        new_h, new_w = (s, w * s // h) if h < w else (h * s // w, s)
        if self.num_spatial_views == 1:
            assert min(new_h, new_w) >= s   # dataset.py:182
        else:
            assert min(new_h, new_w) == s   # dataset.py:189

    def __call__(self, frames, out=None):
        """frames: uint8 [n, H, W, 3] on the GPU -> fp32 [3, T, S, S] (dataset.py returns frames[0] of this shape)."""
        self._check(frames)
        T, S = self.num_frames, self.spatial_size
        if out is None:
            out = torch.empty(3, T, S, S, dtype=torch.float32, device=frames.device)
        hip.preprocess_clip(frames.contiguous(), out, T=T, rate=self.sampling_rate, size=S, mean=self.mean, std=self.std,
                            first_temporal_view=self.num_temporal_views > 1, first_spatial_view=self.num_spatial_views == 3,
                            lut=self.lut(frames.device))
        return out

    def descriptors(self, videos):
        """-> (device array of gava_clip_desc, keep-alive list) for a list of checked videos: what the kernels read."""
        return hip.clip_descriptors(videos, T=self.num_frames, rate=self.sampling_rate, size=self.spatial_size,
                                    first_temporal_view=self.num_temporal_views > 1,
                                    first_spatial_view=self.num_spatial_views == 3)

    def batch(self, videos):
        """list of uint8 [n_i, H_i, W_i, 3] -> fp32 [B, 3, T, S, S]: one launch for the batch (gava_preprocess_clips), videos
        of different sizes included; the same bits as calling the preprocessor clip by clip."""
        return _batch(self, videos, self.descriptors)


    @property
    def num_views(self):
        """crops per video that upstream builds (dataset.py:135-136)"""
        return self.num_spatial_views * self.num_temporal_views

    def view_descriptors(self, videos):
        """-> (device array of B * num_views gava_clip_desc, keep-alive list, host int32 [B * num_views, 3] of (t_st, h_st,
        w_st)): every view of every checked video, video-major, a video's views in upstream's order (spatial-major)."""
        return hip.clip_descriptors_views(videos, T=self.num_frames, rate=self.sampling_rate, size=self.spatial_size,
                                          n_spatial=self.num_spatial_views, n_temporal=self.num_temporal_views)

    def batch_views(self, videos):
        """list of uint8 [n_i, H_i, W_i, 3] -> fp32 [B, V, 3, T, S, S], V = num_views: every crop upstream builds, in its order.
        One gava_preprocess_clips launch, or several where B * V * T passes that kernel's grid bound of 65535 frames."""
        T, S, V = self.num_frames, self.spatial_size, self.num_views
        dev = videos[0].device
        with torch.cuda.device(dev):
            self.check(videos)
            desc, keep, _ = self.view_descriptors([v.contiguous() for v in videos])
            x = torch.empty(len(videos), V, 3, T, S, S, dtype=torch.float32, device=dev)
            flat, stride = x.view(-1, 3, T, S, S), desc.numel() // (len(videos) * V)
            step = hip.MAX_GRID_FRAMES // T
            if step < 1:
                raise hip.GavaError(f"num_frames = {T} is past the {hip.MAX_GRID_FRAMES} frames one launch covers")
            for i in range(0, flat.shape[0], step):
                hip.preprocess_clips(desc[i * stride:(i + step) * stride], flat[i:i + step], T=T, size=S, lut=self.lut(dev))
        return x


def _batch(pre, videos, descriptors):
    T, S = pre.num_frames, pre.spatial_size
    dev = videos[0].device
    with torch.cuda.device(dev):
        pre.check(videos)
        desc, keep = descriptors([v.contiguous() for v in videos])
        x = torch.empty(len(videos), 3, T, S, S, dtype=torch.float32, device=dev)
        hip.preprocess_clips(desc, x, T=T, size=S, lut=pre.lut(dev))
    return x


class TrainClipPreprocessor:
    """Mirror of VideoDataset(random_sample=True, auto_augment=None, ...) (dataset.py:93-114), the upstream Vita-CLIP training
    recipe; argument names as in the reference constructor (dataset.py:23-33).  `mirror` is accepted and ignored, as
    upstream stores and never applies it.  sampling_rate < 0 selects TSN sampling.

    The host draws (frame indices, crop box) with the generators the reference uses, in its order - np.random for the
    frames, Python's random (plus one unused np.random draw per attempt) for the box - so seeding both reproduces a
    reference run; the device normalises and resizes the box to S x S."""

    SCALE = (0.08, 1.0)                 # transform.py:549-550, the defaults dataset.py:112-114 leaves in place
    RATIO = (3.0 / 4.0, 4.0 / 3.0)
    ATTEMPTS = 10

    def __init__(self, num_frames=8, sampling_rate=1, spatial_size=224, mean=CLIP_MEAN, std=CLIP_STD, auto_augment=None,
                 interpolation="bicubic", mirror=False):
        if auto_augment is not None:
            raise NotImplementedError("auto_augment (dataset.py:98-108) is the work of gava_clip_amd.AugmentedClipPreprocessor("
                                      f"{auto_augment!r}, ...), which runs RandAugment on the device; this class is the data path "
                                      "without it")
        self.num_frames, self.sampling_rate, self.spatial_size = num_frames, sampling_rate, spatial_size
        self.mean = tuple(float(v) for v in torch.as_tensor(mean).flatten().tolist())
        self.std = tuple(float(v) for v in torch.as_tensor(std).flatten().tolist())
        self.interpolation, self.mirror = interpolation, mirror       # neither is read without auto_augment upstream
        self._lut = {}

    lut = ClipPreprocessor.lut

    def check(self, videos):
        for v in videos:
            self._check(v)

    def _check(self, frames):
        if not frames.is_cuda:
            raise hip.GavaError("TrainClipPreprocessor takes device tensors (no CPU fallback)")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or 0 in frames.shape:
            raise ValueError("frames must be uint8 [n_frames, H, W, 3] (to_rgb().to_ndarray() order)")

    # ---- the random draws (host) ---------------------------------------------------------------
    def _frame_indices(self, n):
        T, rate = self.num_frames, self.sampling_rate
        if rate < 0:
            # TSN: the video is cut into T equal segments, one frame drawn from each (both rounded ends included)
            seg = (n - 1) / T
            return [int(np.random.randint(round(seg * k), round(seg * (k + 1)) + 1)) for k in range(T)]
        if rate * (T - 1) + 1 >= n:
            # the video is not longer than the strided segment: no draw, stride from frame 0 and repeat the last index reached
            idx = []
            for k in range(T):
                idx.append(k * rate if k * rate < n else idx[-1])
            return idx
        start = int(np.random.randint(n - rate * (T - 1)))
        return [start + k * rate for k in range(T)]

    def _box(self, height, width):
        area = height * width
        log_lo, log_hi = math.log(self.RATIO[0]), math.log(self.RATIO[1])
        for _ in range(self.ATTEMPTS):
            target = random.uniform(*self.SCALE) * area               # area fraction, then a log-uniform aspect ratio
            aspect = math.exp(random.uniform(log_lo, log_hi))
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            np.random.uniform()     # upstream draws its (switched-off) height/width swap here: keeps np.random in step
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
                return i, j, h, w
        # no attempt fitted: the largest centred box whose aspect ratio is inside RATIO
        frame_ratio = float(width) / float(height)
        if frame_ratio < self.RATIO[0]:
            w, h = width, int(round(width / self.RATIO[0]))
        elif frame_ratio > self.RATIO[1]:
            h, w = height, int(round(height * self.RATIO[1]))
        else:
            h, w = height, width
        return (height - h) // 2, (width - w) // 2, h, w

    def sample(self, n_frames, height, width):
        """One draw -> (idx, i, j, h, w): T source frame indices, then the crop box rows i + [0, h), columns j + [0, w)."""
        idx = self._frame_indices(n_frames)
        return (idx, *self._box(height, width))

    # ---- device ---------------------------------------------------------------------------------
    def descriptors(self, videos, draws=None):
        """-> (device array of gava_clip_desc, keep-alive list); draws: one (idx, i, j, h, w) per video, default: sample()
        per video, in batch order."""
        if draws is None:
            draws = [self.sample(v.shape[0], v.shape[1], v.shape[2]) for v in videos]
        if len(draws) != len(videos) or any(len(d[0]) != self.num_frames for d in draws):
            # the kernels read num_frames entries of every clip's frame table
            raise ValueError("draws must hold one (idx, i, j, h, w) per video, each with num_frames frame indices")
        return hip.clip_descriptors_box(videos, draws, size=self.spatial_size)

    def __call__(self, frames, draw=None):
        """frames: uint8 [n, H, W, 3] on the GPU -> fp32 [3, T, S, S]."""
        return self.batch([frames], None if draw is None else [draw])[0]

    def batch(self, videos, draws=None):
        """list of uint8 [n_i, H_i, W_i, 3] -> fp32 [B, 3, T, S, S] in one launch (gava_preprocess_clips)."""
        return _batch(self, videos, lambda vs: self.descriptors(vs, draws))
