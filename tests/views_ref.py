"""TEST INFRASTRUCTURE ONLY - CPU restatement of the reference's evaluation preprocessing with EVERY view kept.

The torch calls of oracle/preprocess_oracle.py (video_dataset/dataset.py:117-136,160-199): float()/255, (x-mean)/std, permute
to (C,T,H,W), F.interpolate(bilinear, align_corners=False) of all frames to the short-side size, the spatial crops, the
last-frame padding and the temporal crops - returning the whole list upstream builds at :135-136 (spatial-major) instead of
`crops[0]`.  `view_offsets` is the crop bookkeeping on its own: (t_st, h_st, w_st) of every view, which `preprocess_views`
slices by.  PINNED: tests/golden/preprocess_views_ref.npz holds what the reference's own VideoDataset code builds for six
synthetic videos (tools/gen_golden_views.py); tests/test_views_host.py requires this file to reproduce every view bit for
bit.  Imported by tests/ only.
"""
import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
VIDEO_SEED = 9000            # the fixture's video of case i is video(n, h, w, VIDEO_SEED + i)
SAMPLE = 1024                # values of the strided sample kept per view


def video(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8))


def sample(a):
    """the strided sample of a view the fixture stores next to its sha256"""
    return a.reshape(-1)[::max(1, a.size // SAMPLE)][:SAMPLE]


def resized_size(h, w, spatial_size):
    """dataset.py:124-129"""
    if h < w:
        return spatial_size, w * spatial_size // h
    return h * spatial_size // w, spatial_size


def view_offsets(n_frames, h, w, num_frames, sampling_rate, spatial_size, num_spatial_views, num_temporal_views):
    """(t_st, h_st, w_st) of every view in upstream's order, view = sv * num_temporal_views + tv"""
    new_h, new_w = resized_size(h, w, spatial_size)
    if num_spatial_views == 1:
        assert min(new_h, new_w) >= spatial_size                              # :180
        spatial = [((new_h - spatial_size) // 2, (new_w - spatial_size) // 2)]   # :181-182
    else:
        assert num_spatial_views == 3 and min(new_h, new_w) == spatial_size   # :186-187
        margin = max(new_h, new_w) - spatial_size
        spatial = [(st, 0) if new_h > new_w else (0, st) for st in (0, margin // 2, margin)]   # :190-195
    seg_len = (num_frames - 1) * sampling_rate + 1                            # :161
    slide_len = max(n_frames, seg_len) - seg_len                              # :162-164 (a short video is padded to seg_len)
    out = []
    for h_st, w_st in spatial:
        for i in range(num_temporal_views):
            st = slide_len // 2 if num_temporal_views == 1 else round(slide_len / (num_temporal_views - 1) * i)   # :168-171
            out.append((st, h_st, w_st))
    return out


def preprocess_views(frames_u8, num_frames, sampling_rate, spatial_size, mean=MEAN, std=STD, num_spatial_views=1,
                     num_temporal_views=1):
    """-> list of num_spatial_views * num_temporal_views contiguous fp32 (3, T, S, S) crops"""
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    frames = torch.as_tensor(frames_u8).float() / 255.                       # :118-119
    frames = (frames - mean) / std                                           # :121
    frames = frames.permute(3, 0, 1, 2)                                      # :122  C, T, H, W
    new_height, new_width = resized_size(frames.size(-2), frames.size(-1), spatial_size)
    frames = torch.nn.functional.interpolate(frames, size=(new_height, new_width), mode='bilinear',
                                             align_corners=False)            # :130-133
    seg_len = (num_frames - 1) * sampling_rate + 1
    if frames.size(1) < seg_len:                                             # :162-163
        frames = torch.cat([frames, frames[:, -1:].repeat(1, seg_len - frames.size(1), 1, 1)], dim=1)
    S = spatial_size
    offsets = view_offsets(frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2], num_frames, sampling_rate, S,
                           num_spatial_views, num_temporal_views)
    return [frames[:, st: st + num_frames * sampling_rate: sampling_rate, h_st:h_st + S, w_st:w_st + S].contiguous()
            for st, h_st, w_st in offsets]
