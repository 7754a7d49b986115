"""GPU: gava_augment_hist / gava_augment_luts / gava_augment_apply, RandAugment.apply and AugmentedClipPreprocessor against the
numpy restatement (tests/rand_augment_ref.py, pinned to the reference under Pillow by tests/test_rand_augment_host.py): every
comparison is bit for bit.  T = 3 frames unless a fixture case says otherwise."""
import hashlib
import random

import numpy as np
import pytest
import torch

import rand_augment_ref as ref
from helpers import CLASSES_3, mixed_violation, model_kwargs, synth_torch_state
from test_rand_augment_host import MEAN, STD, fixture, source_frames

pytestmark = pytest.mark.gpu
T = 3
SIZES = [(37, 53), (3, 3), (2, 5), (1, 7), (64, 64)]          # odd with unaligned rows; no interior / one interior pixel; a row; aligned


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _run(aug, videos, plans, idx=None):
    dev = torch.device("cuda")
    idx = idx or [list(range(v.shape[0])) for v in videos]
    out = aug.apply([torch.from_numpy(v).to(dev) for v in videos], idx, plans)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(videos, plans, what):
    from gava_clip_amd import RandAugment
    got = _run(RandAugment("rand"), videos, plans)
    for n, (v, plan, g) in enumerate(zip(videos, plans, got)):
        want = ref.apply_plan(v, plan)
        assert g.shape == want.shape and g.dtype == np.uint8
        diff = int((g != want).sum())
        assert diff == 0, (what, n, v.shape, plan, diff)


@pytest.mark.parametrize("H,W", SIZES)
def test_affine_ops_both_filters_both_signs_and_the_identity(H, W):
    v = ref.video(T, H, W, 11)
    plans = []
    for name, mag in (("Rotate", 21.0), ("Rotate", 30.0), ("ShearX", 0.21), ("ShearY", 0.3), ("TranslateXRel", 0.315),
                      ("TranslateYRel", 0.45), ("TranslateX", 2.5), ("TranslateY", 1.25)):
        for sign in (1, -1):
            plans += [[(name, sign * mag, [ref.BILINEAR] * T)], [(name, sign * mag, [ref.BICUBIC] * T)],
                      [(name, sign * mag, [ref.BICUBIC, ref.BILINEAR, ref.BICUBIC])]]
    for f in (ref.BILINEAR, ref.BICUBIC):
        plans += [[("ShearX", 0.0, [f] * T)], [("TranslateYRel", 0.0, [f] * T)], [("Rotate", 360.0, [f] * T)], [("Rotate", 0.0, [f] * T)]]
    _check([v] * len(plans), plans, "affine")


@pytest.mark.parametrize("H,W", SIZES)
def test_blends_and_table_ops_at_their_extremes(H, W):
    v = ref.video(T, H, W, 12)
    plans = [[(name, f, None)] for name in ("Color", "Sharpness", "Brightness", "Contrast") for f in (0.1, 1.0, 1.9, 0.46, 1.54)]
    plans += [[("Invert", None, None)], [("Posterize", 0, None)], [("Posterize", 4, None)], [("Posterize", 1, None)],
              [("PosterizeIncreasing", 8, None)], [("Solarize", 0, None)], [("Solarize", 256, None)], [("Solarize", 179, None)],
              [("SolarizeAdd", 0, None)], [("SolarizeAdd", 110, None)], [("SolarizeAdd", 77, None)]]
    _check([v] * len(plans), plans, "blend/table")


def test_statistics_ops_on_ramps_a_flat_channel_and_tiny_frames():
    videos, plans = [], []
    for H, W in SIZES + [(5, 7), (200, 301)]:       # 5 x 7: Equalize's step is 0; 200 x 301: several slabs per frame in the histogram
        for flat in (None, 0, 2):
            for name, arg in (("AutoContrast", None), ("Equalize", None), ("Contrast", 0.1), ("Contrast", 1.9), ("Contrast", 1.0)):
                videos.append(ref.video(T, H, W, 13, flat))
                plans.append([(name, arg, None)])
    # every pixel one value (a single bin in every channel), and a two-bin frame whose Equalize table passes 255 before the clip
    one = np.full((T, 6, 9, 3), 200, dtype=np.uint8)
    two = np.zeros((T, 40, 40, 3), dtype=np.uint8)
    two[:, :3] = 9
    two[:, 3:, :, 1] = 250
    for v in (one, two):
        for name, arg in (("AutoContrast", None), ("Equalize", None), ("Contrast", 0.5)):
            videos.append(v)
            plans.append([(name, arg, None)])
    _check(videos, plans, "statistics")


def test_one_mixed_batch_twice():
    """clips of different sizes, a different op per clip in a layer, a clip without any op, a clip whose four ops hold two
    statistics ops (their histograms must come from the layer's input, not from the source), frames picked by index"""
    from gava_clip_amd import RandAugment
    videos = [ref.video(7, 37, 53, 21), ref.video(5, 64, 64, 22), ref.video(4, 20, 31, 23, 1), ref.video(6, 48, 80, 24),
              ref.video(3, 2, 5, 25)]
    idx = [[6, 0, 3], [1, 1, 4], [0, 2, 3], [5, 4, 0], [2, 1, 0]]
    plans = [[("Rotate", -17.0, [3, 2, 3]), ("Equalize", None, None), ("ColorIncreasing", 1.54, None), ("AutoContrast", None, None)],
             [("SolarizeAdd", 40, None), ("ShearX", 0.2, [2, 2, 3])],
             [],
             [("ContrastIncreasing", 0.46, None), ("Rotate", 0.0, [3, 3, 3]), ("SharpnessIncreasing", 1.9, None)],
             [("Invert", None, None)]]
    aug = RandAugment("rand-m7-n4-mstd0.5-inc1")
    first = _run(aug, videos, plans, idx)
    again = _run(aug, videos, plans, idx)
    for b, (v, ix, plan) in enumerate(zip(videos, idx, plans)):
        want = ref.apply_plan(v[ix], plan)
        assert np.array_equal(first[b], want), (b, int((first[b] != want).sum()))
        assert np.array_equal(again[b], first[b]), b
    # the statistics of clip 0's second layer are those of the rotated frames: the source's would give another table
    wrong = ref.apply_op(ref.apply_op(videos[0][6], "Rotate", -17.0, 3), "Equalize", None)
    assert not np.array_equal(ref.apply_op(videos[0][6], "Equalize", None), wrong)
    # a clip without an op is not copied: its descriptor keeps the source video and its frame table
    dev = torch.device("cuda")
    vids = [torch.from_numpy(v).to(dev) for v in videos]
    out = aug._run(vids, idx, plans)
    assert out[2] is None and all(o is not None for k, o in enumerate(out) if k != 2)


def test_every_golden_case_on_the_device(golden_dir):
    """the recorded plans of the fixture (the reference's own draws) through the kernels: the reference's sha256"""
    from gava_clip_amd import RandAugment
    cs = fixture(golden_dir)
    videos = [source_frames(c) for c in cs]
    got = _run(RandAugment("rand"), videos, [c["plan"] for c in cs])
    for c, g in zip(cs, got):
        assert hashlib.sha256(np.ascontiguousarray(g).tobytes()).digest() == c["sha"], (c["c"], c["name"])


def test_whole_policy_equals_the_references_item(golden_dir):
    """AugmentedClipPreprocessor.batch under the fixture's seeds == the fp32 clip the reference's own __getitem__ returned,
    for all four configs (sha256), drawn one video at a time as the dataset does"""
    from gava_clip_amd import AugmentedClipPreprocessor
    dev = torch.device("cuda")
    seen = set()
    for c in fixture(golden_dir):
        if not c["policy"]:
            continue
        seen.add((c["name"], c["interpolation"]))
        pre = AugmentedClipPreprocessor(c["name"], num_frames=c["T"], sampling_rate=c["rate"], spatial_size=c["size"], mean=MEAN,
                                        std=STD, interpolation=c["interpolation"])
        v = torch.from_numpy(ref.video(c["n"], c["H"], c["W"], c["vseed"])).to(dev)
        _seed(c["seed"])
        clip = pre.batch([v])[0].cpu().contiguous().numpy()
        assert clip.shape == (3, c["T"], c["size"], c["size"])
        assert np.array_equal(clip.reshape(-1)[::max(1, clip.size // 4096)][:4096], c["clip_sample"]), c["c"]
        assert hashlib.sha256(clip.tobytes()).digest() == c["clip_sha"], c["c"]
        assert np.array_equal(np.array([random.random(), np.random.random()]), c["next"])
        _seed(c["seed"])
        assert torch.equal(pre(v).cpu(), torch.from_numpy(clip))                 # __call__: the same clip
    assert {n for n, _ in seen} >= {"rand-m7-n4-mstd0.5-inc1", "rand-m9-n2", "rand-m5-n3-mstd1-w0"} and any(i == "random" for _, i in seen)


def test_forward_frames_trains_through_the_augmentation():
    """TINY: forward_frames(videos, pre) under the same seeds agrees with model(pre.batch(videos)) to the bound
    tests/test_train_frames.py holds the two routes to (they take different patch GEMMs), and one loss.backward() through it
    gives finite gradients on every trainable parameter"""
    from gava_clip_amd import AugmentedClipPreprocessor, VitaCLIP
    from gava_clip_amd.config import TINY
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
    m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
    m = m.cuda().train()
    pre = AugmentedClipPreprocessor("rand-m7-n4-mstd0.5-inc1", num_frames=TINY.num_frames, sampling_rate=2, spatial_size=TINY.input_size)
    vids = [torch.from_numpy(ref.video(n, h, w, 600 + i)).cuda() for i, (n, h, w) in enumerate([(11, 90, 130), (6, 120, 80), (9, 64, 64)])]
    _seed(31)
    logits = m.forward_frames(vids, pre)[0]
    m.zero_grad(set_to_none=True)
    (logits * torch.randn(logits.shape, generator=torch.Generator().manual_seed(7)).cuda()).sum().backward()
    torch.cuda.synchronize()
    _seed(31)
    with torch.no_grad():
        want = m(pre.batch(vids))[0]
    v = mixed_violation(logits.detach().cpu().numpy(), want.cpu().numpy())
    print(f"forward_frames vs batch: mixed violation {v:.3e}")
    assert v <= 1.0
    _seed(31)
    draws = [pre.sample(*x.shape[:3]) for x in vids]
    assert sum(len(d[5]) for d in draws) >= 3                                    # the seed does apply ops
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(grads) > 20 and all(torch.isfinite(g).all() and float(g.norm()) > 0 for g in grads.values())
    # every parameter the same step without augmentation trains
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    m.zero_grad(set_to_none=True)
    plain = TrainClipPreprocessor(num_frames=TINY.num_frames, sampling_rate=2, spatial_size=TINY.input_size)
    m.forward_frames(vids, plain)[0].sum().backward()
    assert set(grads) == {n for n, p in m.named_parameters() if p.grad is not None}
