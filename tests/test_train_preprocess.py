"""The random-sample data path (video_dataset/dataset.py:93-114, auto_augment=None) and the descriptor geometry behind it:
source box + frame table in gava_clip_desc, one launch per batch, TrainClipPreprocessor.

CPU: the torch restatement (tests/train_preprocess_ref.py) against what the reference's own VideoDataset.__getitem__ returned
(tests/golden/preprocess_train_ref.npz, tools/gen_golden_train_preprocess.py), the parameter draw against the recorded
draws and generator states, the C ABI.  GPU: the kernels against the restatement, bit for bit."""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import train_preprocess_ref as ref
from helpers import REPO

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "preprocess_train_ref.npz"))
    cases = []
    for c, (n, h, w, T, rate, size, seed, vseed) in enumerate(g["cases"].tolist()):
        cases.append(dict(c=c, n=n, h=h, w=w, T=T, rate=rate, size=size, seed=seed, vseed=vseed,
                          idx=g[f"idx_{c}"].tolist(), box=tuple(g[f"box_{c}"].tolist()), fallback=int(g[f"fallback_{c}"]),
                          next=g[f"next_{c}"], sha=g[f"sha256_{c}"].tobytes(), sample=g[f"sample_{c}"]))
    return cases


def _seed(s):
    random.seed(s)
    np.random.seed(s)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_fixture_covers_the_cases_the_kernels_must_handle(golden_dir):
    cs = _fixture(golden_dir)
    assert any(c["h"] < c["w"] for c in cs) and any(c["h"] > c["w"] for c in cs) and any(c["h"] == c["w"] for c in cs)
    assert any(c["box"][2] < c["size"] and c["box"][3] < c["size"] for c in cs)            # upsampling
    assert any(c["box"][2] > c["size"] and c["box"][3] > c["size"] for c in cs)            # downsampling
    assert {8, 16, 70} <= {c["T"] for c in cs} and 224 in {c["size"] for c in cs} and min(c["size"] for c in cs) <= 64
    assert any(c["rate"] > 0 and c["rate"] * (c["T"] - 1) + 1 >= c["n"] for c in cs)       # shorter than the segment
    assert any(c["rate"] < 0 for c in cs)                                                   # TSN
    assert any(c["fallback"] for c in cs)                                                   # ten failed attempts
    assert any(c["box"][0] + c["box"][2] == c["h"] and c["box"][1] + c["box"][3] == c["w"] and not c["fallback"] for c in cs)


def test_restatement_reproduces_the_reference_bit_for_bit(golden_dir):
    """sha256 of the fp32 bytes of every fixture case: the bar tests/test_preprocess.py holds the evaluation branch to."""
    for c in _fixture(golden_dir):
        v = ref.video(c["n"], c["h"], c["w"], c["vseed"])
        a = ref.preprocess_clip(v, c["idx"], *c["box"], c["size"], MEAN, STD).numpy()
        assert a.shape == (3, c["T"], c["size"], c["size"])
        assert np.array_equal(a.reshape(-1)[::max(1, a.size // 4096)][:4096], c["sample"]), c["c"]
        assert hashlib.sha256(a.tobytes()).digest() == c["sha"], c["c"]


def test_both_parameter_draws_reproduce_the_reference(golden_dir):
    """TrainClipPreprocessor.sample and the restatement's draw (written independently) under the fixture's seeds: the recorded
    (idx, i, j, h, w) of every case, the fallback case included, and both generators left in the reference's state (one more
    number drawn from each)."""
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    for c in _fixture(golden_dir):
        pre = TrainClipPreprocessor(num_frames=c["T"], sampling_rate=c["rate"], spatial_size=c["size"], mirror=True)
        for draw in (lambda: pre.sample(c["n"], c["h"], c["w"]), lambda: ref.draw(c["n"], c["h"], c["w"], c["T"], c["rate"])):
            _seed(c["seed"])
            idx, i, j, h, w = draw()
            nxt = np.array([random.random(), np.random.random()])
            assert list(idx) == c["idx"] and (i, j, h, w) == c["box"], (c["c"], idx, (i, j, h, w))
            assert np.array_equal(nxt, c["next"]), c["c"]


def test_auto_augment_is_refused():
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    with pytest.raises(NotImplementedError):
        TrainClipPreprocessor(auto_augment="rand-m7-n4-mstd0.5-inc1")


def test_draws_must_fill_the_frame_table():
    """caller-supplied draws: one per video, each with num_frames indices (the kernels read that many table entries)"""
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    pre = TrainClipPreprocessor(num_frames=4, spatial_size=32)
    v = ref.video(6, 40, 40, 0)
    for draws in ([([0, 1, 2], 0, 0, 8, 8)], [([0, 1, 2, 3, 4], 0, 0, 8, 8)], []):
        with pytest.raises(ValueError):
            pre.descriptors([v], draws)


def test_new_structs_match_header_sizes():
    """sizeof(gava_clip_desc) and sizeof(gava_preprocess_clips_args) as the C compiler sees them == the ctypes mirrors; the box
    and the table are fields of both, at the same offsets."""
    from gava_clip_amd import hip
    names = {"gava_clip_desc": hip.ClipDesc, "gava_preprocess_clips_args": hip.PreprocessClipsArgs,
             "gava_patchify_args": hip.PatchifyArgs}
    fields = ("box_y", "box_x", "box_h", "box_w", "lerp4_frames", "frame_idx")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gava_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "".join(
        f'printf("{f} %zu\\n", offsetof(gava_clip_desc, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert ctypes.sizeof(cls) == sizes[n], n
    for f in fields:
        assert getattr(hip.ClipDesc, f).offset == sizes[f], f


def _lib():
    import __graft_entry__ as ge
    from gava_clip_amd import hip
    from gava_clip_amd.build import needs_build
    if needs_build():
        ge.build()
    return hip.load(), hip


def test_geometry_box_rejects_what_leaves_the_video():
    lib, hip = _lib()
    T = 4
    idx = (ctypes.c_int * T)(0, 3, 5, 9)
    table = ctypes.c_void_p(0x1000)        # never dereferenced on the host

    def call(i, j, h, w, idx=idx, n=10, size=32):
        d = hip.ClipDesc()
        d.n_frames, d.height, d.width = n, 48, 64
        return lib.gava_clip_geometry_box(ctypes.byref(d), size, T, idx, table, i, j, h, w), d

    rc, d = call(4, 22, 44, 42)            # flush with the bottom-right corner: inside
    assert rc == 0
    assert (d.box_y, d.box_x, d.box_h, d.box_w, d.h_st, d.w_st, d.t_st, d.rate) == (4, 22, 44, 42, 0, 0, 0, 1)
    assert d.frame_idx == 0x1000 and d.lerp4_frames == T        # 32 + 32 <= 128: torch's small-output kernel
    assert call(4, 22, 44, 42, size=65)[1].lerp4_frames == 0 and call(4, 22, 44, 42, size=64)[1].lerp4_frames == T
    assert d.scale_h == np.float32(44) / np.float32(32) and d.scale_w == np.float32(42) / np.float32(32)
    assert call(0, 0, 48, 64)[0] == 0      # the whole frame
    for bad in ((5, 22, 44, 42), (4, 23, 44, 42), (-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 0, 10), (0, 0, 10, 0),
                (0, 0, 49, 10), (0, 0, 10, 65), (47, 0, 2, 1), (2 ** 31 - 1, 0, 2, 2)):
        assert call(*bad)[0] == -1, bad
    assert call(0, 0, 8, 8, idx=(ctypes.c_int * T)(0, 3, 5, 10))[0] == -1       # index == n_frames
    assert call(0, 0, 8, 8, idx=(ctypes.c_int * T)(0, -1, 5, 9))[0] == -1
    assert call(0, 0, 8, 8, size=0)[0] == -1
    d = hip.ClipDesc()
    d.n_frames, d.height, d.width = 10, 48, 64
    assert lib.gava_clip_geometry_box(ctypes.byref(d), 32, T, None, table, 0, 0, 8, 8) == -1
    assert lib.gava_clip_geometry_box(ctypes.byref(d), 32, T, idx, None, 0, 0, 8, 8) == -1


def test_geometry_keeps_its_results_and_fills_the_whole_frame_box(golden_dir):
    """gava_clip_geometry for the nine cases of preprocess_ref.npz: the values of dataset.py:124-129,163-199 (what it returned
    before the box existed), plus the whole-frame box and no frame table."""
    lib, hip = _lib()
    g = np.load(os.path.join(golden_dir, "preprocess_ref.npz"))
    assert len(g["cases"]) == 9
    for n, h, w, T, rate, size, sv, tv in g["cases"].tolist():
        d = hip.ClipDesc()
        d.n_frames, d.height, d.width = n, h, w
        d.box_h, d.frame_idx = -7, 0x10
        assert lib.gava_clip_geometry(ctypes.byref(d), T, rate, size, int(tv > 1), int(sv == 3)) == 0
        new_h, new_w = (size, w * size // h) if h < w else (h * size // w, size)
        seg = (T - 1) * rate + 1
        want = dict(t_st=(n - seg) // 2 if (n > seg and tv == 1) else 0, rate=rate,
                    h_st=0 if sv == 3 else (new_h - size) // 2, w_st=0 if sv == 3 else (new_w - size) // 2,
                    scale_h=float(np.float32(h) / np.float32(new_h)), scale_w=float(np.float32(w) / np.float32(new_w)),
                    box_y=0, box_x=0, box_h=h, box_w=w, lerp4_frames=0, frame_idx=None)
        assert {k: getattr(d, k) for k in want} == want


def test_preprocess_kernels_compile_without_scratch():
    """tools/kernel_resources.py on preprocess.hip (cross-compiles for gfx950): every kernel of the file - stand-alone
    preprocessing, the batched launch, patchify - keeps its pixels in registers."""
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "preprocess.hip"]).decode()
    print(out)
    rows = [ln for ln in out.splitlines() if "scratch" in ln]
    names = " ".join(rows)
    assert "preprocess_kernel" in names and "preprocess_clips_kernel" in names and "patchify_kernel" in names
    for ln in rows:
        assert int(re.search(r"scratch\s+(\d+)", ln).group(1)) == 0, ln


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _groups(cases):
    """fixture cases that can share a batch: same T and crop size"""
    by = {}
    for c in cases:
        by.setdefault((c["T"], c["size"]), []).append(c)
    return by


@pytest.mark.gpu
def test_gpu_batched_launch_equals_the_restatement_on_every_fixture_case(golden_dir):
    """gava_preprocess_clips from box + table descriptors, and TrainClipPreprocessor drawing under the fixture's seed, == the
    CPU restatement == the reference, bit for bit; cases of equal (T, size) - videos of different sizes - share one launch."""
    from gava_clip_amd import hip
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    dev = torch.device("cuda")
    groups = _groups(_fixture(golden_dir))
    assert max(len(g) for g in groups.values()) >= 4
    for (T, size), cs in groups.items():
        vids_cpu = [ref.video(c["n"], c["h"], c["w"], c["vseed"]) for c in cs]
        vids = [v.to(dev) for v in vids_cpu]
        want = torch.stack([ref.preprocess_clip(v, c["idx"], *c["box"], size, MEAN, STD) for v, c in zip(vids_cpu, cs)])
        pre = TrainClipPreprocessor(num_frames=T, sampling_rate=cs[0]["rate"], spatial_size=size, mean=MEAN, std=STD)
        draws = [(c["idx"], *c["box"]) for c in cs]
        desc, keep = hip.clip_descriptors_box(vids, draws, size=size)
        x = torch.full((len(cs), 3, T, size, size), float("nan"), device=dev)
        hip.preprocess_clips(desc, x, T=T, size=size, lut=pre.lut(dev))
        assert torch.equal(x.cpu(), want), (T, size)
        assert torch.equal(pre.batch(vids, draws).cpu(), want)
        for v, c, w in zip(vids, cs, want):          # the preprocessor's own draw, one clip at a time (sampling rates differ)
            p1 = TrainClipPreprocessor(num_frames=T, sampling_rate=c["rate"], spatial_size=size, mean=MEAN, std=STD)
            _seed(c["seed"])
            got = p1(v).cpu()
            assert torch.equal(got, w), c["c"]
            assert hashlib.sha256(got.contiguous().numpy().tobytes()).digest() == c["sha"]


@pytest.mark.gpu
def test_gpu_evaluation_batch_equals_the_per_clip_kernel():
    """ClipPreprocessor.batch through the one-launch kernel == gava_preprocess_clip clip by clip, bit for bit (mixed sizes,
    a short video, the first-of-many-views offsets)."""
    from gava_clip_amd.preprocess import ClipPreprocessor
    dev = torch.device("cuda")
    shapes = [(20, 240, 320), (9, 320, 240), (5, 256, 256), (12, 224, 224), (10, 181, 333), (30, 224, 400)]
    vids = [ref.video(n, h, w, 40 + i).to(dev) for i, (n, h, w) in enumerate(shapes)]
    for kw in (dict(), dict(num_temporal_views=10), dict(num_spatial_views=3, num_temporal_views=1)):
        for T, rate, size in ((8, 2, 224), (4, 3, 96)):
            pre = ClipPreprocessor(num_frames=T, sampling_rate=rate, spatial_size=size, mean=MEAN, std=STD, **kw)
            x = pre.batch(vids)
            assert x.shape == (len(vids), 3, T, size, size)
            for b, v in enumerate(vids):
                assert torch.equal(x[b], pre(v)), (kw, T, b)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("patch", [16, 14])
def test_gpu_patch_matrix_and_in_loop_loader_read_box_and_table(golden_dir, prec, patch):
    """gava_patchify from box + table descriptors == patchify(the fp32 clips of the stand-alone kernel), and the 128 x 128
    patch GEMM's in-loop uint8 loader == the same GEMM reading those fp32 clips: bit for bit (one clip_pixel1 body)."""
    from gava_clip_amd import hip
    dev = torch.device("cuda")
    P = hip.PREC_NAMES[prec]
    ran = 0
    for (T, size), cs in _groups(_fixture(golden_dir)).items():
        if size % patch or T > 16:
            continue
        ran += 1
        vids = [ref.video(c["n"], c["h"], c["w"], c["vseed"]).to(dev) for c in cs]
        desc, keep = hip.clip_descriptors_box(vids, [(c["idx"], *c["box"]) for c in cs], size=size)
        lut = hip.clip_lut(MEAN, STD, dev)
        B, g = len(cs), size // patch
        n, K = g * g, 3 * patch * patch
        Kp = (K + 63) // 64 * 64
        x = torch.empty(B, 3, T, size, size, device=dev)
        hip.preprocess_clips(desc, x, T=T, size=size, lut=lut)
        A = [torch.full((B * T * n, Kp), 7.0, device=dev, dtype=hip.h16_dtype(P)) for _ in range(2)]
        hip.patchify(A[0], B=B, T=T, size=size, patch=patch, prec=P, x=x)
        hip.patchify(A[1], B=B, T=T, size=size, patch=patch, prec=P, clips=desc, clip_lut=lut)
        assert torch.equal(A[0], A[1]) and not A[1][:, K:].any() and float(A[1].float().abs().max()) > 0.5
        D = 128                       # N % 256 != 0: the 128 x 128 tile kernel, whose k-loop holds both in-loop loaders
        gen = torch.Generator().manual_seed(5)
        W = torch.zeros(D, Kp)
        W[:, :K] = torch.randn(D, K, generator=gen) * K ** -0.5
        W16 = W.to(dev).to(hip.h16_dtype(P))
        bias, pos, tim = (torch.randn(s_, generator=gen).to(dev) for s_ in ((D,), (n + 1, D), (T, D)))
        outs = []
        for kw in (dict(frames=x), dict(clips=desc, clip_lut=lut)):
            X = torch.zeros(B * T * (n + 1), D, device=dev)
            hip.gemm(None, W16, bias, X, epilogue=hip.EPI_F32_PATCH, prec=P, pos=pos, time=tim, n_patches=n, T=T,
                     M=B * T * n, frame_size=size, patch=patch, **kw)
            outs.append(X)
        assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0.1
    assert ran >= (3 if patch == 16 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("T,size", [(12, 32), (4, 64), (70, 48), (8, 65)])
def test_gpu_small_outputs_follow_torchs_four_weight_kernel(T, size):
    """For outputs of height + width <= 128 torch's CPU F.interpolate runs another kernel than for larger ones (four weight
    products and one fma chain, whose order differs between the frames in whole groups of 8 and the T % 8 left over):
    the batch kernel against the CPU restatement, bit for bit, for frame counts with and without left-over frames, and just
    past the switch (65 + 65 > 128)."""
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    shapes = [(T + 3, 48, 64), (T + 1, 150, 111)]
    vids = [ref.video(n, h, w, 90 + i) for i, (n, h, w) in enumerate(shapes)]
    pre = TrainClipPreprocessor(num_frames=T, sampling_rate=1, spatial_size=size, mean=MEAN, std=STD)
    _seed(5)
    draws = [pre.sample(*v.shape[:3]) for v in vids]
    want = torch.stack([ref.preprocess_clip(v, *d, size, MEAN, STD) for v, d in zip(vids, draws)])
    assert torch.equal(pre.batch([v.cuda() for v in vids], draws).cpu(), want)
