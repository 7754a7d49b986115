"""CPU: multi-view evaluation crops - the all-views restatement against the reference's own crops (fixture), and the host
geometry helper gava_clip_geometry_view against the restatement and against Python's round (the library loads without a GPU)."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

import views_ref as vr
from helpers import REPO
from oracle import preprocess_oracle as po


@pytest.fixture(scope="module")
def lib():
    from gava_clip_amd import build, hip
    build.build(verbose=False)          # compiles only when the library is missing or stale
    return hip.load()


def _desc(n, h, w):
    from gava_clip_amd import hip
    d = hip.ClipDesc()
    d.frames, d.n_frames, d.height, d.width = 0x1000, n, h, w      # a host helper: the pointer is only carried along
    return d


def _view(lib, n, h, w, T, rate, size, sv, tv, view):
    d = _desc(n, h, w)
    assert lib.gava_clip_geometry_view(ctypes.byref(d), T, rate, size, sv, tv, view) == 0
    return d


def test_restatement_reproduces_every_reference_view_bit_for_bit(golden_dir):
    """tests/golden/preprocess_views_ref.npz: every crop the reference's VideoDataset builds at dataset.py:135-136 for six
    synthetic videos (tools/gen_golden_views.py), as sha256 of the fp32 bytes and a strided sample.  views_ref.preprocess_views
    must reproduce each of them, and its view 0 is what the committed oracle returns."""
    g = np.load(os.path.join(golden_dir, "preprocess_views_ref.npz"))
    cases = g["cases"].tolist()
    assert len(cases) == 6
    for i, (n, h, w, T, rate, size, sv, tv) in enumerate(cases):
        v = vr.video(n, h, w, vr.VIDEO_SEED + i)
        views = vr.preprocess_views(v, T, rate, size, vr.MEAN, vr.STD, sv, tv)
        assert len(views) == sv * tv == g[f"sha256_{i}"].shape[0]
        for k, a in enumerate(views):
            a = a.numpy()
            assert np.array_equal(vr.sample(a), g[f"sample_{i}"][k]), (i, k)
            assert hashlib.sha256(a.tobytes()).digest() == g[f"sha256_{i}"][k].tobytes(), (i, k)
        first = po.preprocess_clip(v, T, rate, size, vr.MEAN, vr.STD, num_spatial_views=sv, num_temporal_views=tv)
        assert torch.equal(views[0], first), i


def test_temporal_start_is_pythons_round_exhaustively(lib):
    """t_st == round(slide_len / (n_tv - 1) * i) (dataset.py:171: halves to even, the quotient before the product) for every
    n_frames 1...120, T in {1, 4, 8}, rate in {1, 2, 3}, n_tv 1...12 and every temporal view."""
    from gava_clip_amd import hip
    d = hip.ClipDesc()
    d.frames, d.height, d.width = 0x1000, 40, 56
    halves = 0
    for n in range(1, 121):
        d.n_frames = n
        for T in (1, 4, 8):
            for rate in (1, 2, 3):
                slide = max(n - ((T - 1) * rate + 1), 0)
                for n_tv in range(1, 13):
                    for i in range(n_tv):
                        assert lib.gava_clip_geometry_view(ctypes.byref(d), T, rate, 32, 1, n_tv, i) == 0
                        want = slide // 2 if n_tv == 1 else round(slide / (n_tv - 1) * i)
                        assert d.t_st == want, (n, T, rate, n_tv, i, d.t_st, want)
                        halves += n_tv > 1 and (slide / (n_tv - 1) * i) % 1 == 0.5
    assert halves > 100          # the sweep does reach exact halves (the cases where lround or round-half-up would differ)
    assert _view(lib, 12, 40, 57, 4, 2, 32, 1, 3, 1).t_st == 2       # slide_len 5, step 2.5: round(2.5) == 2


@pytest.mark.parametrize("h,w,size", [(40, 56, 32), (56, 40, 32), (48, 48, 32), (181, 333, 96), (333, 181, 96), (97, 97, 96),
                                      (240, 320, 224), (360, 640, 224)])
def test_spatial_offsets_match_the_restatement(lib, h, w, size):
    for sv, tv in ((1, 1), (3, 1), (3, 4), (1, 5)):
        want = vr.view_offsets(21, h, w, 4, 2, size, sv, tv)
        got = []
        for view in range(sv * tv):
            d = _view(lib, 21, h, w, 4, 2, size, sv, tv, view)
            got.append((d.t_st, d.h_st, d.w_st))
            assert d.rate == 2 and (d.box_y, d.box_x, d.box_h, d.box_w) == (0, 0, h, w)
        assert got == want, (sv, tv)
    if h == w:
        assert len({o[1:] for o in vr.view_offsets(21, h, w, 4, 2, size, 3, 1)}) == 1     # a square frame: three equal views


def test_hip_wrapper_returns_views_video_major(lib, monkeypatch):
    """hip.clip_descriptors_views: B*V descriptors, a video's V views contiguous, and the (t_st, h_st, w_st) table - without
    a GPU (the videos are stand-ins carrying a shape; the descriptor tensor stays on the host)."""
    from gava_clip_amd import hip

    class _Video:
        is_cuda, dtype, device = True, torch.uint8, "cpu"

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return 4

        def is_contiguous(self):
            return True

    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0x1000))
    vids = [_Video(13, 40, 56, 3), _Video(9, 56, 40, 3)]
    desc, keep, geom = hip.clip_descriptors_views(vids, T=4, rate=2, size=32, n_spatial=3, n_temporal=3)
    assert desc.numel() == 18 * ctypes.sizeof(hip.ClipDesc) and keep == vids and geom.shape == (18, 3)
    want = vr.view_offsets(13, 40, 56, 4, 2, 32, 3, 3) + vr.view_offsets(9, 56, 40, 4, 2, 32, 3, 3)
    assert [tuple(r) for r in geom.tolist()] == want
    arr = (hip.ClipDesc * 18).from_buffer_copy(desc.numpy().tobytes())
    assert [(d.n_frames, d.height, d.width) for d in arr] == [(13, 40, 56)] * 9 + [(9, 56, 40)] * 9
    assert [(d.t_st, d.h_st, d.w_st) for d in arr] == want


@pytest.mark.parametrize("n,h,w,T,rate,size", [(13, 40, 56, 4, 2, 32), (9, 56, 40, 4, 1, 32), (12, 48, 48, 4, 2, 32),
                                               (3, 40, 56, 4, 2, 32), (30, 240, 320, 8, 2, 224), (10, 181, 333, 4, 3, 96)])
def test_view_zero_is_the_first_view_descriptor_byte_for_byte(lib, n, h, w, T, rate, size):
    from gava_clip_amd import hip
    for sv, tv in ((1, 1), (1, 10), (3, 1), (3, 4)):
        a, b = _desc(n, h, w), _desc(n, h, w)
        assert lib.gava_clip_geometry(ctypes.byref(a), T, rate, size, int(tv > 1), int(sv == 3)) == 0
        assert lib.gava_clip_geometry_view(ctypes.byref(b), T, rate, size, sv, tv, 0) == 0
        assert bytes(a) == bytes(b) and len(bytes(a)) == ctypes.sizeof(hip.ClipDesc)
        assert b.lerp4_frames == 0 and not b.frame_idx


def test_rejected_view_arguments(lib):
    from gava_clip_amd import hip
    einval = -1
    d = _desc(13, 40, 56)
    assert lib.gava_clip_geometry_view(ctypes.byref(d), 4, 2, 32, 2, 3, 0) == einval       # n_spatial == 2
    assert lib.gava_clip_geometry_view(ctypes.byref(d), 4, 2, 32, 3, 3, 9) == einval       # view == V
    assert lib.gava_clip_geometry_view(ctypes.byref(d), 4, 2, 32, 3, 3, -1) == einval
    assert lib.gava_clip_geometry_view(ctypes.byref(d), 4, 2, 32, 1, 0, 0) == einval       # no temporal view at all
    assert lib.gava_clip_geometry_view(ctypes.byref(d), 4, 2, 32, 3, 3, 8) == 0
    # gava_view_scores rejects before it launches anything (no GPU needed): NULL arguments, non-positive V / C
    a = hip.ViewScoresArgs()
    assert lib.gava_view_scores(None, None) == einval
    a.B, a.V, a.C = 1, 1, 1
    assert lib.gava_view_scores(ctypes.byref(a), None) == einval                           # NULL logits / scores
    a.B, a.V, a.C = 1, 0, 3
    assert lib.gava_view_scores(ctypes.byref(a), None) == einval
    a.B, a.V, a.C = 1, 3, 0
    assert lib.gava_view_scores(ctypes.byref(a), None) == einval
    a.B, a.V, a.C = 0, 3, 3
    assert lib.gava_view_scores(ctypes.byref(a), None) == 0                                # B == 0: nothing to do


def test_view_scores_struct_mirror_agrees(lib, tmp_path):
    """sizeof(gava_view_scores_args) as the C compiler sees the header == the ctypes mirror == the library's own report."""
    from gava_clip_amd import hip
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "gava_hip.h"\n'
                   'int main(){printf("%zu %zu\\n", sizeof(gava_view_scores_args), sizeof(gava_clip_desc));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    c_scores, c_desc = map(int, subprocess.check_output([exe]).decode().split())
    assert ctypes.sizeof(hip.ViewScoresArgs) == c_scores and ctypes.sizeof(hip.ClipDesc) == c_desc
    sizes = (ctypes.c_size_t * 32)()
    n = lib.gava_struct_sizes(sizes, 32)
    assert n == 17 and sizes[16] == c_scores and sizes[4] == c_desc
    assert {"gava_clip_geometry_view", "gava_view_scores"} <= set(hip.EXPORTS)
