"""GPU: multi-view evaluation - every spatial x temporal crop through gava_preprocess_clips, the score fusion kernel
gava_view_scores against fp64, and VitaCLIP.forward_views against the per-clip forward and the oracle."""
import os

import numpy as np
import pytest
import torch

import views_ref as vr
from helpers import CLASSES_3, model_kwargs, rel_to_max, synth_torch_state

pytestmark = pytest.mark.gpu


def _pre(T, rate, size, sv, tv):
    from gava_clip_amd.preprocess import ClipPreprocessor
    return ClipPreprocessor(num_frames=T, sampling_rate=rate, spatial_size=size, mean=vr.MEAN, std=vr.STD,
                            num_spatial_views=sv, num_temporal_views=tv)


# ---- preprocessing ---------------------------------------------------------------------------------------------------------

def _fixture_cases():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess_views_ref.npz"))
    return [tuple(c) for c in g["cases"].tolist()]


@pytest.mark.parametrize("case", range(6))
def test_batch_views_matches_the_restatement_on_every_view(case):
    """Every view of the fixture's video (tests/golden/preprocess_views_ref.npz pins the restatement to the reference for
    exactly these) and of a second video of another size and length in the same batch, within the bound
    tests/test_preprocess.py applies to view 0 (6e-6: fp32 arithmetic in torch's order, 2e-6 of the value range); view 0 is
    what batch() serves, bit for bit."""
    n, h, w, T, rate, size, sv, tv = _fixture_cases()[case]
    vids = [vr.video(n, h, w, vr.VIDEO_SEED + case), vr.video(n + 3, w + 9, h + 4, 77 + case)]
    pre = _pre(T, rate, size, sv, tv)
    assert pre.num_views == sv * tv
    dev = [v.cuda() for v in vids]
    x = pre.batch_views(dev)
    assert x.shape == (2, sv * tv, 3, T, size, size) and x.dtype == torch.float32
    assert torch.equal(x[:, 0], pre.batch(dev))
    got = x.cpu()
    for b, v in enumerate(vids):
        ref = vr.preprocess_views(v, T, rate, size, vr.MEAN, vr.STD, sv, tv)
        for k, r in enumerate(ref):
            err = (got[b, k] - r).abs().max().item()
            assert err <= 6e-6, (b, k, err)
    _, _, geom = pre.view_descriptors(dev)
    want = sum((vr.view_offsets(v.shape[0], v.shape[1], v.shape[2], T, rate, size, sv, tv) for v in vids), [])
    assert [tuple(r) for r in geom.tolist()] == want


def test_batch_views_splits_past_the_grid_bound():
    """B * V * T = 1 * (3 * 21846) * 1 = 65538 frames: more than one gava_preprocess_clips launch covers (65535).  The video has
    3 frames and seg_len 1, so the 21846 temporal views start at round(2 / 21845 * i) in {0, 1, 2}: each view must equal the
    restatement's crop of its start (the restatement run with 3 temporal views has exactly the starts 0, 1, 2)."""
    v = vr.video(3, 8, 12, 5)
    tv = 21846
    pre = _pre(1, 1, 8, 3, tv)
    x = pre.batch_views([v.cuda()])
    assert x.shape == (1, 3 * tv, 3, 1, 8, 8)
    ref = torch.stack(vr.preprocess_views(v, 1, 1, 8, vr.MEAN, vr.STD, 3, 3)).view(3, 3, 3, 1, 8, 8)     # [sv][start]
    starts = torch.tensor([round(2 / (tv - 1) * i) for i in range(tv)])
    assert sorted(set(starts.tolist())) == [0, 1, 2]
    want = ref[:, starts].reshape(3 * tv, 3, 1, 8, 8)
    err = (x[0].cpu() - want).abs().amax(dim=(1, 2, 3, 4))
    assert float(err.max()) <= 6e-6, (int(err.argmax()), float(err.max()))
    _, _, geom = pre.view_descriptors([v.cuda()])
    assert geom[:, 0].tolist() == starts.tolist() * 3 and sorted(set(geom[:, 2].tolist())) == [0, 2, 4]


# ---- gava_view_scores ------------------------------------------------------------------------------------------------------

SCORE_SHAPES = [(1, 1, 1), (2, 1, 3), (3, 5, 65), (2, 30, 400), (1, 3, 1000), (5, 7, 64), (4, 9, 63)]


def _logits(B, V, C, seed, offset=False, plant=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, C, generator=g) * 10.0
    winners = torch.randint(0, C, (B,), generator=g)
    if plant:
        x[torch.arange(B), :, winners] += 50.0
    if offset:
        x += (torch.randint(0, 2, (B, V, 1), generator=g).float() * 2 - 1) * 1e4
    return x


def _check_scores(x_dev, x_cpu):
    """x_dev: the device tensor handed to the kernel, x_cpu: the same fp32 values on the host.

    Bound |d| <= 1e-5 on scores in [0, 1], from the arithmetic (fp32, u = 2^-24 = 6e-8), not from a run:
      - the argument x - max is exact when the two are within a factor of two (every term of the +-1e4 rows) and otherwise
        carries one rounding, <= u * |x - max|: for a term that matters (exp(x - max) >= 1e-7, |x - max| <= 16.2) an absolute
        argument error <= 1e-6, i.e. a relative error <= 1e-6 of the exponential; expf itself adds about one ulp (1.2e-7);
      - the sum over the classes is a ceil(C / 64)-long lane sum and a 6-step wave tree: (16 + 6) u = 1.3e-6 relative at
        C = 1000, on top of the terms' 1.1e-6; the reciprocal and the product add two roundings (1.2e-7).  A view's softmax
        term is therefore within 1.1e-6 + 2.4e-6 + 1.2e-7 < 4e-6 relative, and it is at most 1;
      - the mean adds V terms in order and divides: (V + 1) u of a sum that is at most V, i.e. (V + 1) u = 1.9e-6 of the mean at
        V = 30.
    Worst case 4e-6 + 1.9e-6 < 1e-5; the errors are independent roundings, so a correct kernel sits far below."""
    from gava_clip_amd import hip
    B, V, C = x_cpu.shape
    scores, top1 = hip.view_scores(x_dev)
    assert scores.shape == (B, C) and scores.dtype == torch.float32 and scores.is_contiguous()
    assert top1.shape == (B,) and top1.dtype == torch.int32
    want = x_cpu.double().softmax(-1).mean(1)
    got = scores.cpu().double()
    err = float((got - want).abs().max())
    print(f"view_scores {B}x{V}x{C}: max |d| = {err:.3e}, max |row sum - 1| = {float((got.sum(1) - 1).abs().max()):.3e}")
    assert err <= 1e-5, err
    assert float((got.sum(1) - 1).abs().max()) <= 1e-5
    assert torch.equal(top1.cpu().long(), want.argmax(1))
    again, top_again = hip.view_scores(x_dev)
    assert torch.equal(again, scores) and torch.equal(top_again, top1)          # no dependence on timing
    return scores, top1


@pytest.mark.parametrize("B,V,C", SCORE_SHAPES)
def test_view_scores_match_fp64(B, V, C):
    x = _logits(B, V, C, 1000 + C)
    _check_scores(x.cuda(), x)


@pytest.mark.parametrize("B,V,C", [(2, 30, 400), (4, 9, 63)])
def test_view_scores_subtract_the_row_maximum(B, V, C):
    """rows shifted by +-1e4: exp overflows (or every term underflows) unless the maximum is subtracted first"""
    x = _logits(B, V, C, 2000 + C, offset=True)
    _check_scores(x.cuda(), x)


def test_view_scores_read_a_strided_view():
    """a [B, V, C] window of a wider buffer: video and view strides are free, only the class dimension is contiguous"""
    B, V, C = 3, 5, 65
    x = _logits(B, V, C, 31)
    buf = torch.full((B, V + 2, C + 7), float("nan")).cuda()
    win = buf[:, 1:V + 1, 3:3 + C]
    win.copy_(x)
    assert not win.is_contiguous() and win.stride(2) == 1
    s, t = _check_scores(win, x)
    s2, t2 = _check_scores(x.cuda(), x)
    assert torch.equal(s, s2) and torch.equal(t, t2)


def test_view_scores_many_views():
    """more views than one table of per-view statistics holds (64): the running sums cross chunks"""
    x = _logits(2, 130, 70, 41)
    _check_scores(x.cuda(), x)


def test_view_scores_tie_gives_the_lower_class():
    x = _logits(4, 9, 63, 51, plant=False)
    for b, (lo, hi) in enumerate([(3, 40), (0, 62), (17, 18), (61, 62)]):
        x[b, :, lo] += 60.0
        x[b, :, hi] = x[b, :, lo]
    s, t = _check_scores(x.cuda(), x)
    assert t.tolist() == [3, 0, 17, 61]
    assert torch.equal(s[:, [3, 0, 17, 61]].diagonal(), s[:, [40, 62, 18, 62]].diagonal())    # the tie is exact


def test_view_scores_empty_batch_and_rejects():
    from gava_clip_amd import hip
    s, t = hip.view_scores(torch.empty(0, 4, 7, device="cuda"))
    assert s.shape == (0, 7) and t.shape == (0,) and s.dtype == torch.float32 and t.dtype == torch.int32
    with pytest.raises(hip.GavaError):
        hip.view_scores(torch.empty(2, 0, 7, device="cuda"))
    with pytest.raises(AssertionError):
        hip.view_scores(torch.zeros(2, 7, 4, device="cuda").transpose(1, 2))     # class dimension not contiguous


# ---- VitaCLIP.forward_views ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    """TINY model with synthetic weights, three classes; three videos of different sizes, 3 x 3 views, sampling_rate 2;
    forward_views over all of them and the oracle's logits of every restated crop - computed once, left unchanged."""
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.config import TINY
    from oracle.vita_oracle import Oracle
    sd = synth_torch_state(TINY, 3)
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    vids_cpu = [vr.video(11, 90, 130, 21), vr.video(6, 120, 80, 22), vr.video(9, 70, 70, 23)]
    pre = _pre(TINY.num_frames, 2, TINY.input_size, 3, 3)
    vids = [v.cuda() for v in vids_cpu]
    with torch.no_grad():
        out = m.forward_views(vids, pre)
    crops = torch.stack([c for v in vids_cpu for c in vr.preprocess_views(v, TINY.num_frames, 2, TINY.input_size, vr.MEAN, vr.STD, 3, 3)])
    oracle = Oracle(TINY, sd, torch.cat(m.tokenized_prompts)).forward(crops)["logits"].double().view(3, 9, 3)
    return dict(m=m, pre=pre, vids=vids, out=out, oracle=oracle)


def test_forward_views_equals_forward_of_every_preprocessed_view(tiny):
    m, pre, vids = tiny["m"], tiny["pre"], tiny["vids"]
    scores, logits, top1 = tiny["out"]
    assert scores.shape == (3, 3) and logits.shape == (3, 9, 3) and top1.shape == (3,)
    with torch.no_grad():
        want = m(pre.batch_views(vids).flatten(0, 1))[0].view(3, 9, 3)
    assert torch.equal(logits, want)
    assert m.cache_text_features is False


def test_forward_views_meets_the_oracle(tiny):
    scores, logits, top1 = tiny["out"]
    oracle = tiny["oracle"]
    assert rel_to_max(logits.cpu().numpy(), oracle.numpy()) < 1e-3
    want = oracle.softmax(-1).mean(1)
    assert float((scores.cpu().double() - want).abs().max()) < 1e-3
    assert torch.equal(top1.cpu().long(), scores.cpu().argmax(1))


def test_forward_views_first_view_is_forward_frames(tiny):
    """view 0 is the clip forward_frames serves; the batch composition differs (27 clips against 3), so not bit for bit"""
    m, pre, vids = tiny["m"], tiny["pre"], tiny["vids"]
    with torch.no_grad():
        first = m.forward_frames(vids, pre)[0]
    assert rel_to_max(tiny["out"][1][:, 0].cpu().numpy(), first.cpu().numpy()) < 1e-3


def test_forward_views_chunks(tiny, monkeypatch):
    m, pre, vids = tiny["m"], tiny["pre"], tiny["vids"]
    V = pre.num_views
    text_runs, caches = [], []
    encode_text, impl = m.encode_text, m._forward_impl

    def counting_encode_text():
        text_runs.append(1)
        return encode_text()

    def recording_impl(*a, **k):
        out = impl(*a, **k)
        caches.append(m._text_cache)
        return out

    monkeypatch.setattr(m, "encode_text", counting_encode_text)
    monkeypatch.setattr(m, "_forward_impl", recording_impl)
    m._text_cache = None
    with torch.no_grad():
        by_video = m.forward_views(vids, pre, max_clips=V)           # three chunks of one video each
    assert len(caches) == 3 and len(text_runs) == 1                   # one text-tower launch across the three chunks ...
    assert caches[0] is not None and caches[0][0] is not None and all(c is caches[0] for c in caches)    # ... the rest hit its cache entry
    assert m.cache_text_features is False
    with torch.no_grad():
        singles = [m.forward_views([v], pre) for v in vids]
        big = m.forward_views(vids, pre, max_clips=10 ** 6)
        odd = m.forward_views(vids, pre, max_clips=2 * V - 1)        # rounded down to V; never below V:
        tiny_cap = m.forward_views(vids, pre, max_clips=1)
    for k in range(3):
        assert torch.equal(by_video[k], torch.cat([s[k] for s in singles]))
        assert torch.equal(big[k], tiny["out"][k])
        assert torch.equal(odd[k], by_video[k]) and torch.equal(tiny_cap[k], by_video[k])
    m.cache_text_features = True                                      # the caller's setting survives the call
    with torch.no_grad():
        m.forward_views(vids[:1], pre)
    assert m.cache_text_features is True
    m.cache_text_features = False


def test_forward_views_is_the_evaluation_path_only(tiny):
    from gava_clip_amd import hip
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    m, pre, vids = tiny["m"], tiny["pre"], tiny["vids"]
    with pytest.raises(hip.GavaError):
        m.forward_views(vids, pre)                                    # grad enabled
    train_pre = TrainClipPreprocessor(num_frames=pre.num_frames, sampling_rate=2, spatial_size=pre.spatial_size)
    with torch.no_grad(), pytest.raises(hip.GavaError):
        m.forward_views(vids, train_pre)
    assert m.cache_text_features is False
