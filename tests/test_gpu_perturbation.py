"""The faithfulness curves on the device: gava_patch_ranks, gava_perturb_clips (bit-equal to perturbation_ref.py),
gava_blur_clips and gava_perturb_scores (within the bounds written there), and VitaCLIP.perturbation_curves / faithfulness end
to end against the plain forward on clips perturbed by the reference.

Every output buffer of the kernel tests is NaN-filled (int32: a sentinel) and 5 elements longer than the kernel's rows: what
lies behind them must be untouched afterwards.
"""
import ctypes

import numpy as np
import pytest
import torch

from gava_clip_amd import hip
import perturbation_ref as pr

pytestmark = pytest.mark.gpu

PAD = 5
SENTINEL = -77


# =====================================================================================================================
# part one: the kernels
def raw_ranks(scores, layout, scope, g, patch=0):
    """gava_patch_ranks through the library on a padded int32 buffer -> ranks on the host."""
    B, T = scores.shape[:2]
    total = T if layout == hip.RANK_FRAME else T * g * g
    flat = torch.full((B * total + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    dev = scores.cuda()
    pooled = nan_words(B * total + PAD) if layout == hip.RANK_PIXEL else None          # the pixel layout's workspace
    a = hip.PatchRanksArgs()
    a.scores, a.ranks, a.pooled = hip.ptr(dev), hip.ptr(flat), hip.ptr(pooled)
    a.B, a.T, a.g, a.patch, a.layout, a.scope = B, T, g, patch, layout, scope
    assert hip.load().gava_patch_ranks(ctypes.byref(a), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    flat = flat.cpu()
    assert bool((flat[-PAD:] == SENTINEL).all()), "written behind its rows"
    if pooled is not None:
        assert torch.isnan(pooled[-PAD:]).all() and torch.equal(pooled[:-PAD].cpu().double(), pr.pool_pixels(scores, patch).view(-1))
    return flat[:-PAD].view(B, total)


@pytest.mark.parametrize("regime", pr.REGIMES)
@pytest.mark.parametrize("B,T,g", pr.RANK_PATCH_CASES, ids=lambda v: str(v))
def test_patch_ranks_equal_the_reference(B, T, g, regime):
    s = pr.regime_scores((B, T, g, g), regime, 11 + g)
    for scope, code in (("clip", hip.SCOPE_CLIP), ("frame", hip.SCOPE_FRAME)):
        want = pr.ranks(s, scope)
        assert torch.equal(raw_ranks(s, hip.RANK_PATCH, code, g), want), scope
        assert torch.equal(hip.patch_ranks(s.cuda(), scope=scope).cpu(), want), scope
    if regime == "equal":
        assert torch.equal(pr.ranks(s, "clip")[0], torch.arange(T * g * g, dtype=torch.int32))


@pytest.mark.parametrize("regime", pr.REGIMES)
@pytest.mark.parametrize("T", pr.RANK_FRAME_T)
def test_frame_ranks_equal_the_reference(T, regime):
    s = pr.regime_scores((3, T), regime, 5 + T)
    want = pr.ranks(s, "clip")
    assert torch.equal(raw_ranks(s, hip.RANK_FRAME, hip.SCOPE_CLIP, 1), want)
    assert torch.equal(hip.patch_ranks(s.cuda()).cpu(), want)


@pytest.mark.parametrize("B,T,S,P", pr.RANK_PIXEL_CASES, ids=lambda v: str(v))
def test_pixel_ranks_equal_the_reference(B, T, S, P):
    s = pr.integer_pixels(B, T, S, S + P)
    s[0, 0, :P, :P] = s[0, 0, :P, P:2 * P]                 # two patches with the same sum: the tie goes to the lower index
    for scope, code in (("clip", hip.SCOPE_CLIP), ("frame", hip.SCOPE_FRAME)):
        want = pr.ranks(s, scope, patch=P)
        assert torch.equal(raw_ranks(s, hip.RANK_PIXEL, code, S // P, P), want), scope
        assert torch.equal(hip.patch_ranks(s.cuda(), patch=P, scope=scope).cpu(), want), scope


def test_the_unit_cap():
    """65536 units in one ranking are taken (sixty-four slices of one ranking, every tile case), one more is refused by the
    wrapper and by the library."""
    s = pr.regime_scores((1, pr.MAX_UNITS), "randn", 3)
    s[0, 1000:1100] = s[0, 40000]                          # ties across slices
    s[0, 65535] = float("nan")
    want = pr.ranks(s, "clip")
    assert torch.equal(raw_ranks(s, hip.RANK_FRAME, hip.SCOPE_CLIP, 1), want)
    assert torch.equal(hip.patch_ranks(s.view(1, 256, 16, 16).cuda()).cpu(), want)
    over = torch.zeros(1, pr.MAX_UNITS + 1, device="cuda")
    with pytest.raises(hip.GavaError, match="at most 65536"):
        hip.patch_ranks(over)
    out = torch.full((pr.MAX_UNITS + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    a = hip.PatchRanksArgs()
    a.scores, a.ranks, a.B, a.T, a.g, a.layout, a.scope = hip.ptr(over), hip.ptr(out), 1, pr.MAX_UNITS + 1, 1, hip.RANK_FRAME, hip.SCOPE_CLIP
    assert hip.load().gava_patch_ranks(ctypes.byref(a), hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def nan_words(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("B,T,S,P,S1,frames", pr.PERTURB_CASES, ids=lambda v: str(v))
def test_perturbed_clips_equal_the_reference(B, T, S, P, S1, frames):
    gen = torch.Generator().manual_seed(S + S1)
    x = torch.randn(B, 3, T, S, S, generator=gen)
    x[0, 0, 0, 0, :3] = torch.tensor([float("nan"), -0.0, float("inf")])          # a selection keeps any bits
    g = S // P
    scores = pr.regime_scores((B, T) if frames else (B, T, g, g), "half_zero", S1)
    rk = pr.ranks(scores, "clip")
    n = rk.shape[1]
    ks = pr.perturb_case_thresholds(n, S1)
    assert len(ks) == S1 and (S1 == 1 or (ks[0] == 0 and ks[-1] == n))
    baselines = {"zero": None, "channel": torch.tensor([0.5, -1.25, 2.0]), "tensor": torch.randn(B, 3, T, S, S, generator=gen)}
    xd, rd = x.cuda(), rk.cuda()
    clip = 3 * T * S * S
    for mode in ("deletion", "insertion"):
        for name, base in baselines.items():
            want = pr.perturb(x, rk, ks, P, mode, base)
            flat = nan_words(B * S1 * clip + PAD)
            out = flat[:B * S1 * clip].view(B, S1, 3, T, S, S)
            got = hip.perturb_clips(xd, rd, ks, patch=P, mode=mode, baseline=base.cuda() if base is not None else None, out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            h = flat.cpu()
            assert torch.isnan(h[-PAD:]).all(), "written behind its rows"
            # bit for bit, NaNs included
            assert torch.equal(h[:-PAD].view(torch.int32), want.view(-1).view(torch.int32)), (mode, name)
            if S1 > 1:
                full_base = pr.perturb(x, rk, [n], P, "deletion", base)[:, 0]
                first, last = got[:, 0].cpu().view(torch.int32), got[:, -1].cpu().view(torch.int32)
                xs, bs = x.view(torch.int32), full_base.view(torch.int32)
                assert torch.equal(first, xs if mode == "deletion" else bs) and torch.equal(last, bs if mode == "deletion" else xs)


def test_frame_scope_ranks_drive_the_same_kernel():
    """Ranks of scope='frame' (a permutation per frame) with thresholds on g*g units: every frame loses k patches."""
    B, T, S, P = 1, 4, 64, 16
    x = torch.randn(B, 3, T, S, S, generator=torch.Generator().manual_seed(2)) + 5.0
    rk = pr.ranks(pr.regime_scores((B, T, 4, 4), "randn", 9), "frame")
    ks = [0, 3, 16]
    got = hip.perturb_clips(x.cuda(), rk.cuda(), ks, patch=P, mode="deletion").cpu()
    assert torch.equal(got, pr.perturb(x, rk, ks, P, "deletion"))
    assert [(got[0, 1, 0, t] == 0).sum().item() for t in range(T)] == [3 * P * P] * T


def run_blur(x, taps):
    flat = nan_words(x.numel() + PAD)
    out = flat[:x.numel()].view(x.shape)
    hip.blur_clips(x.cuda(), taps.cuda(), out=out)
    torch.cuda.synchronize()
    h = flat.cpu()
    assert torch.isnan(h[-PAD:]).all(), "written behind its rows"
    return h[:-PAD].view(x.shape)


@pytest.mark.parametrize("B,T,S,sigma", pr.BLUR_CASES + [(1, 1, 224, 5.0)], ids=lambda v: str(v))
def test_blur_against_the_fp64_convolution(B, T, S, sigma):
    x = torch.randn(B, 3, T, S, S, generator=torch.Generator().manual_seed(S)) * 2.0 + 0.5
    if S == 224:
        x[:, 1:] = 0.0                                     # one 224^2 plane carries the values; the kernel takes whole clips
    taps = hip.gaussian_taps(sigma)
    assert torch.equal(taps, pr.gaussian_taps(sigma))
    got = run_blur(x, taps)
    ref = pr.blur(x[:, :1] if S == 224 else x, taps)
    err = float((got[:, :ref.shape[1]].double() - ref).abs().max())
    bound = pr.blur_bound(taps, x)
    print(f"blur S={S} sigma={sigma} r={taps.numel() // 2}: max |d| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if S == 224:
        assert float(got[:, 1:].abs().max()) == 0.0
    const = torch.full((1, 3, 1, S, S), -3.3)
    err_c = float((run_blur(const, taps).double() - float(const[0, 0, 0, 0, 0])).abs().max())
    assert err_c <= pr.blur_bound(taps, const)
    assert torch.equal(run_blur(x, taps), got)             # no dependence on timing


def run_scores(logits, S1, fractions, target, ref_step):
    """gava_perturb_scores through the library on padded buffers -> dict on the host."""
    nb, C = logits.shape[0] // S1, logits.shape[1]
    dev = logits.cuda()
    f32 = {k: nan_words(n + PAD) for k, n in (("logit", nb * S1), ("prob", nb * S1), ("auc_logit", nb), ("auc_prob", nb))}
    top1 = torch.full((nb * S1 + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    tout = torch.full((nb + PAD,), SENTINEL, dtype=torch.int64, device="cuda")
    tgt = target.cuda() if target is not None else None
    a = hip.PerturbScoresArgs()
    a.logits, a.ld, a.target = hip.ptr(dev), C, hip.ptr(tgt)
    a.logit, a.prob, a.top1 = hip.ptr(f32["logit"]), hip.ptr(f32["prob"]), hip.ptr(top1)
    a.auc_logit, a.auc_prob, a.target_out = hip.ptr(f32["auc_logit"]), hip.ptr(f32["auc_prob"]), hip.ptr(tout)
    a.nb, a.n_steps, a.C, a.ref_step = nb, S1, C, ref_step
    for s, v in enumerate(fractions):
        a.fractions[s] = v
    assert hip.load().gava_perturb_scores(ctypes.byref(a), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    out = {}
    for k, t in {**f32, "top1": top1, "target": tout}.items():
        h = t.cpu()
        assert bool(torch.isnan(h[-PAD:]).all() if h.is_floating_point() else (h[-PAD:] == SENTINEL).all()), f"{k}: written behind its rows"
        out[k] = h[:-PAD]
    out["logit"], out["prob"], out["top1"] = out["logit"].view(nb, S1), out["prob"].view(nb, S1), out["top1"].view(nb, S1)
    return out


def check_scores(got, ref, logits, S1, clips=None):
    sel = slice(None) if clips is None else clips
    assert torch.equal(got["logit"][sel].double(), ref["logit"][sel])                     # a gather: exact
    assert torch.equal(got["top1"].long(), ref["top1"]) and torch.equal(got["target"], ref["target"])
    dp = float((got["prob"][sel].double() - ref["prob"][sel]).abs().max())
    dap = float((got["auc_prob"][sel].double() - ref["auc_prob"][sel]).abs().max())
    dal = float((got["auc_logit"][sel].double() - ref["auc_logit"][sel]).abs().max())
    bound = pr.auc_logit_bound(S1, logits)
    print(f"scores C={logits.shape[1]} S1={S1}: |d prob| {dp:.2e}, |d auc_prob| {dap:.2e}, |d auc_logit| {dal:.2e} (bound {bound:.2e})")
    assert dp <= pr.PROB_TOL and dap <= pr.PROB_TOL and dal <= bound


@pytest.mark.parametrize("C,S1", pr.SCORE_CASES, ids=lambda v: str(v))
def test_perturb_scores(C, S1):
    nb = 5
    gen = torch.Generator().manual_seed(C + S1)
    logits = torch.randn(nb * S1, C, generator=gen) * 3.0
    logits[:S1] *= 100.0 / float(logits[:S1].abs().max())                     # clip 0: logits up to +-100 (logit_scale can reach 100)
    logits[S1:2 * S1] = (logits[S1:2 * S1] * 0.01).round()                    # clip 1: many exact ties
    logits[2 * S1, 0] = logits[2 * S1, C - 1] = float(logits[2 * S1].max()) + 1.0   # clip 2: the maximum twice, first and last class
    fr = pr.linspace_fractions(S1 - 1) if S1 > 1 else [0.0]
    for ref_step in sorted({0, S1 - 1}):
        ref = pr.scores_ref(logits, S1, fr, None, ref_step)
        got = run_scores(logits, S1, fr, None, ref_step)
        check_scores(got, ref, logits, S1)
        assert int(got["target"][2]) == 0 or ref_step != 0                    # the lowest class on the exact tie
        assert got["target"].tolist() == np.argmax(logits.view(nb, S1, C)[:, ref_step].numpy(), axis=1).tolist()
    target = torch.randint(0, C, (nb,), generator=gen)
    check_scores(run_scores(logits, S1, fr, target, 0), pr.scores_ref(logits, S1, fr, target, 0), logits, S1)
    again = run_scores(logits, S1, fr, target, 0)
    first = run_scores(logits, S1, fr, target, 0)
    assert all(torch.equal(again[k], first[k]) for k in again)
    # the wrapper gives the same bits
    w = hip.perturb_scores(logits.cuda(), fr, ref_step=0, target=target.cuda())
    assert all(torch.equal(w[k].cpu().view(-1), first[k].view(-1)) for k in first)


@pytest.mark.parametrize("C,S1", [(3, 11), (400, 1)], ids=lambda v: str(v))
def test_an_out_of_range_target_gives_nan_for_that_clip_only(C, S1):
    nb = 4
    logits = torch.randn(nb * S1, C, generator=torch.Generator().manual_seed(1)) * 2.0
    fr = pr.linspace_fractions(S1 - 1) if S1 > 1 else [0.0]
    target = torch.tensor([1, C, 0, -1])
    got = run_scores(logits, S1, fr, target, 0)
    ref = pr.scores_ref(logits, S1, fr, target, 0)
    for b in (1, 3):
        assert torch.isnan(got["logit"][b]).all() and torch.isnan(got["prob"][b]).all()
        assert torch.isnan(got["auc_logit"][b]) and torch.isnan(got["auc_prob"][b])
    check_scores(got, ref, logits, S1, clips=[0, 2])
    assert got["target"].tolist() == target.tolist()


# =====================================================================================================================
# part two: VitaCLIP.perturbation_curves and faithfulness end to end
from gava_clip_amd import VitaCLIP, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

_CACHE = {}


def model(prec="fp16"):
    if prec not in _CACHE:
        m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
        m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
        m = m.cuda().eval()
        m.set_operand_dtype(prec)
        _CACHE[prec] = m
    return _CACHE[prec]


def clip(B=3, T=TINY.num_frames):
    return torch.from_numpy(synth.synth_clip(B, T, TINY.input_size)).cuda()


G = TINY.input_size // TINY.patch_size


def patch_scores(B, T, seed=4):
    return pr.regime_scores((B, T, G, G), "half_zero", seed)


def curves_from_logits(logits, S1, fr, target, ref_step):
    r = pr.scores_ref(logits.cpu(), S1, fr, None if target is None else target.cpu(), ref_step)
    return r["logit"].float(), r["top1"].int(), r["target"]


@pytest.mark.parametrize("mode", ["deletion", "insertion"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_curves_equal_the_plain_forward_on_reference_clips(prec, mode):
    """The masked clips built on the host by the reference, in (clip, step) order and in the call's own chunks, through the
    plain model(...): logit, top1 and target must be what those logits give, bit for bit; the whole-batch call equals the
    chunked one."""
    m, x = model(prec), clip(3)
    B, T, S, P = 3, x.shape[2], TINY.input_size, TINY.patch_size
    scores = patch_scores(B, T)
    steps = 4
    S1 = steps + 1
    base = torch.tensor([0.25, -0.5, 1.0])
    with torch.no_grad():
        chunked = m.perturbation_curves(x, scores.cuda(), mode=mode, steps=steps, baseline=base.cuda(), max_clips=2 * S1)
        whole = m.perturbation_curves(x, scores.cuda(), mode=mode, steps=steps, baseline=base.cuda())
        rk = pr.ranks(scores, "clip")
        fr, ks = hip.perturb_thresholds(T * G * G, steps)
        xp = pr.perturb(x.cpu(), rk, ks, P, mode, base)                  # [B, S1, 3, T, S, S]
        lg = torch.cat([m(xp[i:i + 2].reshape(-1, 3, T, S, S).cuda())[0] for i in (0, 2)])         # chunks of 2 and 1 clips
    torch.cuda.synchronize()
    assert torch.equal(chunked.ranks.cpu(), rk) and chunked.fractions.tolist() == torch.tensor(fr).float().tolist()
    logit, top1, target = curves_from_logits(lg, S1, fr, None, 0 if mode == "deletion" else S1 - 1)
    assert torch.equal(chunked.logit.cpu(), logit) and torch.equal(chunked.top1.cpu(), top1) and torch.equal(chunked.target.cpu(), target)
    for k in ("logit", "prob", "top1", "auc_logit", "auc_prob", "target", "ranks"):
        assert torch.equal(getattr(chunked, k), getattr(whole, k)), k
    assert chunked.logit.shape == (B, S1) and chunked.auc_prob.shape == (B,) and chunked.mode == mode
    assert bool(torch.isfinite(chunked.prob).all()) and bool(torch.isfinite(chunked.auc_logit).all())


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_endpoints(prec):
    """Insertion at f = 1 and deletion at f = 0 are model(x), whatever the ranking; deletion at f = 1 with "zero" is
    model(zeros), for every clip."""
    m, x = model(prec), clip(3)
    B, T = x.shape[0], x.shape[2]
    with torch.no_grad():
        plain, zeros = m(x)[0], m(torch.zeros_like(x))[0]
        tgt = torch.tensor([2, 0, 1], device="cuda")
        for seed, regime in ((1, "randn"), (2, "equal")):
            s = pr.regime_scores((B, T, G, G), regime, seed).cuda()
            d = m.perturbation_curves(x, s, mode="deletion", target=tgt, steps=3)
            i = m.perturbation_curves(x, s, mode="insertion", target=tgt, steps=3, baseline="blur", blur_sigma=1.0)
            want = plain.gather(1, tgt.view(-1, 1)).view(-1)
            assert torch.equal(d.logit[:, 0], want) and torch.equal(i.logit[:, -1], want)
            assert torch.equal(d.logit[:, -1], zeros.gather(1, tgt.view(-1, 1)).view(-1))
            assert d.top1[:, 0].tolist() == np.argmax(plain.cpu().numpy(), axis=1).tolist() and torch.equal(d.target, tgt)


def test_ranking_sources_and_baselines_run():
    m, x = model("fp16"), clip(2)
    B, T = x.shape[0], x.shape[2]
    rel = m.relevance_maps(x)
    sal = m.saliency(x)[0]
    assert sal.shape == (B, T, TINY.input_size, TINY.input_size)
    with torch.no_grad():
        runs = [m.perturbation_curves(x, rel.patches, steps=5),
                m.perturbation_curves(x, rel.patches, steps=5, scope="frame", mode="insertion", baseline="blur"),
                m.perturbation_curves(x, rel.cls, steps=2, baseline=torch.randn_like(x)),
                m.perturbation_curves(x, sal, fractions=[0, 0.1, 0.25, 0.5, 1], mode="insertion", target=1)]
    torch.cuda.synchronize()
    for c, S1, n in zip(runs, (6, 6, 3, 5), (T * G * G, T * G * G, T, T * G * G)):
        assert c.logit.shape == c.prob.shape == c.top1.shape == (B, S1) and c.ranks.shape == (B, n) and c.fractions.shape == (S1,)
        assert c.auc_logit.shape == c.auc_prob.shape == c.target.shape == (B,)
        assert all(bool(torch.isfinite(t).all()) for t in (c.logit, c.prob, c.auc_logit, c.auc_prob))
        assert bool(((c.prob >= 0) & (c.prob <= 1)).all())
    assert runs[3].target.tolist() == [1, 1]
    assert torch.equal(runs[1].ranks.cpu(), pr.ranks(rel.patches.cpu(), "frame"))
    assert torch.equal(runs[3].ranks.cpu(), hip.patch_ranks(sal, patch=TINY.patch_size).cpu())


def test_faithfulness_table_repeats_with_its_seed():
    m, x = model("fp16"), clip(2)
    with torch.no_grad():
        a = m.faithfulness(x, steps=3, seed=5)
        b = m.faithfulness(x, steps=3, seed=5)
        c = m.faithfulness(x, methods=("relevance",), steps=3, seed=6, target=0)
    torch.cuda.synchronize()
    assert list(a) == ["rollout", "relevance", "saliency", "random"] and list(c) == ["relevance", "random"]
    for name in a:
        assert set(a[name]) == {"deletion", "insertion"}
        for md in a[name]:
            assert a[name][md].mode == md
            for k in ("logit", "prob", "top1", "auc_logit", "auc_prob", "target", "ranks"):
                assert torch.equal(getattr(a[name][md], k), getattr(b[name][md], k)), (name, md, k)
            assert torch.equal(a[name][md].target, a["random"]["deletion"].target)          # one target for every method
    assert not torch.equal(a["random"]["deletion"].ranks, c["random"]["deletion"].ranks)   # another seed, another control
    assert c["relevance"]["insertion"].target.tolist() == [0, 0]
    table = a.table()
    assert len(table.splitlines()) == 5 and "random" in table and "ins auc_prob" in table


def test_refused_outside_evaluation_and_leaves_no_trace():
    m, x = model("fp16"), clip(2)
    s = patch_scores(2, x.shape[2]).cuda()
    with pytest.raises(hip.GavaError, match="no_grad"):
        m.perturbation_curves(x, s)
    with pytest.raises(hip.GavaError, match="no_grad"):
        m.faithfulness(x)
    m.train()
    try:
        with torch.no_grad(), pytest.raises(hip.GavaError, match="eval"):
            m.perturbation_curves(x, s)
    finally:
        m.eval()
    grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
    before = m.cache_text_features
    try:
        for cached in (False, True):
            m.cache_text_features = cached
            with torch.no_grad():
                m.perturbation_curves(x, s, steps=2)
                with pytest.raises(hip.GavaError, match="fractions"):
                    m.perturbation_curves(x, s, fractions=[0.0, 2.0])
            assert m.cache_text_features is cached
    finally:
        m.cache_text_features = before
    for n, p in m.named_parameters():
        assert (p.grad is None) == (grads[n] is None) and (p.grad is None or torch.equal(p.grad, grads[n])), n


def test_blurred_curves_add_no_host_synchronisation():
    """Counted as tests/test_gpu_path_grad.py counts the path calls': the blur baseline's taps go up from pinned memory, so
    the call - three clips in an uneven 2 + 1 split, top-1 or a given target - waits for the device no more often than the
    plain no-grad forward of the same clips."""
    import warnings
    m, x = model("fp16"), clip(3)
    s = patch_scores(3, x.shape[2]).cuda()
    S1 = 4

    def count(fn):
        with torch.no_grad():
            fn()                                    # warm-up: packs, workspaces, the side stream
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        return len([w for w in caught if "synchroniz" in str(w.message).lower()])

    curves = lambda **kw: m.perturbation_curves(x, s, steps=S1 - 1, baseline="blur", max_clips=2 * S1, **kw)
    n_plain, n_top1, n_target = count(lambda: m(x)), count(curves), count(lambda: curves(target=1))
    print(f"\n[perturbation] host synchronisations: forward {n_plain}, blurred curves (top-1) {n_top1}, (target) {n_target}")
    assert n_top1 <= n_plain and n_target <= n_plain
