"""gava_attention_mass against the fp64 reference of attention_maps_ref.py on the same 16-bit operands (the table, the forms,
the regimes and the bound live there, test_attention_maps_host.py checks them on the CPU), and VitaCLIP.attention_maps end
to end: against fp64 torch on the buffers the kept forward left, and against the reference implementation's own attention
(tests/golden/tiny_attention_maps.npz).

Every output buffer of part one is NaN-filled and 5 floats longer than the kernel's rows: what lies behind them must still
be NaN afterwards, what lies inside must be finite.
"""
import os

import numpy as np
import pytest
import torch

from gava_clip_amd import hip
import attention_maps_ref as mr

pytestmark = pytest.mark.gpu

PAD = 5


def query_buffer(c, t):
    """[BT*nq][W] -> the separate query buffer of qbr rows per frame; rows that are no query hold NaN."""
    nq, W = mr.n_queries(c), t.shape[1]
    buf = torch.full((c.BT, c.qbr, W), float("nan"), dtype=t.dtype)
    buf[:, :nq] = t.view(c.BT, nq, W)
    return buf.view(c.BT * c.qbr, W).cuda()


def run_mass(c, x, form, prec, w):
    """-> fp32 [BT][H][n_out] on the host, the padding behind it checked."""
    D = c.heads * 64
    if c.qbr:
        q, k = query_buffer(c, x.q), x.k.cuda()
    else:
        qk = torch.cat([x.q, x.k], 1).cuda()
        q, k = qk[:, :D], qk[:, D:]
    side = x.side.cuda() if c.side else None
    n_out = mr.n_out(c, form)
    flat = torch.full((c.BT * c.heads * n_out + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    out = flat[:c.BT * c.heads * n_out].view(c.BT, c.heads, n_out)
    hip.attention_mass(q, k, out, batch=c.BT, heads=c.heads, n_q=mr.n_queries(c), n_kmain=c.n, prec=prec,
                       w=w.cuda() if w is not None else None, renorm=mr.renorm_of(form),
                       side_k=side[:, :D] if c.side else None, n_g=c.G, T=c.T if c.side else 0, has_summary=c.has_summary,
                       q_batch_rows=c.qbr)
    torch.cuda.synchronize()
    flat = flat.cpu()
    assert torch.isnan(flat[-PAD:]).all(), "written behind its rows"
    got = flat[:-PAD].view(c.BT, c.heads, n_out)
    assert torch.isfinite(got).all()
    return got


PARAMS = mr.params()


@pytest.mark.parametrize("c,form,regime,prec", PARAMS, ids=[mr.param_id(*p) for p in PARAMS])
def test_attention_mass(c, form, regime, prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    seed = mr.seed_of(c, regime)
    x = mr.make_inputs(c, regime, seed, prec)
    w = mr.weights(c, form, seed)
    ref, smax = mr.reference(c, x, form, w)
    got = run_mass(c, x, form, prec, w)
    r = mr.ratio(c, got, ref, smax)
    print(f"error / bound = {r:.3f}  (in units of 2^-23 f max|ref|: {r * mr.BOUND_C:.2f})")
    assert r <= 1, f"|out - ref| reaches {r:.2f} of {mr.BOUND_C} * 2^-23 (1 + Smax + n_q / 16) max|ref|"
    if not mr.renorm_of(form):
        total = got.double().sum(-1)                 # every query's probabilities sum to 1
        assert float((total - mr.n_queries(c)).abs().max()) <= 1e-5 * mr.n_queries(c)


@pytest.mark.parametrize("prec", [mr.F16, mr.BF16], ids=["f16", "bf16"])
def test_too_many_keys_are_refused(prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mr.TOO_MANY
    assert mr.n_keys(c) == mr.MAX_KEYS + 1 == hip.ATTENTION_MASS_MAX_KEYS + 1
    x = mr.make_inputs(c, "randn", 1, prec)
    D = c.heads * 64
    qk, side = torch.cat([x.q, x.k], 1).cuda(), x.side.cuda()
    for renorm in (False, True):
        with pytest.raises(hip.GavaError, match="at most 640"):
            hip.attention_mass(qk[:, :D], qk[:, D:], batch=c.BT, heads=c.heads, n_q=c.n, n_kmain=c.n, prec=prec, renorm=renorm,
                               side_k=side[:, :D], n_g=c.G, T=c.T, has_summary=True)
    # the library itself, behind the wrapper's own check
    a = hip.AttentionMassArgs()
    out = torch.empty(c.BT, c.heads, mr.n_keys(c), dtype=torch.float32, device="cuda")
    a.q, a.k, a.ld_qkv, a.side_k, a.ld_side, a.out = hip.ptr(qk), hip.ptr(qk[:, D:]), 2 * D, hip.ptr(side), 2 * D, hip.ptr(out)
    a.batch, a.heads, a.n_q, a.n_kmain, a.n_g, a.T, a.has_summary, a.prec = c.BT, c.heads, c.n, c.n, c.G, c.T, 1, prec
    import ctypes
    assert hip.load().gava_attention_mass(ctypes.byref(a), hip.stream_ptr()) == -1
    a.n_kmain = a.n_q = c.n - 1
    assert hip.load().gava_attention_mass(ctypes.byref(a), hip.stream_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [mr.TABLE[1], mr.TABLE[9], mr.TABLE[13]], ids=mr.ar.case_id)
def test_null_weights_are_ones_and_runs_repeat(c):
    """w = NULL against an explicit w of ones, and two runs of the weighted chain form: the same bits."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for prec in (mr.F16, mr.BF16):
        x = mr.make_inputs(c, "randn", mr.seed_of(c, "randn"), prec)
        for form in ("mass", "chain"):
            ones = torch.ones(c.BT, c.n)
            assert torch.equal(run_mass(c, x, form, prec, None), run_mass(c, x, form, prec, ones))
        w = mr.weights(c, "chain", 3)
        assert torch.equal(run_mass(c, x, "chain", prec, w), run_mass(c, x, "chain", prec, w))
        assert torch.equal(run_mass(c, x, "mass", prec, None), run_mass(c, x, "mass", prec, None))


# =====================================================================================================================
# part two: VitaCLIP.attention_maps end to end
from gava_clip_amd import VitaCLIP, synth, training  # noqa: E402
from gava_clip_amd.config import TINY, VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, REPO, model_kwargs, synth_torch_state  # noqa: E402

U23 = 2.0 ** -23
_CACHE = {}


def tiny_model(prec="fp16"):
    if prec not in _CACHE:
        m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
        m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
        m = m.cuda().eval()
        m.set_operand_dtype(prec)
        _CACHE[prec] = m
    return _CACHE[prec]


def kept_reference(m, x):
    """The test's own kept forward and, from its buffers in fp64: per block the CLS row's scores and probabilities over all
    keys [BT][H][n_all] and, for every block but the last, the probabilities of every query restricted to the frame's own
    tokens [BT][H][n][n].  Shared by the tests below (computed once per model and input)."""
    key = (id(m), tuple(x.shape))
    if key in _CACHE:
        return _CACHE[key]
    sh, Tm = m._shape, m.num_frames
    B, T = x.shape[0], x.shape[2]
    BT, D, H, G, NL = B * T, sh["D"], sh["H"], sh["G"], sh["layers"]
    n1 = (sh["size"] // sh["P"]) ** 2 + 1
    kept = training.alloc_kept(m, B, T, x.device)
    with torch.no_grad():
        m.encode_video(x, kept=kept)
    torch.cuda.synchronize()
    idx = mr.ar.side_index(BT, Tm, G, "cpu")
    heads = lambda t: t.view(BT, -1, H, 64).transpose(1, 2)
    cls_s, full_p = [], []
    for l in range(NL):
        qkv, side = kept["qkv"][l].double().cpu().view(BT, n1, 3 * D), kept["sidekv"][l].double().cpu()
        q = kept["last_q"].double().cpu().view(BT, 1, D) if l == NL - 1 else qkv[:, :, :D]
        k_main = qkv[:, :, D:2 * D]
        S = heads(q[:, :1].contiguous()) @ heads(torch.cat([k_main, side[idx, :D]], 1)).transpose(-1, -2)
        cls_s.append(S[:, :, 0])
        if l < NL - 1:
            full_p.append((heads(q.contiguous()) @ heads(k_main.contiguous()).transpose(-1, -2)).softmax(-1))
    _CACHE[key] = (torch.stack(cls_s), full_p, heads(kept["last_q"].double().cpu().view(BT, 1, D)) @
                   heads(kept["qkv"][NL - 1].double().cpu().view(BT, n1, 3 * D)[:, :, D:2 * D].contiguous()).transpose(-1, -2))
    return _CACHE[key]


def block_bound(ref, smax, nq):
    """attention_maps_ref.bound for a [BT][H][n_out] result with nq queries."""
    return mr.BOUND_C * U23 * mr.f_of(smax, nq) * ref.abs().amax(-1)


def clip(T):
    return torch.from_numpy(synth.synth_clip(2, T, TINY.input_size)).cuda()


def split_groups(m, maps):
    return [maps.cls.unsqueeze(-1), maps.patches.flatten(-2), maps.global_prompts, maps.local_prompts, maps.summary.unsqueeze(-1)]


@pytest.mark.parametrize("T", [TINY.num_frames, 2 * TINY.num_frames], ids=["T4", "T8"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_cls_maps_match_the_kept_buffers(prec, T):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, x = tiny_model(prec), clip(T)
    cls_s, _, _ = kept_reference(m, x)
    sh = m._shape
    NL, H, G, Tm = sh["layers"], sh["H"], sh["G"], m.num_frames
    g = sh["size"] // sh["P"]
    n1, B = g * g + 1, x.shape[0]
    for layer in list(range(NL)) + [-1, -NL]:
        S = cls_s[layer % NL]                                        # [BT][H][n_all]
        ref = S.softmax(-1)
        bh = block_bound(ref, S.abs().amax(-1), 1)                   # [BT][H]
        per_head = m.attention_maps(x, mode="cls", layer=layer, heads=None)
        mean = m.attention_maps(x, mode="cls", layer=layer, heads="mean")
        torch.cuda.synchronize()
        assert per_head.layer == mean.layer == layer % NL and per_head.mode == "cls"
        assert per_head.patches.shape == (B, T, H, g, g) and per_head.cls.shape == (B, T, H) and per_head.summary.shape == (B, T, H)
        assert per_head.global_prompts.shape == (B, T, H, G) and per_head.local_prompts.shape == (B, T, H, Tm)
        assert mean.patches.shape == (B, T, g, g) and mean.local_prompts.shape == (B, T, Tm) and mean.logits.shape == (B, 3)
        got = torch.cat(split_groups(m, per_head), -1).double().cpu().view(B * T, H, -1)
        want = torch.cat([ref[..., :1], ref[..., 1:n1], ref[..., n1:n1 + G], ref[..., n1 + G:n1 + G + Tm], ref[..., -1:]], -1)
        r = float(((got - want).abs().amax(-1) / bh).max())
        print(f"layer {layer}: per-head error / bound = {r:.3f}")
        assert r <= 1
        got_m = torch.cat(split_groups(m, mean), -1).double().cpu().view(B * T, -1)
        bm = bh.mean(1) + U23 * want.mean(1).abs().amax(-1)          # the mean over the heads: one more rounding
        assert float(((got_m - want.mean(1)).abs().amax(-1) / bm).max()) <= 1
        for maps in (per_head, mean):                                # the groups of one frame sum to 1
            total = sum(t.double().sum(-1) for t in split_groups(m, maps))
            assert float((total - 1).abs().max()) <= 1e-5
        assert torch.equal(per_head.logits, mean.logits) and torch.isfinite(mean.logits).all()


@pytest.mark.parametrize("T", [TINY.num_frames, 2 * TINY.num_frames], ids=["T4", "T8"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_rollout_matches_the_kept_buffers(prec, T):
    """The device chain against the same chain in fp64 on the kept buffers, the kernel's bound compounded element by element:
    with b the bound of r, a step r' = r/2 + mean_h mass(w = r)/2 has  b' = b/2 + (B_l + b A_l)/2 + 2^-23 r'  (B_l the mean over
    the heads of the step's block bounds, b A_l the weights' error carried through the block's probabilities, the last term
    the roundings of the mean and the mix)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, x = tiny_model(prec), clip(T)
    cls_s, full_p, last_s = kept_reference(m, x)
    sh = m._shape
    NL, g = sh["layers"], sh["size"] // sh["P"]
    n1, B = g * g + 1, x.shape[0]
    S = last_s[:, :, 0]                                              # the last block's CLS scores on the frame's own keys
    P = S.softmax(-1)
    r = 0.5 * P.mean(1)
    r[:, 0] += 0.5
    b = 0.5 * block_bound(P, S.abs().amax(-1), 1).mean(1, keepdim=True) + U23 * r
    for l in range(NL - 2, -1, -1):
        A = full_p[l]                                                # [BT][H][n][n]
        out = torch.einsum("fi,fhij->fhj", r, A)
        # Smax of the block: from the probabilities' own scores (log P differs from S by a row constant; recomputed below)
        smax = _smax_main(m, x, l)
        Bl = block_bound(out, smax, n1).mean(1, keepdim=True)
        Am = A.mean(1)
        r_new = 0.5 * r + 0.5 * out.mean(1)
        b = 0.5 * b + 0.5 * (Bl + torch.einsum("fi,fij->fj", b, Am)) + U23 * r_new
        r = r_new
    assert float((r.sum(-1) - 1).abs().max()) < 1e-12
    maps = m.attention_maps(x)                                       # mode="rollout"
    torch.cuda.synchronize()
    assert maps.mode == "rollout" and maps.layer is None and maps.global_prompts is None and maps.summary is None
    assert maps.patches.shape == (B, T, g, g) and maps.cls.shape == (B, T) and maps.logits.shape == (B, 3)
    got = torch.cat([maps.cls.unsqueeze(-1), maps.patches.flatten(-2)], -1).double().cpu().view(B * T, n1)
    ratio = float(((got - r).abs() / b).max())
    print(f"rollout error / compounded bound = {ratio:.3f}; bound / max = {float((b.amax(-1) / r.amax(-1)).max()):.2e}")
    assert ratio <= 1
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-5
    ignored = m.attention_maps(x, mode="rollout", layer=0)           # `layer` is ignored
    assert torch.equal(ignored.patches, maps.patches) and torch.equal(ignored.cls, maps.cls)


def _smax_main(m, x, l):
    """max |score| of block l's queries on the frame's own keys, per (frame, head), from the kept buffers."""
    key = ("smax", id(m), tuple(x.shape), l)
    if key not in _CACHE:
        sh = m._shape
        B, T, D, H = x.shape[0], x.shape[2], sh["D"], sh["H"]
        n1 = (sh["size"] // sh["P"]) ** 2 + 1
        kept = training.alloc_kept(m, B, T, x.device)
        with torch.no_grad():
            m.encode_video(x, kept=kept)
        qkv = kept["qkv"][l].double().cpu().view(B * T, n1, 3 * D)
        heads = lambda t: t.contiguous().view(B * T, n1, H, 64).transpose(1, 2)
        _CACHE[key] = (heads(qkv[:, :, :D]) @ heads(qkv[:, :, D:2 * D]).transpose(-1, -2)).abs().amax(dim=(2, 3))
    return _CACHE[key]


@pytest.mark.parametrize("T", [TINY.num_frames, 2 * TINY.num_frames], ids=["T4", "T8"])
def test_chunked_equals_unchunked(T):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, x = tiny_model(), clip(T)
    for kw in (dict(mode="rollout"), dict(mode="cls", layer=0, heads=None), dict(mode="cls", layer=-1)):
        whole, parts = m.attention_maps(x, **kw), m.attention_maps(x, max_clips=1, **kw)
        for name in whole.__slots__[2:]:
            a, b = getattr(whole, name), getattr(parts, name)
            assert (a is None and b is None) or torch.equal(a, b), (kw, name)


def test_modes_of_the_model_and_what_the_call_leaves_behind():
    """train() and eval() give the same maps; no .grad, no graph; bad arguments are refused."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, x = tiny_model(), clip(TINY.num_frames)
    ev = m.attention_maps(x)
    m.train()
    try:
        tr = m.attention_maps(x.requires_grad_())
    finally:
        m.eval()
    assert torch.equal(ev.patches, tr.patches) and torch.equal(ev.cls, tr.cls)
    assert not tr.patches.requires_grad and not tr.logits.requires_grad and x.grad is None
    assert all(p.grad is None for p in m.parameters())
    E = hip.GavaError
    with pytest.raises(E, match="HIP device"):
        m.attention_maps(x.detach().cpu())
    with pytest.raises(E, match="clip batch"):
        m.attention_maps(x.detach()[0])
    for layer in (TINY.num_layers, -TINY.num_layers - 1, 0.5):
        with pytest.raises(E, match="outside"):
            m.attention_maps(x.detach(), mode="cls", layer=layer)
    with pytest.raises(E, match="heads"):
        m.attention_maps(x.detach(), mode="rollout", heads=None)


def test_vit_b16_shapes_and_sums():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = VIT_B16_T8
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(synth.synth_clip(1, cfg.num_frames, cfg.input_size)).cuda()
    g, T, H, G = cfg.input_size // cfg.patch_size, cfg.num_frames, cfg.num_heads, cfg.num_global_prompts
    roll = m.attention_maps(x)
    assert roll.patches.shape == (1, T, g, g) and roll.cls.shape == (1, T) and roll.logits.shape == (1, 3)
    assert float((roll.patches.double().sum((-1, -2)) + roll.cls.double() - 1).abs().max()) <= 1e-5
    assert bool((roll.patches >= 0).all()) and bool(torch.isfinite(roll.logits).all())
    c = m.attention_maps(x, mode="cls", layer=5, heads=None)
    assert c.patches.shape == (1, T, H, g, g) and c.global_prompts.shape == (1, T, H, G) and c.local_prompts.shape == (1, T, H, T)
    total = c.patches.double().sum((-1, -2)) + c.cls.double() + c.global_prompts.double().sum(-1) + c.local_prompts.double().sum(-1) + c.summary.double()
    assert float((total - 1).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# against the reference implementation's own attention (tools/gen_golden_attention_maps.py)
# GOLDEN_MEASURED: the worst deviation measured on an MI355X (fp16 operands), relative to each map's maximum, over the CLS rows
# of both blocks and heads and the rollout.  The asserted tolerance is twice that (box-to-box and batch-form rounding), and
# may not exceed GOLDEN_CAP.
GOLDEN_MEASURED = 1.61e-3
GOLDEN_CAP = 2e-2


def test_maps_match_the_reference_fixture():
    """CLS probabilities of every block and head, and the rollout, against what the reference's own forward produced
    (fixture: fp32 activations, probabilities in fp64).  The deviation is the 16-bit operand rounding of the whole tower in
    front of each block's softmax.  Measured: worst 1.606e-3 of a map's maximum (the logits of the same kept forward: max |d|
    1.13e-3); asserted: 3.22e-3."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    gold = np.load(os.path.join(REPO, "tests", "golden", "tiny_attention_maps.npz"))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "tiny_attention_maps.npz")) < 32 << 10
    m, x = tiny_model("fp16"), clip(TINY.num_frames)
    sh = m._shape
    NL, H, G, Tm = sh["layers"], sh["H"], sh["G"], m.num_frames
    g = sh["size"] // sh["P"]
    n1, BT = g * g + 1, x.shape[0] * x.shape[2]
    worst = 0.0
    for l in range(NL):
        maps = m.attention_maps(x, mode="cls", layer=l, heads=None)
        got = torch.cat(split_groups(m, maps), -1).double().cpu().view(BT, H, -1).numpy()
        want = gold["cls"][l].astype(np.float64)
        worst = max(worst, float((np.abs(got - want).max(-1) / np.abs(want).max(-1)).max()))
    roll = m.attention_maps(x)
    got = torch.cat([roll.cls.unsqueeze(-1), roll.patches.flatten(-2)], -1).double().cpu().view(BT, n1).numpy()
    want = gold["rollout"].astype(np.float64)
    dev = np.abs(got - want).max(-1) / np.abs(want).max(-1)
    worst = max(worst, float(dev.max()))
    logit_dev = float(np.abs(roll.logits.cpu().numpy() - gold["logits"]).max())
    print(f"\n[attention-maps-golden] worst deviation relative to each map's maximum {worst:.3e}; logits max |d| {logit_dev:.3e}")
    tol = 2 * GOLDEN_MEASURED
    assert tol <= GOLDEN_CAP
    assert worst <= tol, worst
    # the argmax patch per frame agrees wherever the fixture's top two differ by more than the tolerance
    wp, gp = want[:, 1:], got[:, 1:]
    top2 = np.sort(wp, -1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > tol * np.abs(want).max(-1)
    assert (wp.argmax(-1)[clear] == gp.argmax(-1)[clear]).all()
