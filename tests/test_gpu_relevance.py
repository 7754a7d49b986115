"""gava_attention_relevance against the fp64 reference of relevance_ref.py on the same 16-bit operands (the table, the forms,
the regimes, the kinds of dout and the bound live there; test_relevance_host.py checks them on the CPU), and
VitaCLIP.relevance_maps end to end: against the fp64 chain on the very operands its steps ran on, and against the reference
implementation's own relevance (tests/golden/tiny_relevance.npz, c1_relevance.npz).

Every output buffer of part one is NaN-filled and 5 floats longer than the kernel's rows: what lies behind them must still
be NaN afterwards, what lies inside must be finite.  Query rows that are no query hold NaN.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from gava_clip_amd import hip
import relevance_ref as rr

pytestmark = pytest.mark.gpu

PAD = 5


def query_buffer(c, t):
    """[BT*nq][W] -> the separate buffer of qbr rows per frame; rows that are no query hold NaN."""
    nq, W = rr.n_queries(c), t.shape[1]
    buf = torch.full((c.BT, c.qbr, W), float("nan"), dtype=t.dtype)
    buf[:, :nq] = t.view(c.BT, nq, W)
    return buf.view(c.BT * c.qbr, W).cuda()


def run_relevance(c, x, pair, w):
    """-> fp32 [BT][H][n] on the host, the padding behind it checked."""
    prec, act = pair
    D = c.heads * 64
    if c.qbr:
        kv = torch.cat([x.k, x.v], 1).cuda()
        q, k, v, dout = query_buffer(c, x.q), kv[:, :D], kv[:, D:], query_buffer(c, x.dout)
    else:
        qkv = torch.cat([x.q, x.k, x.v], 1).cuda()
        q, k, v, dout = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], x.dout.cuda()
    side = x.side.cuda()
    flat = torch.full((c.BT * c.heads * c.n + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    out = flat[:c.BT * c.heads * c.n].view(c.BT, c.heads, c.n)
    hip.attention_relevance(q, k, v, dout, out, batch=c.BT, heads=c.heads, n_q=rr.n_queries(c), n_kmain=c.n, prec=prec,
                            act_prec=None if act == prec else act, w=w.cuda() if w is not None else None,
                            side_k=side[:, :D], n_g=c.G, T=c.T, has_summary=c.has_summary, q_batch_rows=c.qbr)
    torch.cuda.synchronize()
    flat = flat.cpu()
    assert torch.isnan(flat[-PAD:]).all(), "written behind its rows"
    got = flat[:-PAD].view(c.BT, c.heads, c.n)
    assert torch.isfinite(got).all()
    return got


PARAMS = rr.params()


@pytest.mark.parametrize("c,form,regime,kind,pair", PARAMS, ids=[rr.param_id(*p) for p in PARAMS])
def test_attention_relevance(c, form, regime, kind, pair):
    seed = rr.seed_of(c, regime)
    x = rr.make_inputs(c, regime, seed, pair[0], pair[1], kind)
    w = rr.weights(c, form, seed)
    ref, smax, A = rr.reference(c, x, pair[0], w)
    got = run_relevance(c, x, pair, w)
    r = rr.ratio(c, got, ref, smax, A)
    print(f"error / bound = {r:.3f}  (in units of 2^-23 f A: {r * rr.BOUND_C:.2f})")
    assert r <= 1, f"|out - ref| reaches {r:.2f} of {rr.BOUND_C} * 2^-23 (5 + Smax + n_q / 16) A"
    if kind == "negative":
        assert float(ref.abs().max()) == 0.0 and float(got.abs().max()) == 0.0          # every product <= 0: exactly nothing
    else:
        assert float(got.min()) >= 0.0 and float(got.max()) > 0.0


def test_too_many_keys_are_refused():
    c = rr.TOO_MANY
    assert rr.n_keys(c) == rr.MAX_KEYS + 1 == hip.ATTENTION_RELEVANCE_MAX_KEYS + 1
    x = rr.make_inputs(c, "randn", 1, rr.F16, rr.F16, "random")
    D = c.heads * 64
    qkv, side, dout = torch.cat([x.q, x.k, x.v], 1).cuda(), x.side.cuda(), x.dout.cuda()
    with pytest.raises(hip.GavaError, match="at most 640"):
        hip.attention_relevance(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], dout, batch=c.BT, heads=c.heads, n_q=c.n, n_kmain=c.n,
                                prec=rr.F16, side_k=side[:, :D], n_g=c.G, T=c.T, has_summary=True)
    # the library itself, behind the wrapper's own check
    a = hip.AttentionRelevanceArgs()
    out = torch.empty(c.BT, c.heads, c.n, dtype=torch.float32, device="cuda")
    a.q, a.k, a.v, a.ld_qkv = hip.ptr(qkv), hip.ptr(qkv[:, D:2 * D]), hip.ptr(qkv[:, 2 * D:]), 3 * D
    a.side_k, a.ld_side, a.dout, a.ld_dout, a.out = hip.ptr(side), 2 * D, hip.ptr(dout), D, hip.ptr(out)
    a.batch, a.heads, a.n_q, a.n_kmain, a.n_g, a.T, a.has_summary, a.prec = c.BT, c.heads, c.n, c.n, c.G, c.T, 1, rr.F16
    assert hip.load().gava_attention_relevance(ctypes.byref(a), hip.stream_ptr()) == -1
    a.n_kmain = a.n_q = c.n - 1          # 640 keys: taken (the rows of frame f then start at f * (n - 1): still inside the buffers)
    assert hip.load().gava_attention_relevance(ctypes.byref(a), hip.stream_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [rr.TABLE[0], rr.TABLE[1], rr.TABLE[5]], ids=rr.ar.case_id)
def test_null_weights_are_ones_and_runs_repeat(c):
    """w = NULL against an explicit w of ones, and two runs of the weighted form: the same bits."""
    for pair in rr.PAIRS:
        x = rr.make_inputs(c, "randn", rr.seed_of(c, "randn"), pair[0], pair[1], "random")
        ones = torch.ones(c.BT, rr.n_queries(c))
        first = run_relevance(c, x, pair, None)
        assert torch.equal(first, run_relevance(c, x, pair, ones)) and torch.equal(first, run_relevance(c, x, pair, None))
        w = rr.weights(c, "chain", 3)
        if rr.n_queries(c) > 1:
            assert torch.equal(run_relevance(c, x, pair, w), run_relevance(c, x, pair, w))


# =====================================================================================================================
# part two: VitaCLIP.relevance_maps end to end
from gava_clip_amd import VitaCLIP, synth  # noqa: E402
from gava_clip_amd.config import TINY, VIT_B16_T8  # noqa: E402
from helpers import CLASSES_3, REPO, model_kwargs, synth_torch_state  # noqa: E402

GRAD_TOL = 4e-2         # the frozen norm-wise criterion of the backward's gradients (tests/test_gpu_backward.py)
_CACHE = {}


def model(cfg=TINY, prec="fp16", keep=True, train=False):
    key = (cfg.num_layers, cfg.input_size, prec, keep, train)
    if key not in _CACHE:
        m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
        m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
        m = m.cuda()
        m = m.train() if train else m.eval()
        m.set_operand_dtype(prec)
        if not keep:
            m.keep_activation_bytes = 0
        _CACHE[key] = m
    return _CACHE[key]


def clip(T, cfg=TINY, B=2):
    return torch.from_numpy(synth.synth_clip(B, T, cfg.input_size)).cuda()


def flat(maps):
    """RelevanceMaps -> r fp64 [B*T][n] on the host (cls first)."""
    B, T = maps.cls.shape
    return torch.cat([maps.cls.unsqueeze(-1), maps.patches.flatten(-2)], -1).double().cpu().view(B * T, -1)


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
@pytest.mark.parametrize("T", [TINY.num_frames, 2 * TINY.num_frames], ids=["T4", "T8"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_relevance_matches_the_chain_on_its_own_operands(prec, T, keep):
    """The device chain against the fp64 chain on the operands its steps ran on (the kept or recomputed q / k / v, the prompt
    rows' keys and the backward's d mix, cloned by the request's test-only capture), within the kernel's bound compounded
    step by step (relevance_ref.chain_from_buffers).  The kept route runs fp16 (or bf16) activations under bf16 gradients
    with the last block in its CLS-only form, the recompute route bf16 throughout with the block's full buffers."""
    m, x = model(prec=prec, keep=keep), clip(T)
    sh = m._shape
    NL, H, G, Tm = sh["layers"], sh["H"], sh["G"], m.num_frames
    g = sh["size"] // sh["P"]
    n1, B = g * g + 1, x.shape[0]
    state = dict(capture=[])
    r_dev, logits, target = m._relevance_chunk(x, None, state)
    maps = m.relevance_maps(x)
    torch.cuda.synchronize()
    assert maps.patches.shape == (B, T, g, g) and maps.cls.shape == (B, T) and maps.logits.shape == (B, 3) and maps.target.shape == (B,)
    assert torch.equal(flat(maps), r_dev.double().cpu()) and torch.equal(maps.logits, logits) and torch.equal(maps.target, target)
    assert torch.equal(target, logits.argmax(1)) and target.dtype == torch.int64 and not maps.patches.requires_grad
    steps = state["capture"]
    assert [s["layer"] for s in steps] == list(range(NL - 1, -1, -1)) and "r" not in state
    act = {s["act"] for s in steps}
    assert act == ({m.prec} if keep else {hip.PREC_BF16})
    rows0 = steps[0]["q"].shape[0] // (B * T)
    assert rows0 == (1 if keep else n1)                                # the CLS-only buffers, or the block's own
    if not keep:                                                       # off the CLS rows the last block's d mix is zero
        assert float(steps[0]["dmix"].view(B * T, n1, -1)[:, 1:].abs().max()) == 0.0
    cpu = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in s.items()} for s in steps]
    ref, bound = rr.chain_from_buffers(cpu, B * T, Tm, G, n1, H, hip.PREC_BF16)
    got = r_dev.double().cpu()
    ratio = float(((got - ref).abs() / bound).max())
    print(f"\n[relevance-error] chain {prec} T={T} {'kept' if keep else 'recompute'}: error / compounded bound = {ratio:.3f}; "
          f"bound / max patch = {float((bound[:, 1:].amax(-1) / ref[:, 1:].amax(-1)).max()):.2e}")
    assert ratio <= 1
    assert bool((got[:, 0] >= 1).all()) and bool((got[:, 1:] >= 0).all()) and float(got[:, 1:].max()) > 0


def test_kept_and_recompute_routes_agree_within_rounding():
    """The same clips through both routes: fp16 activations kept from the forward against blocks recomputed in bf16.  Both are
    the relevance of the same model, apart by the operand rounding of a bf16 forward: the frozen gradient criterion."""
    x = clip(TINY.num_frames)
    a, b = flat(model(keep=True).relevance_maps(x, target=1)), flat(model(keep=False).relevance_maps(x, target=1))
    a[:, 0] -= 1
    b[:, 0] -= 1
    dev = float(((a - b).norm(dim=-1) / a.norm(dim=-1)).max())
    print(f"\n[relevance-error] kept vs recompute, per frame norm-wise: {dev:.3e}")
    assert dev <= GRAD_TOL


@pytest.mark.parametrize("T", [TINY.num_frames, 2 * TINY.num_frames], ids=["T4", "T8"])
def test_chunked_equals_unchunked(T):
    m, x = model(), clip(T, B=4)
    target = torch.tensor([0, 2, 1, 2], device="cuda")
    for tg in (None, 1, target):
        whole, parts = m.relevance_maps(x, target=tg), m.relevance_maps(x, target=tg, max_clips=2 if T == TINY.num_frames else 1)
        for name in whole.__slots__:
            assert torch.equal(getattr(whole, name), getattr(parts, name)), (tg, name)
    assert m.relevance_maps(x, target=target).target is target and m.relevance_maps(x, target=1).target.tolist() == [1] * 4


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
def test_asking_moves_nothing_else(keep):
    """A training step after a relevance_maps call is the step of a model that never made the call, bit for bit; the call
    touches no .grad and leaves nothing attached to text_features."""
    m, x = model(keep=keep, train=True), clip(TINY.num_frames)
    w = torch.randn(2, 3, generator=torch.Generator().manual_seed(3)).cuda()

    def step():
        for p in m.parameters():
            p.grad = None
        logits = m(x)[0]
        (logits * w).sum().backward()
        return logits.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}

    l0, g0 = step()
    for p in m.parameters():
        p.grad = None
    maps = m.relevance_maps(x)
    assert all(p.grad is None for p in m.parameters()) and x.grad is None and not x.requires_grad
    assert not (torch.is_tensor(m.text_features) and (m.text_features.requires_grad or m.text_features.grad_fn is not None))
    assert not maps.patches.requires_grad and not maps.logits.requires_grad
    sentinel = {n: torch.full_like(p, 3.0) for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = sentinel[n].clone()
    again = m.relevance_maps(x)
    assert all(torch.equal(p.grad, sentinel[n]) for n, p in m.named_parameters())
    assert torch.equal(again.patches, maps.patches) and torch.equal(again.cls, maps.cls)
    l1, g1 = step()
    assert torch.equal(l0, l1) and set(g0) == set(g1) and "visual.time_embed" in g0
    for n in g0:
        if ".summary_ln." in n:       # fp32 atomics: compared as the repeat test of tests/test_gpu_backward.py does
            assert float((g1[n].double() - g0[n].double()).norm() / g0[n].double().norm()) <= 1e-5, n
        else:
            assert torch.equal(g1[n], g0[n]), n
    m.eval()
    try:                               # eval() gives the maps train() gave
        ev = m.relevance_maps(x)
    finally:
        m.train()
    assert torch.equal(ev.patches, maps.patches) and torch.equal(ev.cls, maps.cls) and torch.equal(ev.logits, maps.logits)
    # nothing kept: the second call's memory is all returned
    del maps, again, ev
    out = m.relevance_maps(x)
    del out
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = m.relevance_maps(x)
    del out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


def test_relevance_maps_adds_no_host_synchronisation():
    """Counted as tests/test_gpu_input_grad.py counts saliency's: no more host synchronisations than a plain forward + backward."""
    import warnings
    m, x = model(train=True), clip(TINY.num_frames)
    target = torch.tensor([0, 2], device="cuda")

    def plain():
        for p in m.parameters():
            p.grad = None
        m(x)[0].gather(1, target.view(-1, 1)).sum().backward()

    def count(fn):
        fn()                                        # warm-up: packs, workspaces, the side stream
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return len([w for w in caught if "synchroniz" in str(w.message).lower()])

    n_plain, n_rel, n_top1 = count(plain), count(lambda: m.relevance_maps(x, target=target)), count(lambda: m.relevance_maps(x, max_clips=1))
    for p in m.parameters():
        p.grad = None
    print(f"\n[relevance-error] host synchronisations: forward + backward {n_plain}, relevance_maps(target) {n_rel}, relevance_maps(top-1, chunked) {n_top1}")
    assert n_rel <= n_plain and n_top1 <= n_plain


def test_refusals(tmp_path, monkeypatch):
    m, x = model(), clip(TINY.num_frames)
    E = hip.GavaError
    with pytest.raises(E, match="HIP device"):
        m.relevance_maps(x.cpu())
    for target in (3, -1):
        with pytest.raises(E, match="outside the 3 classes"):
            m.relevance_maps(x, target=target)
    with pytest.raises(E, match="int64"):
        m.relevance_maps(x, target=torch.tensor([0, 1], device="cuda", dtype=torch.int32))
    with pytest.raises(E, match="int64"):
        m.relevance_maps(x, target=torch.tensor([0, 1, 2], device="cuda"))
    with pytest.raises(E, match="whole groups"):
        m.relevance_maps(x[:1, :, :3])
    big = VitaCLIP(**model_kwargs(dataclasses.replace(TINY, input_size=416), CLASSES_3))     # 26^2 + 1 own keys alone are past 640
    with pytest.raises(E, match="at most 640"):
        big.relevance_maps(torch.zeros(1, 3, TINY.num_frames, 416, 416, device="cuda"))
    synth.synth_descriptor_files(str(tmp_path), "updrs", (2, 3, 1))
    monkeypatch.chdir(tmp_path)
    d = VitaCLIP(**{**model_kwargs(TINY, CLASSES_3), "text_prompt_init": "cntn_split_uni_disc", "knowledge_version": ["v1", "v2", "v3"],
                    "use_descriptor": True}).cuda().eval()
    with pytest.raises(E, match="per-descriptor"):
        d.relevance_maps(x)


# ---------------------------------------------------------------------------------------------------------------------
# against the reference implementation's own relevance (tools/gen_golden_relevance.py)
# GOLDEN_MEASURED: the worst per-frame deviation  |got - ref| / |ref|  (2-norms over the frame's tokens, of r - e_cls: the CLS
# entry's constant 1 would hide everything else) measured on an MI355X with fp16 operands; the record is
# profiles/relevance_errors.txt.  The asserted tolerance is twice that, and may not exceed the frozen gradient criterion.
GOLDEN_MEASURED = {"tiny": 9.102e-3, "c1": 1.454e-3}


def _golden(name, cfg):
    gold = np.load(os.path.join(REPO, "tests", "golden", f"{name}_relevance.npz"))
    m = model(cfg)
    x = clip(cfg.num_frames, cfg)
    maps = m.relevance_maps(x, target=torch.from_numpy(gold["target"]).cuda())
    got, want = flat(maps).numpy(), gold["relevance"].astype(np.float64)
    got[:, 0] -= 1
    want[:, 0] -= 1
    dev = np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1)
    lg, lw = maps.logits.cpu().numpy(), gold["logits"]
    logit_dev = float(np.abs(lg - lw).max() / np.abs(lw).max())
    print(f"\n[relevance-error] {name} vs the reference's own relevance: per frame norm-wise worst {dev.max():.3e} median "
          f"{np.median(dev):.3e}; logits max |d| / max |ref| {logit_dev:.3e}")
    return maps, got, want, dev, logit_dev, gold


@pytest.mark.parametrize("name,cfg", [("tiny", TINY), ("c1", VIT_B16_T8)], ids=["tiny", "c1"])
def test_relevance_matches_the_reference_fixture(name, cfg):
    """The device's relevance against what the reference's own forward and backward give (fixture: fp32 activations and
    gradients, the chain in fp64), for the reference's own top-1 class.  The deviation is the 16-bit operand rounding of the
    forward times that of the bf16 backward, carried through the chain - twelve steps at c1.  Measured: TINY worst 9.10e-3
    (median 3.9e-3), c1 worst 1.45e-3 (median 1.1e-3; its A-_l are small, so the chain is close to linear in them); asserted:
    1.82e-2 and 2.91e-3."""
    maps, got, want, dev, logit_dev, gold = _golden(name, cfg)
    tol = min(2 * GOLDEN_MEASURED[name], GRAD_TOL)
    assert float(dev.max()) <= tol, (float(dev.max()), tol)
    # the argmax patch per frame agrees wherever the fixture's top two are further apart than two elements can move together
    wp, gp = want[:, 1:], got[:, 1:]
    top2 = np.sort(wp, -1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * tol * np.linalg.norm(want, axis=-1)
    print(f"[relevance-error] {name}: argmax compared on {int(clear.sum())} of {len(clear)} frames")
    assert (wp.argmax(-1)[clear] == gp.argmax(-1)[clear]).all()
    # the logits of the same call: what tests/test_gpu_input_grad.py asserts of this very forward against its fixture
    assert logit_dev <= 1e-3
    assert (maps.target.cpu().numpy() == gold["target"]).all()


def test_vit_b16_shapes_signs_and_class_specificity():
    cfg = VIT_B16_T8
    m, x = model(cfg), clip(cfg.num_frames, cfg)
    g, T = cfg.input_size // cfg.patch_size, cfg.num_frames
    maps = [m.relevance_maps(x, target=t) for t in (0, 1, 2)]
    for mp in maps:
        assert mp.patches.shape == (2, T, g, g) and mp.cls.shape == (2, T) and mp.logits.shape == (2, 3) and mp.target.shape == (2,)
        assert all(bool(torch.isfinite(t).all()) for t in (mp.patches, mp.cls, mp.logits))
        assert bool((mp.cls >= 1).all()) and bool((mp.patches >= 0).all()) and float(mp.patches.max()) > 0
    assert torch.equal(maps[0].logits, maps[1].logits)
    for a, b in ((0, 1), (0, 2), (1, 2)):                              # another class, another map - in every frame
        pa, pb = maps[a].patches.flatten(-2).double(), maps[b].patches.flatten(-2).double()
        apart = (pa - pb).norm(dim=-1) / pa.norm(dim=-1)
        assert float(apart.min()) > GRAD_TOL, (a, b, float(apart.min()))
