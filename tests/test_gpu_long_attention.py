"""Attention past the 320-key class (key-streaming kernels, attention.hip / attention_bwd.hip), op by op against fp64
references on the same 16-bit inputs: vision layout (frame rows + G global | T local | 1 summary prompt rows), the
CLS-only last block, the split (hi | lo | hi) output, plain sequences; forward and backward.  Odd sizes exercise the
partial last key block and partial query tiles."""
import pytest
import torch

from gava_clip_amd import hip
from attention_ref import ref_attention, side_index   # the gather and the fp64 forward, shared with the edge tests

pytestmark = pytest.mark.gpu

EPS16 = {hip.PREC_F16: 2 ** -11, hip.PREC_BF16: 2 ** -8}
PRECS = [hip.PREC_F16, hip.PREC_BF16]

# (frames BT, clip length T, global prompts G, frame rows n, heads): keys = n + G + T + 1
VISION = [(55, 55, 8, 257, 2),     # 321 keys: one key past the 320-key class
          (64, 64, 8, 257, 2),     # 330: ViT-L/14, T = 64
          (128, 128, 8, 197, 2),   # 334: ViT-B/16, T = 128
          (70, 70, 8, 257, 3),     # 336: ViT-L/14, T = 70
          (9, 9, 4, 401, 2),       # 415: a 320 px input at P = 16 (401 queries)
          (8, 8, 8, 577, 2),       # 594: ViT-L/14 at 336 px (577 queries)
          (6, 3, 8, 983, 1)]       # 998 keys, two clips
IDS = [f"keys{n + G + T + 1}" for BT, T, G, n, H in VISION]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def make(BT, G, n, heads, prec, seed):
    d = dev()
    dt = hip.h16_dtype(prec)
    D = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(BT * n, 3 * D, generator=g)
    qkv[:, :D] *= 0.125
    side = torch.randn(G + 2 * BT, 2 * D, generator=g)
    return qkv.to(d).to(dt), side.to(d).to(dt)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("BT,T,G,n,heads", VISION, ids=IDS)
def test_long_attention_with_side_rows(prec, BT, T, G, n, heads):
    qkv, side = make(BT, G, n, heads, prec, BT * 7 + n)
    D = heads * 64
    out = torch.full((BT * n, D), float("nan"), dtype=qkv.dtype, device=qkv.device)
    hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=BT, heads=heads, n_q=n, n_kmain=n, prec=prec,
                  side_k=side[:, :D], side_v=side[:, D:], n_g=G, T=T, has_summary=True)
    ref = ref_attention(qkv[:, :D].view(BT, n, D), qkv[:, D:2 * D].view(BT, n, D), qkv[:, 2 * D:].view(BT, n, D), side,
                        BT, T, G, n, heads, n)
    tol = 6 * EPS16[prec]
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double().view(BT, n, D), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("BT,T,G,n,heads", [VISION[1], VISION[4], VISION[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_long_attention_cls_only_queries(prec, BT, T, G, n, heads):
    """The CLS-only last block: one query per frame from its own [BT][D] buffer (q_batch_rows = 1, ld_q = D)."""
    qkv, side = make(BT, G, n, heads, prec, BT * 5 + n)
    D = heads * 64
    qc = qkv.view(BT, n, 3 * D)[:, 0, :D].contiguous()
    out = torch.full((BT, D), float("nan"), dtype=qkv.dtype, device=qkv.device)
    hip.attention(qc, qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=BT, heads=heads, n_q=1, n_kmain=n, prec=prec,
                  side_k=side[:, :D], side_v=side[:, D:], n_g=G, T=T, has_summary=True, q_batch_rows=1)
    ref = ref_attention(qc.view(BT, 1, D), qkv[:, D:2 * D].view(BT, n, D), qkv[:, 2 * D:].view(BT, n, D), side,
                        BT, T, G, n, heads, 1)
    tol = 6 * EPS16[prec]
    assert torch.allclose(out.double().view(BT, 1, D), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("prec", PRECS)
def test_long_attention_split_output(prec):
    """split_out: rows [hi | lo | hi]; hi + lo carries the fp32 result (only P's 16-bit rounding stays)."""
    BT, T, G, n, heads = VISION[5]
    qkv, side = make(BT, G, n, heads, prec, 77)
    D = heads * 64
    out = torch.zeros(BT * n, 3 * D, dtype=qkv.dtype, device=qkv.device)
    hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=BT, heads=heads, n_q=n, n_kmain=n, prec=prec,
                  side_k=side[:, :D], side_v=side[:, D:], n_g=G, T=T, has_summary=True, split_out=True)
    ref = ref_attention(qkv[:, :D].view(BT, n, D), qkv[:, D:2 * D].view(BT, n, D), qkv[:, 2 * D:].view(BT, n, D), side,
                        BT, T, G, n, heads, n).view(BT * n, D)
    hi, lo = out[:, :D].double(), out[:, D:2 * D].double()
    assert torch.equal(out[:, :D], out[:, 2 * D:])
    assert (lo.abs() <= EPS16[prec] * hi.abs() + 1e-6).all()
    tol = 6 * EPS16[prec]
    assert torch.allclose(hi + lo, ref, rtol=tol, atol=tol)
    # hi + lo is closer to the reference than hi alone on average
    assert (hi + lo - ref).abs().mean() < (hi - ref).abs().mean()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch,heads,L", [(3, 2, 333), (2, 3, 641)])
def test_long_plain_attention(prec, batch, heads, L):
    """No side rows (the T-token summary attention once T > 320)."""
    qkv, _ = make(batch, 0, L, heads, prec, L)
    D = heads * 64
    out = torch.zeros(batch * L, D, dtype=qkv.dtype, device=qkv.device)
    hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=batch, heads=heads, n_q=L, n_kmain=L, prec=prec)
    ref = ref_attention(qkv[:, :D].view(batch, L, D), qkv[:, D:2 * D].view(batch, L, D), qkv[:, 2 * D:].view(batch, L, D),
                        None, batch, 1, 0, L, heads, L)
    tol = 6 * EPS16[prec]
    assert torch.allclose(out.double().view(batch, L, D), ref, rtol=tol, atol=tol)


# ---------------------------------------------------------------------------------------------------------------------
# backward (bf16 gradients), against torch autograd in fp64 on the same bf16-rounded operands; same bound as the existing
# backward op tests (P and dS are rounded to bf16 between the two MFMA products)
BF = hip.PREC_BF16
TOL_BWD = 3 * 2 ** -8


@pytest.mark.parametrize("BT,T,heads,n,G,n_q,act16", [
    (64, 64, 2, 257, 8, 0, False),     # 330 keys (streamed dQ), 257 queries (resident dK/dV)
    (8, 8, 2, 300, 8, 0, False),       # 317 keys (resident dQ), 300 queries (streamed dK/dV)
    (9, 9, 2, 401, 4, 0, True),        # 415 keys, 401 queries: both streamed; activations kept in fp16
    (6, 3, 2, 577, 8, 0, False),       # 589 keys, 577 queries
    (8, 8, 2, 401, 4, 1, False),       # CLS-only last block at 414 keys
])
def test_long_attention_backward_with_prompt_rows(BT, T, heads, n, G, n_q, act16):
    g = torch.Generator().manual_seed(BT * 31 + n)
    D = heads * 64
    qkv = torch.randn(BT * n, 3 * D, generator=g).bfloat16()
    side = torch.randn(G + 2 * BT, 2 * D, generator=g).bfloat16()
    nq = n_q or n
    do = torch.randn(BT * n, D, generator=g).bfloat16()
    q64 = qkv[:, :D].double().requires_grad_()
    k64 = qkv[:, D:2 * D].double().requires_grad_()
    v64 = qkv[:, 2 * D:].double().requires_grad_()
    s64 = side.double().requires_grad_()
    idx = side_index(BT, T, G, "cpu")
    K = torch.cat([k64.view(BT, n, D), s64[idx, :D]], 1).view(BT, -1, heads, 64).transpose(1, 2)
    V = torch.cat([v64.view(BT, n, D), s64[idx, D:]], 1).view(BT, -1, heads, 64).transpose(1, 2)
    Q = q64.view(BT, n, heads, 64)[:, :nq].transpose(1, 2) * 0.125
    o = ((Q @ K.transpose(-1, -2)).softmax(-1) @ V).transpose(1, 2).reshape(BT, nq, D)
    (o * do.double().view(BT, n, D)[:, :nq]).sum().backward()

    qs = qkv.float().clone()
    qs[:, :D] *= 0.125
    qd, sd_ = qs.bfloat16().cuda(), side.cuda()
    act = None
    if act16:   # bf16-exact values stored as fp16: lossless, same result as all-bf16
        qd, sd_, act = qd.half(), sd_.half(), hip.PREC_F16
    dqkv = torch.zeros(BT * n, 3 * D, dtype=torch.bfloat16, device="cuda")
    part = torch.full((BT, G + T + 1, 2 * D), float("nan"), dtype=torch.float32, device="cuda")
    dside = part.view(-1, 2 * D)
    q_arg, do_arg, dq_arg, qbr = qd[:, :D], do.cuda(), dqkv[:, :D], 0
    if n_q == 1:
        q_arg = qd.view(BT, n, 3 * D)[:, 0, :D].contiguous()
        do_arg = do.cuda().view(BT, n, D)[:, 0].contiguous()
        dq_arg = torch.zeros(BT, D, dtype=torch.bfloat16, device="cuda")
        qbr = 1
    hip.attention_backward(q_arg, qd[:, D:2 * D], qd[:, 2 * D:], do_arg, dq_arg, dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                           batch=BT, heads=heads, n=n, prec=BF, q_scale=0.125, q_batch_rows=qbr,
                           side_k=sd_[:, :D], side_v=sd_[:, D:], dside_k=dside[:, :D], dside_v=dside[:, D:],
                           n_g=G, T=T, has_summary=True, n_q=n_q, act_prec=act)
    ref_q = q64.grad.view(BT, n, D)[:, :nq]
    got_q = dq_arg.double().cpu().view(BT, 1, D) if n_q == 1 else dqkv[:, :D].double().cpu().view(BT, n, D)[:, :nq]
    assert (got_q - ref_q).abs().max() <= TOL_BWD * ref_q.abs().max() + 1e-6, "dq"
    for name, got, ref in (("dk", dqkv[:, D:2 * D].double().cpu(), k64.grad), ("dv", dqkv[:, 2 * D:].double().cpu(), v64.grad)):
        assert (got - ref).abs().max() <= TOL_BWD * ref.abs().max() + 1e-6, name
    # prompt rows: per-frame fp32 partials, summed over the frames sharing a row
    pv = part.double().cpu().view(BT // T, T, G + T + 1, 2 * D)
    total = torch.cat([pv[:, :, :G].sum(dim=(0, 1)), pv[:, :, G:G + T].sum(dim=1).reshape(BT, 2 * D), pv[:, :, G + T].reshape(BT, 2 * D)])
    assert (total - s64.grad).abs().max() <= TOL_BWD * s64.grad.abs().max(), "dside"


@pytest.mark.parametrize("batch,heads,n", [(3, 2, 333), (2, 2, 641)])
def test_long_plain_attention_backward(batch, heads, n):
    """No prompt rows (the T-token summary attention at T > 320): both kernels streamed."""
    g = torch.Generator().manual_seed(n)
    W = heads * 64
    qkv = torch.randn(batch * n, 3 * W, generator=g).bfloat16()
    do = torch.randn(batch * n, W, generator=g).bfloat16()
    q, k, v = [t.double().view(batch, n, heads, 64).transpose(1, 2).requires_grad_() for t in qkv.split(W, dim=1)]
    o = ((q * 0.125) @ k.transpose(-1, -2)).softmax(-1) @ v
    o.backward(do.double().view(batch, n, heads, 64).transpose(1, 2))
    qkv_s = qkv.float().clone()
    qkv_s[:, :W] *= 0.125
    qd = qkv_s.bfloat16().cuda()
    dqkv = torch.empty(batch * n, 3 * W, dtype=torch.bfloat16, device="cuda")
    hip.attention_backward(qd[:, :W], qd[:, W:2 * W], qd[:, 2 * W:], do.cuda(), dqkv[:, :W], dqkv[:, W:2 * W], dqkv[:, 2 * W:],
                           batch=batch, heads=heads, n=n, prec=BF, q_scale=0.125)
    for name, grad, sl in (("dq", q.grad, slice(0, W)), ("dk", k.grad, slice(W, 2 * W)), ("dv", v.grad, slice(2 * W, 3 * W))):
        ref = grad.transpose(1, 2).reshape(batch * n, W)
        got = dqkv[:, sl].double().cpu()
        assert (got - ref).abs().max() <= TOL_BWD * ref.abs().max() + 1e-6, name
