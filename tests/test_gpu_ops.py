"""GPU: every C-ABI kernel against a plain torch fp32 reference of the same op on the same
16-bit-rounded operands (so the only differences are fp32 summation order and the final rounding)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import hip  # noqa: E402

PRECS = [hip.PREC_F16, hip.PREC_BF16]
EPS16 = {hip.PREC_F16: 2 ** -11, hip.PREC_BF16: 2 ** -8}
EIGHT_WORKGROUPS = 1 << 20     # gava_gemm_args.cu_reserve: any reserve >= CUs - 8 leaves a persistent launch 8 workgroups, on any device


def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 256, 192), (3, 128, 128), (1000, 384, 768), (257, 768, 3072),
                                   (4100, 768, 768), (2500, 512, 192), (20000, 256, 64), (3000, 384, 128)])
def test_gemm_epilogues(prec, M, N, K):
    d = dev()
    dt = hip.h16_dtype(prec)
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = rnd((N, K), K ** -0.5, 2).to(d).to(dt)
    bias = rnd((N,), 0.5, 3).to(d)
    ref = A.float() @ W.float().t() + bias
    tol = 4 * EPS16[prec]
    # H16 with column scaling
    out = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, bias, out, epilogue=hip.EPI_H16, prec=prec, scale_cols=N // 2, scale=0.125)
    r = ref.clone(); r[:, :N // 2] *= 0.125
    assert torch.allclose(out.float(), r, rtol=tol, atol=tol * 2)
    # quick-gelu
    out = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, bias, out, epilogue=hip.EPI_H16_QGELU, prec=prec)
    r = ref * torch.sigmoid(1.702 * ref)
    assert torch.allclose(out.float(), r, rtol=tol, atol=tol * 2)
    # fp32, no residual, no bias
    out = torch.zeros(M, N, dtype=torch.float32, device=d)
    hip.gemm(A, W, None, out, epilogue=hip.EPI_F32, prec=prec)
    assert torch.allclose(out, ref - bias, rtol=1e-4, atol=1e-4)
    # fp32 in-place residual
    X = rnd((M, N), 1.0, 4).to(d)
    X0 = X.clone()
    hip.gemm(A, W, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X)
    assert torch.allclose(X, X0 + ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_does_not_touch_rows_beyond_M(prec):
    d = dev()
    dt = hip.h16_dtype(prec)
    M, N, K = 130, 128, 64
    A = rnd((M, K)).to(d).to(dt)
    W = rnd((N, K)).to(d).to(dt)
    out = torch.full((256, N), 7.0, dtype=torch.float32, device=d)
    hip.gemm(A, W, None, out, epilogue=hip.EPI_F32, prec=prec, M=M)
    assert torch.all(out[M:] == 7.0)
    assert torch.allclose(out[:M], A.float() @ W.float().t(), rtol=1e-4, atol=1e-4)


def test_gemm_patch_epilogue_and_rejects():
    d = dev()
    prec = hip.PREC_F16
    frames, n, T, D, K = 6, 16, 3, 128, 192
    A = rnd((frames * n, K), 1.0, 5).to(d).half()
    W = rnd((D, K), K ** -0.5, 6).to(d).half()
    bias, pos, tim = rnd((D,), 1, 7).to(d), rnd((n + 1, D), 1, 8).to(d), rnd((T, D), 1, 9).to(d)
    X = torch.zeros(frames * (n + 1), D, device=d)
    hip.gemm(A, W, bias, X, epilogue=hip.EPI_F32_PATCH, prec=prec, pos=pos, time=tim, n_patches=n, T=T)
    ref = (A.float() @ W.float().t() + bias).view(frames, n, D) + pos[1:].unsqueeze(0) \
        + tim[torch.arange(frames, device=d) % T].unsqueeze(1)
    Xv = X.view(frames, n + 1, D)
    assert torch.allclose(Xv[:, 1:], ref, rtol=1e-4, atol=1e-4)
    assert torch.all(Xv[:, 0] == 0)
    with pytest.raises(hip.GavaError):   # N not a multiple of 128
        hip.gemm(A, W[:100], None, torch.zeros(frames * n, 100, device=d), epilogue=hip.EPI_F32, prec=prec)
    with pytest.raises(hip.GavaError):   # K not a multiple of 64
        hip.gemm(A[:, :40].contiguous(), W[:, :40].contiguous(), None, X, epilogue=hip.EPI_F32, prec=prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,D", [(5, 128), (1001, 768), (64, 1024), (33, 512)])
def test_layernorm(prec, rows, D):
    d = dev()
    x = (rnd((rows, D), 3.0, 1) + 1.5).to(d)
    g, b = (1 + rnd((D,), 0.1, 2)).to(d), rnd((D,), 0.1, 3).to(d)
    ref = torch.nn.functional.layer_norm(x, (D,), g, b, 1e-5)
    o16 = torch.zeros(rows, D, dtype=hip.h16_dtype(prec), device=d)
    o32 = torch.zeros(rows, D, device=d)
    hip.layernorm(x, g, b, out16=o16, out32=o32, prec=prec)
    assert torch.allclose(o32, ref, rtol=2e-6, atol=2e-6)
    assert torch.equal(o16, o32.to(o16.dtype))
    # in place fp32, strided gather of rows, cast-only
    x2 = x.clone()
    hip.layernorm(x2, g, b, out32=x2, prec=prec)
    assert torch.allclose(x2, ref, rtol=2e-6, atol=2e-6)
    idx = torch.arange(rows - 1, -1, -2, device=d, dtype=torch.int32)
    o = torch.zeros(idx.numel(), D, device=d)
    hip.layernorm(x, g, b, out32=o, prec=prec, rows=idx.numel(), row_index=idx)
    assert torch.allclose(o, ref[idx.long()], rtol=2e-6, atol=2e-6)
    c = torch.zeros(rows, D, dtype=hip.h16_dtype(prec), device=d)
    hip.layernorm(x, None, None, out16=c, prec=prec)
    assert torch.equal(c, x.to(c.dtype))
    # two LayerNorms in one row pass (ln_pre + norm1 of block 0): out32 = first, out16 = second applied to the first;
    # bit-identical to two separate launches, also in place
    g2, b2 = (1 + rnd((D,), 0.1, 4)).to(d), rnd((D,), 0.1, 5).to(d)
    sep16 = torch.zeros(rows, D, dtype=hip.h16_dtype(prec), device=d)
    hip.layernorm(o32, g2, b2, out16=sep16, prec=prec)
    x3, f16 = x.clone(), torch.zeros(rows, D, dtype=hip.h16_dtype(prec), device=d)
    hip.layernorm(x3, g, b, out16=f16, out32=x3, prec=prec, gamma2=g2, beta2=b2)
    assert torch.equal(x3, o32) and torch.equal(f16, sep16)
    with pytest.raises(hip.GavaError):
        hip.layernorm(x, g, b, out16=f16, prec=prec, gamma2=g2, beta2=b2)      # needs out32 for the first result


def attn_ref(q, k, v, causal):
    s = q.float() @ k.float().transpose(-1, -2)
    if causal:
        L = s.shape[-1]
        s = s + torch.full((L, L), float("-inf"), device=s.device).triu_(1)
    return s.softmax(-1) @ v.float()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch,heads,L,causal", [(3, 8, 77, True), (5, 2, 8, False), (2, 12, 16, False),
                                                  (4, 2, 197, False), (1, 16, 257, False),
                                                  (90, 12, 215, False),    # persistent kernel, no prompt rows, 14 query tiles
                                                  (86, 12, 224, False),    # ... its largest problem: 224 keys, no masked key at all
                                                  (3, 4, 209, False)])     # smallest key count of the 14-tile class (one key in the last tile)
def test_attention_plain_and_causal(prec, batch, heads, L, causal):
    d = dev()
    dt = hip.h16_dtype(prec)
    D = heads * 64
    qkv = rnd((batch * L, 3 * D), 1.0, 11).to(d)
    qkv[:, :D] *= 0.125
    qkv = qkv.to(dt)
    out = torch.zeros(batch * L, D, dtype=dt, device=d)
    hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=batch, heads=heads, n_q=L, n_kmain=L,
                  prec=prec, causal=causal)
    r = qkv.view(batch, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = attn_ref(r[0], r[1], r[2], causal).permute(0, 2, 1, 3).reshape(batch * L, D)
    tol = 6 * EPS16[prec]
    assert torch.allclose(out.float(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,T,G,n_main,heads", [(2, 4, 4, 17, 2), (2, 8, 8, 197, 12), (1, 16, 8, 197, 3),
                                                (11, 8, 8, 197, 13), (32, 8, 4, 130, 6),
                                                (1, 32, 8, 257, 2), (2, 32, 8, 257, 3), (1, 32, 8, 241, 2), (1, 16, 8, 225, 2)])
def test_attention_with_side_rows(prec, B, T, G, n_main, heads):
    """Vision layout: per-frame main tokens + [G global | T per-clip local | 1 per-frame summary].  Cases 4 and 5 have
    enough (frame, head) problems (>= 4 per CU) for the persistent double-buffered kernel, with an uneven number of
    problems per workgroup.  The 257-query cases are ViT-L/14's (298 keys, the 320-key class): 16 query tiles + the CLS query,
    whose tile the four waves of a workgroup share by keys (parts met in LDS); 241 (16 tiles, no odd one) and 225 (15 tiles: the
    odd tile stays a half-empty pair) run the same class without the shared tile."""
    d = dev()
    dt = hip.h16_dtype(prec)
    D, BT = heads * 64, B * T
    qkv = rnd((BT * n_main, 3 * D), 1.0, 21).to(d)
    qkv[:, :D] *= 0.125
    qkv = qkv.to(dt)
    side = rnd((G + 2 * BT, 2 * D), 1.0, 22).to(d).to(dt)
    out = torch.zeros(BT * n_main, D, dtype=dt, device=d)
    hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, batch=BT, heads=heads, n_q=n_main,
                  n_kmain=n_main, prec=prec, side_k=side[:, :D], side_v=side[:, D:], n_g=G, T=T, has_summary=True)
    q = qkv[:, :D].view(BT, n_main, heads, 64)
    k = qkv[:, D:2 * D].view(BT, n_main, D)
    v = qkv[:, 2 * D:].view(BT, n_main, D)
    ref = torch.zeros(BT, n_main, D, device=d)
    for f in range(BT):
        b = f // T
        rows = torch.cat([torch.arange(G), G + b * T + torch.arange(T), torch.tensor([G + BT + f])]).to(d)
        kf = torch.cat([k[f], side[rows, :D]], 0).view(-1, heads, 64).permute(1, 0, 2)
        vf = torch.cat([v[f], side[rows, D:]], 0).view(-1, heads, 64).permute(1, 0, 2)
        ref[f] = attn_ref(q[f].permute(1, 0, 2), kf, vf, False).permute(1, 0, 2).reshape(n_main, D)
    tol = 6 * EPS16[prec]
    assert torch.allclose(out.float(), ref.view(BT * n_main, D), rtol=tol, atol=tol)


def test_similarity_head():
    d = dev()
    lib = hip.load()
    B, Cn, E = 5, 3, 512
    v, t = rnd((B, E), 2.0, 31).to(d), rnd((Cn, E), 3.0, 32).to(d)
    ls = torch.tensor([math.log(1 / 0.07)], device=d)
    logits, tf, vn = torch.zeros(B, Cn, device=d), torch.zeros(Cn, E, device=d), torch.zeros(B, E, device=d)
    hip.check(lib.gava_similarity_head(hip.ptr(v), hip.ptr(t), hip.ptr(ls), None, B, Cn, 1, E, hip.ptr(logits),
                                       hip.ptr(tf), hip.ptr(vn), hip.stream_ptr()), "head")
    vr, tr = v / v.norm(dim=-1, keepdim=True), t / t.norm(dim=-1, keepdim=True)
    assert torch.allclose(vn, vr, rtol=1e-6, atol=1e-7)
    assert torch.allclose(tf, tr / tr.norm(dim=-1, keepdim=True), rtol=1e-6, atol=1e-7)
    assert torch.allclose(logits, ls.exp() * vr @ tr.t(), rtol=1e-5, atol=1e-5)


def test_similarity_head_with_several_prompts_per_class():
    """n_kv prompts per class (knowledge-aware prompts): class logit = mean over its prompts of the cosine logits, class
    feature = re-normalised mean of the unit prompt features (VitaCLIP_model.py:282-291), plus the logit bias."""
    d = dev()
    lib = hip.load()
    B, C_, K, E = 7, 3, 5, 512
    v, t = rnd((B, E), 2.0, 41).to(d), rnd((C_ * K, E), 3.0, 42).to(d)
    ls, lb = torch.tensor([math.log(1 / 0.07)], device=d), torch.tensor([-0.5], device=d)
    logits, tf, vn = torch.zeros(B, C_, device=d), torch.zeros(C_, E, device=d), torch.zeros(B, E, device=d)
    hip.check(lib.gava_similarity_head(hip.ptr(v), hip.ptr(t), hip.ptr(ls), hip.ptr(lb), B, C_, K, E, hip.ptr(logits),
                                       hip.ptr(tf), hip.ptr(vn), hip.stream_ptr()), "head")
    vr, tr = v / v.norm(dim=-1, keepdim=True), t / t.norm(dim=-1, keepdim=True)
    want = (ls.exp() * vr @ tr.t()).view(B, C_, K).mean(-1) + lb
    m = tr.view(C_, K, E).mean(1)
    assert torch.allclose(logits, want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(tf, m / m.norm(dim=-1, keepdim=True), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("prec,tol", [(hip.PREC_F16, 2e-5), (hip.PREC_BF16, 2e-4)])
def test_split_precision_chain(prec, tol):
    """LN(split) -> GEMM(QGELU, split out) -> GEMM with [W_hi|W_hi|W_lo] weights tracks the fp32 chain
    ~100x closer than plain 16-bit operands (3 MFMA passes per product)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    M, D, F = 200, 256, 512
    x = rnd((M, D), 2.0, 41).to(d)
    g, b = (1 + rnd((D,), 0.1, 42)).to(d), rnd((D,), 0.1, 43).to(d)
    W1, b1 = rnd((F, D), D ** -0.5, 44).to(d), rnd((F,), 0.1, 45).to(d)
    W2, b2 = rnd((D, F), F ** -0.5, 46).to(d), rnd((D,), 0.1, 47).to(d)
    xn = torch.zeros(M, 3 * D, dtype=dt, device=d)
    hip.layernorm(x, g, b, out16=xn, prec=prec, split_out=True)
    h = torch.zeros(M, 3 * F, dtype=dt, device=d)
    hip.gemm(xn, hip.split_pack_weight(W1, prec), b1, h, epilogue=hip.EPI_H16_QGELU, prec=prec, split_out=True)
    out = torch.zeros(M, D, device=d)
    hip.gemm(h, hip.split_pack_weight(W2, prec), b2, out, epilogue=hip.EPI_F32, prec=prec)
    r = torch.nn.functional.layer_norm(x, (D,), g, b, 1e-5).double() @ W1.double().t() + b1
    r = r * torch.sigmoid(1.702 * r)
    ref = (r @ W2.double().t() + b2).float()
    err = float((out - ref).abs().max() / ref.abs().max())
    assert err < tol, err


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_large_m_patch_split_and_ragged(prec):
    """M > 2048 with N = 256, K = 192: patch epilogue, split output, rows >= M.  With today's launch_prec both shapes (3200 x 256
    x 192 patch, 2600 x 256 x 192 split) go to the 128^2 tile kernel with the two-stage ring, launch_tile<128, 128, 2>: N < 1536,
    K < 2048 and fewer than 512 tiles of 256^2.  The persistent 256^2 kernel's SPLIT and EPI_F32_PATCH instantiations are
    launched by name in test_gpu_gemm_edges.py."""
    d = dev()
    dt = hip.h16_dtype(prec)
    frames, n, T, D, K = 200, 16, 4, 256, 192
    A = rnd((frames * n, K), 1.0, 5).to(d).to(dt)
    W = rnd((D, K), K ** -0.5, 6).to(d).to(dt)
    bias, pos, tim = rnd((D,), 1, 7).to(d), rnd((n + 1, D), 1, 8).to(d), rnd((T, D), 1, 9).to(d)
    X = torch.zeros(frames * (n + 1), D, device=d)
    hip.gemm(A, W, bias, X, epilogue=hip.EPI_F32_PATCH, prec=prec, pos=pos, time=tim, n_patches=n, T=T)
    ref = (A.float() @ W.float().t() + bias).view(frames, n, D) + pos[1:].unsqueeze(0) \
        + tim[torch.arange(frames, device=d) % T].unsqueeze(1)
    Xv = X.view(frames, n + 1, D)
    assert torch.allclose(Xv[:, 1:], ref, rtol=1e-4, atol=1e-4)
    assert torch.all(Xv[:, 0] == 0)
    # split output + rows beyond M untouched
    M = 2600
    A2 = rnd((M, K), 1.0, 15).to(d).to(dt)
    out = torch.full((M + 300, 3 * D), 3.0, dtype=dt, device=d)
    hip.gemm(A2, W, bias, out, epilogue=hip.EPI_H16_QGELU, prec=prec, split_out=True, M=M)
    r = A2.float() @ W.float().t() + bias
    r = r * torch.sigmoid(1.702 * r)
    hi, lo = out[:M, :D].float(), out[:M, D:2 * D].float()
    assert torch.equal(out[:M, :D], out[:M, 2 * D:])
    assert torch.all(out[M:] == 3.0)
    assert torch.allclose(hi + lo, r, rtol=3e-5 if prec == hip.PREC_F16 else 3e-4, atol=1e-4)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("size,patch,B,T", [(64, 16, 2, 3), (56, 14, 1, 2), (224, 16, 1, 2)])
def test_gemm_patch_embed_im2col_free(prec, size, patch, B, T):
    """EPI_F32_PATCH with A == NULL: the A tile is built from the NCTHW fp32 frames inside the kernel."""
    d = dev()
    dt = hip.h16_dtype(prec)
    g = size // patch
    n, D = g * g, 128
    K = 3 * patch * patch
    Kp = (K + 63) // 64 * 64
    x = rnd((B, 3, T, size, size), 1.0, 51).to(d)
    Wf = rnd((D, K), K ** -0.5, 52)
    W = torch.zeros(D, Kp); W[:, :K] = Wf
    W = W.to(d).to(dt)
    bias, pos, tim = rnd((D,), 1, 53).to(d), rnd((n + 1, D), 1, 54).to(d), rnd((T, D), 1, 55).to(d)
    X = torch.zeros(B * T * (n + 1), D, device=d)
    hip.gemm(None, W, bias, X, epilogue=hip.EPI_F32_PATCH, prec=prec, pos=pos, time=tim, n_patches=n, T=T,
             M=B * T * n, frames=x, frame_size=size, patch=patch)
    frames = x.permute(0, 2, 1, 3, 4).reshape(B * T, 3, size, size)
    cols = frames.view(B * T, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * T, n, K)
    ref = cols.to(dt).float() @ W[:, :K].float().t() + bias + pos[1:].unsqueeze(0) \
        + tim[torch.arange(B * T, device=d) % T].unsqueeze(1)
    Xv = X.view(B * T, n + 1, D)
    assert torch.allclose(Xv[:, 1:], ref, rtol=1e-4, atol=1e-4)
    assert torch.all(Xv[:, 0] == 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,K_prod", [(777, 768), (5000, 768), (45000, 3072)])   # 128^2 / 128^2 / persistent 256^2 producer
def test_layernorm_folded_into_the_next_gemm(prec, M, K_prod):
    """Producer (EPI_F32 + residual) also emits x16 and per-64-column (sum, sum^2) partials; gava_row_stats turns them
    into (mean, rstd); the consumer GEMM on raw x16 with gamma-scaled weights reproduces LN(x) @ W^T + b
    (DESIGN.md "LayerNorm folding").  Reference: fp32 LayerNorm + fp32 GEMM on the same 16-bit operands."""
    d = dev()
    dt = hip.h16_dtype(prec)
    D = 768
    A = rnd((M, K_prod), 1.0, 1).to(d).to(dt)
    Wp = rnd((D, K_prod), K_prod ** -0.5, 2).to(d).to(dt)
    bp = rnd((D,), 0.3, 3).to(d)
    X = rnd((M, D), 1.0, 4).to(d)
    x_ref = X + A.float() @ Wp.float().t() + bp
    Mp = (M + 255) // 256 * 256
    x16 = torch.zeros(Mp, D, dtype=dt, device=d)
    rowsum = torch.zeros(Mp, D // 64, 2, dtype=torch.float32, device=d)
    hip.gemm(A, Wp, bp, X, epilogue=hip.EPI_F32, prec=prec, resid=X, x16_out=x16, rowsum_out=rowsum)
    assert torch.allclose(X, x_ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(x16[:M], X.to(dt))
    assert torch.allclose(rowsum[:M, :, 0].sum(1), X.sum(1), rtol=1e-4, atol=1e-3)
    assert torch.allclose(rowsum[:M, :, 1].sum(1), (X * X).sum(1), rtol=1e-4, atol=1e-3)
    stats = hip.row_stats(rowsum, D)
    mean, var = X.mean(1), X.var(1, unbiased=False)
    assert torch.allclose(stats[:M, 0], mean, rtol=1e-4, atol=1e-5)
    assert torch.allclose(stats[:M, 1], (var + 1e-5).rsqrt(), rtol=1e-4, atol=1e-5)

    gamma, beta = (1 + rnd((D,), 0.2, 5)).to(d), rnd((D,), 0.2, 6).to(d)
    for N, epi in ((2304, hip.EPI_H16), (3072, hip.EPI_H16_QGELU), (256, hip.EPI_H16)):
        W = rnd((N, D), D ** -0.5, 7).to(d)
        b = rnd((N,), 0.3, 8).to(d)
        Wf = (W * gamma).to(dt)                       # gamma folded into the weight, then rounded
        fs = Wf.float().sum(1).contiguous()
        ft = (W @ beta + b).contiguous()
        out = torch.zeros(M, N, dtype=dt, device=d)
        kw = dict(scale_cols=N // 2, scale=0.125) if epi == hip.EPI_H16 else {}
        hip.gemm(x16[:M], Wf, None, out, epilogue=epi, prec=prec, fold_stats=stats, fold_s=fs, fold_t=ft, **kw)
        # the same operands in fp32: LN of the fp32 row, but the GEMM sees the 16-bit x and the 16-bit folded weight
        xh = x16[:M].float()
        r = (stats[:M, 1:2] * (xh @ Wf.float().t() - stats[:M, 0:1] * fs)) + ft
        if epi == hip.EPI_H16:
            r[:, :N // 2] *= 0.125
        else:
            r = r * torch.sigmoid(1.702 * r)
        tol = 4 * EPS16[prec]
        assert torch.allclose(out.float(), r, rtol=tol, atol=tol * 2), (N, epi)
        # and against the unfolded definition (16-bit rounding of x and gamma*W is the only difference)
        full = torch.nn.functional.layer_norm(X, (D,), gamma, beta) @ W.t() + b
        if epi == hip.EPI_H16:
            full[:, :N // 2] *= 0.125
        else:
            full = full * torch.sigmoid(1.702 * full)
        assert (out.float() - full).abs().max() < 40 * EPS16[prec] * full.abs().max()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,D", [(45000, 768), (20000, 1024), (300, 768)])
def test_layernorm_folding_without_the_row_stats_launch(prec, M, D):
    """rowsum_reduced / fold_partials (gava_hip.h): the persistent producer pre-reduces its (sum, sum^2) per 256-column tile
    (a fixed-order sum of its four waves' partials, exchanged through LDS) and the persistent consumer derives (mean, rstd)
    of its rows itself - same results as the three-launch form (producer, gava_row_stats, consumer) up to the summation
    order of the statistics, and deterministic.  M = 300: a single ragged tile; D = 1024: four slots (ViT-L/14)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    Kp = 768
    A = rnd((M, Kp), 1.0, 1).to(d).to(dt)
    Wp = rnd((D, Kp), Kp ** -0.5, 2).to(d).to(dt)
    bp = rnd((D,), 0.3, 3).to(d)
    X0 = (rnd((M, D), 1.0, 4) + 0.7).to(d)            # a non-zero mean, so that E[x^2] - mean^2 is exercised
    Mp = (M + 255) // 256 * 256
    X = X0.clone()
    x16 = torch.zeros(Mp, D, dtype=dt, device=d)
    part = torch.full((Mp + 32, 4, 2), float("nan"), dtype=torch.float32, device=d)   # unwritten slots must never be read
    hip.gemm(A, Wp, bp, X, epilogue=hip.EPI_F32, prec=prec, resid=X, x16_out=x16, rowsum_out=part, rowsum_reduced=True)
    slots = D // 256
    assert torch.isfinite(part[:M, :slots]).all()
    assert torch.allclose(part[:M, :slots, 0].sum(1), X.sum(1), rtol=1e-4, atol=2e-3)
    assert torch.allclose(part[:M, :slots, 1].sum(1), (X * X).sum(1), rtol=1e-4, atol=2e-3)
    # the three-launch form on the same inputs
    X2, x16b = X0.clone(), torch.zeros(Mp, D, dtype=dt, device=d)
    rowsum = torch.zeros(Mp, D // 64, 2, dtype=torch.float32, device=d)
    hip.gemm(A, Wp, bp, X2, epilogue=hip.EPI_F32, prec=prec, resid=X2, x16_out=x16b, rowsum_out=rowsum)
    assert torch.equal(X, X2) and torch.equal(x16, x16b)
    stats = hip.row_stats(rowsum, D)
    gamma, beta = (1 + rnd((D,), 0.2, 5)).to(d), rnd((D,), 0.2, 6).to(d)
    for N, epi in ((3 * D, hip.EPI_H16), (4 * D, hip.EPI_H16_QGELU)):
        W = rnd((N, D), D ** -0.5, 7).to(d)
        b = rnd((N,), 0.3, 8).to(d)
        Wf = (W * gamma).to(dt)
        fs, ft = Wf.float().sum(1).contiguous(), (W @ beta + b).contiguous()
        kw = dict(scale_cols=N // 3, scale=0.125) if epi == hip.EPI_H16 else {}
        a = torch.zeros(M, N, dtype=dt, device=d)
        b1 = torch.zeros(M, N, dtype=dt, device=d)
        b2 = torch.zeros(M, N, dtype=dt, device=d)
        hip.gemm(x16[:M], Wf, None, a, epilogue=epi, prec=prec, fold_stats=stats, fold_s=fs, fold_t=ft, **kw)
        hip.gemm(x16[:M], Wf, None, b1, epilogue=epi, prec=prec, fold_partials=part, fold_s=fs, fold_t=ft, **kw)
        hip.gemm(x16[:M], Wf, None, b2, epilogue=epi, prec=prec, fold_partials=part, fold_s=fs, fold_t=ft, **kw)
        assert torch.equal(b1, b2)
        tol = 4 * EPS16[prec]
        assert torch.allclose(a.float(), b1.float(), rtol=tol, atol=tol * 2), (N, epi)
        full = torch.nn.functional.layer_norm(X, (D,), gamma, beta) @ W.t() + b
        if epi == hip.EPI_H16:
            full[:, :N // 3] *= 0.125
        else:
            full = full * torch.sigmoid(1.702 * full)
        assert float((b1.float() - full).abs().max()) < 40 * EPS16[prec] * float(full.abs().max())
    # only the persistent kernel implements the mode: a shape it does not take is rejected, not routed elsewhere
    with pytest.raises(hip.GavaError):
        hip.gemm(A[:, :128].contiguous(), rnd((128, 128), 0.1, 9).to(d).to(dt), None, torch.zeros(M, 128, dtype=dt, device=d),
                 epilogue=hip.EPI_H16, prec=prec, fold_partials=part, fold_s=fs[:128].contiguous(), fold_t=ft[:128].contiguous())


@pytest.mark.parametrize("mode", ["partials", "stats"])
def test_layernorm_fold_with_outlier_channels(mode):
    """the folded LayerNorm takes its statistics from sum / sum-of-squares of the un-normalised stream and feeds the
    GEMM a 16-bit copy of it.  Real CLIP activations carry a few channels with a large, constant offset; here three channels
    sit at +60 / -45 / +25 on top of unit-variance data (row mean ~ 0.05, row variance ~ 8.6: E[x^2] - mean^2 keeps its
    digits, but the fp16 copy of an outlier carries 0.03 of absolute rounding).  The folded GEMM must stay within the 16-bit
    operand rounding of the unfolded LayerNorm + GEMM on the same inputs - measured and asserted, fp16 and bf16."""
    d = dev()
    M, D, N = 9000, 768, 1024
    X = rnd((M, D), 1.0, 11).to(d)
    X[:, 17] += 60.0
    X[:, 300] -= 45.0
    X[:, 555] += 25.0
    gamma, beta = (1 + rnd((D,), 0.2, 5)).to(d), rnd((D,), 0.2, 6).to(d)
    W = rnd((N, D), D ** -0.5, 7).to(d)
    b = rnd((N,), 0.3, 8).to(d)
    full = torch.nn.functional.layer_norm(X, (D,), gamma, beta) @ W.t() + b
    for prec in PRECS:
        dt = hip.h16_dtype(prec)
        # a producer that reproduces X exactly: X = 0 * A W^T + resid
        A = torch.zeros(M, 64, dtype=dt, device=d)
        Wz = torch.zeros(D, 64, dtype=dt, device=d)
        Xo = X.clone()
        Mp = (M + 255) // 256 * 256
        x16 = torch.zeros(Mp, D, dtype=dt, device=d)
        Wf = (W * gamma).to(dt)
        fs, ft = Wf.float().sum(1).contiguous(), (W @ beta + b).contiguous()
        out = torch.zeros(M, N, dtype=dt, device=d)
        if mode == "partials":
            part = torch.zeros(Mp + 32, 4, 2, device=d)
            hip.gemm(A, Wz, None, Xo, epilogue=hip.EPI_F32, prec=prec, resid=Xo, x16_out=x16, rowsum_out=part, rowsum_reduced=True)
            hip.gemm(x16[:M], Wf, None, out, epilogue=hip.EPI_H16, prec=prec, fold_partials=part, fold_s=fs, fold_t=ft)
        else:
            rowsum = torch.zeros(Mp, D // 64, 2, device=d)
            hip.gemm(A, Wz, None, Xo, epilogue=hip.EPI_F32, prec=prec, resid=Xo, x16_out=x16, rowsum_out=rowsum)
            hip.gemm(x16[:M], Wf, None, out, epilogue=hip.EPI_H16, prec=prec, fold_stats=hip.row_stats(rowsum, D), fold_s=fs, fold_t=ft)
        assert torch.equal(Xo, X)
        # the unfolded path of the same precision: LayerNorm in fp32, its OUTPUT rounded to 16 bits, plain GEMM
        xn16 = torch.zeros(M, D, dtype=dt, device=d)
        hip.layernorm(X, gamma, beta, out16=xn16, prec=prec)
        plain = torch.zeros(M, N, dtype=dt, device=d)
        hip.gemm(xn16, W.to(dt), b, plain, epilogue=hip.EPI_H16, prec=prec)
        scale = float(full.abs().max())
        e_fold = float((out.float() - full).abs().max()) / scale
        e_plain = float((plain.float() - full).abs().max()) / scale
        print(f"\n[outliers/{mode}/prec {prec}] max error / max|ref|: folded {e_fold:.2e}, unfolded {e_plain:.2e}")
        assert e_fold < 12 * EPS16[prec], (mode, prec, e_fold)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 768, 768), (4133, 1024, 256), (129, 512, 3072), (7, 768, 128),
                                   (45056, 768, 768), (33001, 768, 3072)])
def test_gemm_pair_kernel(prec, M, N, K):
    """The two-workgroups-per-CU 128 x 256 kernel (gava_gemm_args.kernel = GAVA_KERNEL_PAIR: never taken automatically - it
    measured slower than the 256^2 kernel, DESIGN.md "Round 3") named explicitly on small, ragged and full-size shapes: plain fp32 output,
    fp32 residual (in place and from another buffer with its own stride), and the folding-producer form (16-bit copy +
    per-256-column row sums) - against torch on the same rounded operands, bit for bit against the 256^2 kernel (same
    k order: the two kernels differ in tiling only), rows beyond M untouched."""
    d = dev()
    dt = hip.h16_dtype(prec)
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = rnd((N, K), K ** -0.5, 2).to(d).to(dt)
    bias = rnd((N,), 0.5, 3).to(d)
    ref = A.float() @ W.float().t() + bias
    pad = 256
    # plain, no bias, rows beyond M must stay
    out = torch.full((M + pad, N), 7.0, dtype=torch.float32, device=d)
    hip.gemm(A, W, None, out, epilogue=hip.EPI_F32, prec=prec, M=M, kernel=hip.KERNEL_PAIR)
    assert torch.all(out[M:] == 7.0)
    assert torch.allclose(out[:M], ref - bias, rtol=1e-4, atol=1e-4)
    # residual from another buffer with a wider stride
    Rbuf = rnd((M, N + 64), 1.0, 4).to(d)
    out2 = torch.zeros(M, N, dtype=torch.float32, device=d)
    hip.gemm(A, W, bias, out2, epilogue=hip.EPI_F32, prec=prec, resid=Rbuf[:, :N], kernel=hip.KERNEL_PAIR)
    assert torch.allclose(out2, Rbuf[:, :N] + ref, rtol=1e-4, atol=1e-4)
    ref256 = torch.zeros(M, N, dtype=torch.float32, device=d)
    hip.gemm(A, W, bias, ref256, epilogue=hip.EPI_F32, prec=prec, resid=Rbuf[:, :N], kernel=hip.KERNEL_256)
    assert torch.equal(out2, ref256)
    # folding producer, in place
    Mp = (M + 255) // 256 * 256
    X = Rbuf[:, :N].contiguous()
    x16 = torch.full((Mp, N), 3.0, dtype=dt, device=d)
    part = torch.full((Mp + 32, 4, 2), float("nan"), dtype=torch.float32, device=d)
    hip.gemm(A, W, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, x16_out=x16, rowsum_out=part, rowsum_reduced=True,
             kernel=hip.KERNEL_PAIR)
    assert torch.equal(X, out2)
    assert torch.equal(x16[:M], X.to(dt)) and torch.all(x16[M:] == 3.0)
    slots = N // 256
    assert torch.isfinite(part[:M, :slots]).all() and torch.isnan(part[M:]).all() and torch.isnan(part[:, slots:]).all()
    Xs = X.view(M, slots, 256)
    assert torch.allclose(part[:M, :slots, 0], Xs.sum(2), rtol=1e-4, atol=2e-3)
    assert torch.allclose(part[:M, :slots, 1], (Xs * Xs).sum(2), rtol=1e-4, atol=2e-3)
    # deterministic
    X2 = Rbuf[:, :N].contiguous()
    part2 = torch.full_like(part, float("nan"))
    hip.gemm(A, W, bias, X2, epilogue=hip.EPI_F32, prec=prec, resid=X2, x16_out=x16, rowsum_out=part2, rowsum_reduced=True,
             kernel=hip.KERNEL_PAIR)
    assert torch.equal(X, X2) and torch.equal(part[:M, :slots], part2[:M, :slots])


def test_gemm_named_kernel_rejects_what_it_does_not_take():
    d = dev()
    A = rnd((300, 192)).to(d).half()
    W = rnd((256, 192)).to(d).half()
    with pytest.raises(hip.GavaError):       # K % 128 != 0
        hip.gemm(A, W, None, torch.zeros(300, 256, device=d), epilogue=hip.EPI_F32, prec=hip.PREC_F16, kernel=hip.KERNEL_PAIR)
    with pytest.raises(hip.GavaError):       # 16-bit output
        hip.gemm(A[:, :128].contiguous(), W[:, :128].contiguous(), None, torch.zeros(300, 256, device=d).half(),
                 epilogue=hip.EPI_H16, prec=hip.PREC_F16, kernel=hip.KERNEL_PAIR)
    with pytest.raises(hip.GavaError):       # unknown kernel id
        hip.gemm(A, W, None, torch.zeros(300, 256, device=d), epilogue=hip.EPI_F32, prec=hip.PREC_F16, kernel=9)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch,heads,L,causal,split", [(3, 8, 77, True, True), (5, 2, 17, True, False), (2, 12, 128, False, True),
                                                      (400, 8, 19, True, True), (1, 1, 1, True, False)])
def test_attention_f32_core(prec, batch, heads, L, causal, split):
    """gava_attention_f32 (the text tower's softmax core in inference): fp32 q/k/v in, scores / softmax / P.V in fp32, only
    the output is rounded - to 16 bits, or to a [hi | lo | hi] pair whose hi + lo carries ~22 bits."""
    d = dev()
    dt = hip.h16_dtype(prec)
    Wd = heads * 64
    qkv = rnd((batch * L, 3 * Wd), 1.0, 11).to(d)
    S = 3 if split else 1
    out = torch.zeros(batch * L, S * Wd, dtype=dt, device=d)
    hip.attention_f32(qkv[:, :Wd], qkv[:, Wd:2 * Wd], qkv[:, 2 * Wd:], out, batch=batch, heads=heads, L=L, prec=prec,
                      causal=causal, split_out=split, scale=0.125)
    q, k, v = (qkv[:, i * Wd:(i + 1) * Wd].reshape(batch, L, heads, 64).permute(0, 2, 1, 3).double() for i in range(3))
    sc = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        sc = sc + torch.full((L, L), float("-inf"), device=d, dtype=torch.float64).triu(1)
    ref = (sc.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(batch * L, Wd)
    if split:
        hi, lo = out[:, :Wd].double(), out[:, Wd:2 * Wd].double()
        assert torch.equal(out[:, :Wd], out[:, 2 * Wd:])
        got, tol = hi + lo, 4 * EPS16[prec] ** 2 + 2e-6          # two 16-bit words: the error is fp32's
    else:
        got, tol = out.double(), 2 * EPS16[prec]
    assert float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
    with pytest.raises(hip.GavaError):
        hip.attention_f32(qkv[:, :Wd], qkv[:, Wd:2 * Wd], qkv[:, 2 * Wd:], out, batch=1, heads=heads, L=129, prec=prec)


def _hi_lo(W, dt):
    hi = W.to(dt)
    return hi, (W - hi.float()).to(dt)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (1000, 384, 768), (4100, 768, 768), (45000, 768, 3072), (30000, 2304, 768)])
def test_gemm_weight_lo_pass(prec, M, N, K):
    """gava_gemm_args.w_lo = 1: W packed [W_hi | W_lo], the k-loop runs 2K deep and re-reads A.  The product must equal
    A16 . (W_hi + W_lo)^T, i.e. the 16-bit ACTIVATIONS times the (almost) exact weights - and be far closer to A16 . W^T
    than the plain 16-bit GEMM, whose error is the rounding of W (VERDICT r3 / tools/error_budget.py).  Shapes cover the
    128^2 tile kernel, the persistent 256^2 kernel (fp32 output with residual: fc2 / out_proj; 16-bit output: qkv)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    Wf = rnd((N, K), K ** -0.5, 2).to(d)
    hi, lo = _hi_lo(Wf, dt)
    Wp = torch.cat([hi, lo], 1).contiguous()
    bias = rnd((N,), 0.5, 3).to(d)
    exact = A.double() @ Wf.double().t() + bias.double()
    X0 = rnd((M, N), 1.0, 4).to(d)
    X = X0.clone()
    hip.gemm(A, Wp, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, w_lo=1)
    want = (X0.double() + A.double() @ (hi.double() + lo.double()).t() + bias.double())
    assert torch.allclose(X.double(), want, rtol=2e-5, atol=2e-5)
    Y = X0.clone()
    hip.gemm(A, hi.contiguous(), bias, Y, epilogue=hip.EPI_F32, prec=prec, resid=Y)
    e_lo = float((X.double() - X0.double() - exact).abs().max()); e_plain = float((Y.double() - X0.double() - exact).abs().max())
    print(f"\n[w_lo {M}x{N}x{K} prec {prec}] max error vs A16.W^T: with lo {e_lo:.2e}, plain {e_plain:.2e}")
    assert e_lo < 0.12 * e_plain
    # 16-bit output epilogues
    out = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, Wp, bias, out, epilogue=hip.EPI_H16_QGELU, prec=prec, w_lo=1)
    r = (want - X0.double()).float()
    r = r * torch.sigmoid(1.702 * r)
    tol = 4 * EPS16[prec]
    assert torch.allclose(out.float(), r, rtol=tol, atol=2 * tol)
    # rejected: the pair kernel has no lo pass; ldw must cover both halves
    with pytest.raises(hip.GavaError):
        hip.gemm(A, Wp, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, w_lo=1, kernel=hip.KERNEL_PAIR)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, hi.contiguous(), bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, w_lo=1, K=K)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_weight_lo_with_folded_layernorm_and_patch_loader(prec):
    """w_lo = 1 together with the consumers' LayerNorm fold (fold_s = row sums of hi + lo; stats and partials modes) and with
    the im2col-free patch loader (the A tile is rebuilt for the second half of the k-loop)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    M, D = 20000, 768
    X = (rnd((M, D), 1.0, 4) + 0.3).to(d)
    x16 = X.to(dt)
    Mp = (M + 255) // 256 * 256
    part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
    xf = x16.float()          # the statistics are those of the fp32 stream
    for sl in range(D // 256):
        seg = X[:, sl * 256:(sl + 1) * 256]
        part[:M, sl, 0], part[:M, sl, 1] = seg.sum(1), (seg * seg).sum(1)
    mean, var = X.mean(1), X.var(1, unbiased=False)
    stats = torch.zeros(Mp, 2, device=d); stats[:M, 0], stats[:M, 1] = mean, (var + 1e-5).rsqrt()
    gamma, beta = (1 + rnd((D,), 0.2, 5)).to(d), rnd((D,), 0.2, 6).to(d)
    N = 2304
    W = rnd((N, D), D ** -0.5, 7).to(d)
    b = rnd((N,), 0.3, 8).to(d)
    hi, lo = _hi_lo(W * gamma, dt)
    Wp = torch.cat([hi, lo], 1).contiguous()
    fs, ft = (hi.float() + lo.float()).sum(1).contiguous(), (W @ beta + b).contiguous()
    want = stats[:M, 1:2] * (xf @ (hi.float() + lo.float()).t() - stats[:M, 0:1] * fs) + ft
    for kw in (dict(fold_stats=stats), dict(fold_partials=part)):
        out = torch.zeros(M, N, dtype=dt, device=d)
        hip.gemm(x16, Wp, None, out, epilogue=hip.EPI_H16, prec=prec, fold_s=fs, fold_t=ft, w_lo=1, **kw)
        tol = 4 * EPS16[prec]
        assert torch.allclose(out.float(), want, rtol=tol, atol=2 * tol), list(kw)
    # patch loader
    size, patch, B, T, Dp = 64, 16, 2, 3, 128
    g = size // patch
    n, K = g * g, 3 * patch * patch
    x = rnd((B, 3, T, size, size), 1.0, 51).to(d)
    Wf = rnd((Dp, K), K ** -0.5, 52).to(d)
    hi, lo = _hi_lo(Wf, dt)
    bias, pos, tim = rnd((Dp,), 1, 53).to(d), rnd((n + 1, Dp), 1, 54).to(d), rnd((T, Dp), 1, 55).to(d)
    Xo = torch.zeros(B * T * (n + 1), Dp, device=d)
    hip.gemm(None, torch.cat([hi, lo], 1).contiguous(), bias, Xo, epilogue=hip.EPI_F32_PATCH, prec=prec, pos=pos, time=tim, n_patches=n, T=T,
             M=B * T * n, frames=x, frame_size=size, patch=patch, w_lo=1)
    frames = x.permute(0, 2, 1, 3, 4).reshape(B * T, 3, size, size)
    cols = frames.view(B * T, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * T, n, K)
    ref = cols.to(dt).float() @ (hi.float() + lo.float()).t() + bias + pos[1:].unsqueeze(0) + tim[torch.arange(B * T, device=d) % T].unsqueeze(1)
    assert torch.allclose(Xo.view(B * T, n + 1, Dp)[:, 1:], ref, rtol=2e-5, atol=2e-5)


def _bf8(t):
    """bf8 (e5m2) bytes of a tensor, rounded to nearest even on the host - what the kernels' v_cvt_pk_bf8_f32 produces."""
    return t.float().cpu().to(torch.float8_e5m2)


def _a8_rows(a16, pitch):
    M, K = a16.shape
    buf = torch.zeros(M, pitch, dtype=torch.uint8)
    buf[:, :K] = _bf8(a16).view(torch.uint8)
    return buf


# (the last one: the kernel's minimum K = 128, one 8-bit stage per tile, on 8 workgroups - 16 tiles, two per workgroup, so that the
# tile switch inside the 8-bit loop runs at nk8 = 1)
@pytest.mark.parametrize("M,N,K,kind,cu_reserve", [(45056, 768, 3072, "fc2", 0), (20000, 2304, 768, "qkv", 0), (300, 3072, 768, "fc1", 0),
                                                   (5000, 768, 768, "fc2", 0), (3900, 256, 128, "fc2", EIGHT_WORKGROUPS)],
                         ids=["45056-768-3072-fc2", "20000-2304-768-qkv", "300-3072-768-fc1", "5000-768-768-fc2", "3900-256-128-fc2-wg8"])
def test_gemm_weight_lo_pass_at_8_bits(M, N, K, kind, cu_reserve):
    """gava_gemm_args.w_lo = 2: after the K-deep fp16 loop the persistent kernel runs K / 128 stages of
    v_mfma_scale_f32_16x16x128_f8f6f4 on A8 = bf8(A) and W8 = e4m3(2^e (W - W_hi)) into the same accumulators.  Checked
    against exactly that arithmetic on the host (A16 . W_hi^T + A8 . W8^T 2^-e in fp64), then against A16 . W^T (the point of
    it: the weight rounding is gone up to the 8-bit lo's own ~6 %).  fc2 / out form: fp32 residual epilogue with the x16 + x8
    copies; qkv / fc1 form: LayerNorm-folded consumer with the out8 copy."""
    d = dev()
    prec, dt = hip.PREC_F16, torch.float16
    Wf = rnd((N, K), K ** -0.5, 2).to(d)
    hi, w8, e8, s8 = hip.pack_w8(Wf, prec)
    hl = torch.cat([hi, (Wf - hi.float()).to(dt)], 1).contiguous()                  # the [W_hi | W_lo] rows the model packs
    w8deq = w8[:, :K].view(torch.float8_e4m3fn).float().double() * 2.0 ** -e8
    if kind == "fc2":
        A = rnd((M, K), 1.0, 1).to(d).to(dt)
        A8 = _a8_rows(A, 2 * K).to(d)
        bias = rnd((N,), 0.5, 3).to(d)
        X0 = rnd((M, N), 1.0, 4).to(d)
        X = X0.clone()
        Mp = (M + 255) // 256 * 256
        x16 = torch.zeros(Mp, N, dtype=dt, device=d)
        x8 = torch.zeros(Mp, 2 * N, dtype=torch.uint8, device=d)
        part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
        hip.gemm(A, hl, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, w_lo=2, K=K, A8=A8, W8=w8, w8_exp=e8,
                 x16_out=x16, rowsum_out=part, rowsum_reduced=True, x8_out=x8, cu_reserve=cu_reserve)
        want = X0.double() + A.double() @ hi.double().t() + _bf8(A).float().double().to(d) @ w8deq.t() + bias.double()
        assert torch.allclose(X.double(), want, rtol=2e-5, atol=2e-5)
        exact = X0.double() + A.double() @ Wf.double().t() + bias.double()
        Y = X0.clone()
        hip.gemm(A, hi.contiguous(), bias, Y, epilogue=hip.EPI_F32, prec=prec, resid=Y)
        e_lo, e_plain = float((X.double() - exact).abs().max()), float((Y.double() - exact).abs().max())
        print(f"\n[w_lo=2 {M}x{N}x{K}] max error vs A16.W^T: 8-bit lo {e_lo:.2e}, plain fp16 weights {e_plain:.2e}")
        assert e_lo < 0.2 * e_plain
        assert torch.equal(x16[:M], X.to(dt))
        assert torch.equal(x8[:M, :N].cpu(), _bf8(x16[:M]).view(torch.uint8))
        with pytest.raises(hip.GavaError):      # the 8-bit rows must keep the byte pitch of their 16-bit twins
            hip.gemm(A, hl, bias, X, epilogue=hip.EPI_F32, prec=prec, resid=X, w_lo=2, K=K, A8=A8[:, :K].contiguous(), W8=w8, w8_exp=e8)
        return
    # folded consumers: x16 = the un-normalised stream, W = gamma-folded weight
    D = K
    X = (rnd((M, D), 1.0, 4) + 0.3).to(d)
    x16 = X.to(dt)
    A8 = _a8_rows(x16, 2 * D).to(d)
    Mp = (M + 255) // 256 * 256
    part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
    for sl in range(D // 256):
        seg = X[:, sl * 256:(sl + 1) * 256]
        part[:M, sl, 0], part[:M, sl, 1] = seg.sum(1), (seg * seg).sum(1)
    mean, var = X.mean(1), X.var(1, unbiased=False)
    stats = torch.zeros(Mp, 2, device=d); stats[:M, 0], stats[:M, 1] = mean, (var + 1e-5).rsqrt()
    ft = rnd((N,), 0.3, 8).to(d)
    epi = hip.EPI_H16 if kind == "qkv" else hip.EPI_H16_QGELU
    acc = x16.double() @ hi.double().t() + _bf8(x16).float().double().to(d) @ w8deq.t()
    want = (stats[:M, 1:2].double() * (acc - stats[:M, 0:1].double() * s8.double()) + ft.double()).float()
    if epi == hip.EPI_H16_QGELU:
        want = want * torch.sigmoid(1.702 * want)
    tol = 4 * EPS16[prec]
    for kw in (dict(fold_stats=stats), dict(fold_partials=part)):
        out = torch.zeros(M, N, dtype=dt, device=d)
        out8 = torch.zeros(M, 2 * N, dtype=torch.uint8, device=d)
        hip.gemm(x16, hl, None, out, epilogue=epi, prec=prec, fold_s=s8, fold_t=ft, w_lo=2, K=K, A8=A8, W8=w8, w8_exp=e8, out8=out8, cu_reserve=cu_reserve, **kw)
        assert torch.allclose(out.float(), want, rtol=tol, atol=2 * tol), list(kw)
        got8 = out8[:, :N].cpu().view(torch.float8_e5m2).float()
        assert torch.allclose(got8, out.float().cpu(), rtol=0.13, atol=1e-4)      # bf8: 2 mantissa bits


def test_gemm_weight_lo_8_bit_rejects_what_it_does_not_take():
    d = dev()
    A = rnd((512, 256), 1.0, 1).to(d).half()
    Wf = rnd((256, 256), 0.06, 2).to(d)
    hi, w8, e8, s8 = hip.pack_w8(Wf, hip.PREC_F16)
    hl = torch.cat([hi, (Wf - hi.float()).half()], 1).contiguous()
    A8 = _a8_rows(A, 512).to(d)
    out = torch.zeros(512, 256, dtype=torch.float16, device=d)
    with pytest.raises(hip.GavaError):       # plain 16-bit-output GEMM (no LayerNorm fold): no 8-bit instantiation
        hip.gemm(A, hl, None, out, epilogue=hip.EPI_H16, prec=hip.PREC_F16, w_lo=2, K=256, A8=A8, W8=w8, w8_exp=e8)
    with pytest.raises(hip.GavaError):       # bf16 operands
        hip.gemm(A.bfloat16(), hl.bfloat16(), None, torch.zeros(512, 256, device=d), epilogue=hip.EPI_F32, prec=hip.PREC_BF16,
                 resid=torch.zeros(512, 256, device=d), w_lo=2, K=256, A8=A8, W8=w8, w8_exp=e8)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (300, 512, 256), (5000, 768, 768), (20000, 2304, 768), (1000, 256, 3072), (70000, 768, 768)])
def test_gemm_ping_pong_kernel(prec, M, N, K):
    """GAVA_KERNEL_PP (gemm256_kernel<..., PP>): four 16-MFMA phases per k-tile, the wave groups one barrier apart, half-tiles
    staged six ahead through the tile switch.  Same k order as the default loop -> bit-identical 16-bit outputs; ragged M, bias,
    rows beyond M untouched, several tiles per workgroup (M = 70000: 822 tiles on 256 workgroups)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = rnd((N, K), K ** -0.5, 2).to(d).to(dt)
    bias = rnd((N,), 0.5, 3).to(d)
    out = torch.full((M + 7, N), 3.0, dtype=dt, device=d)
    hip.gemm(A, W, bias, out, epilogue=hip.EPI_H16, prec=prec, kernel=hip.KERNEL_PP, M=M)
    ref = A.float() @ W.float().t() + bias
    tol = 4 * EPS16[prec]
    assert torch.allclose(out[:M].float(), ref, rtol=tol, atol=2 * tol)
    assert torch.all(out[M:] == 3.0)
    o2 = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, bias, o2, epilogue=hip.EPI_H16, prec=prec, kernel=hip.KERNEL_256)
    assert torch.equal(out[:M], o2)
    for _ in range(3):      # the schedule has no data-dependent path: repeated runs are bit-identical
        o3 = torch.zeros(M, N, dtype=dt, device=d)
        hip.gemm(A, W, bias, o3, epilogue=hip.EPI_H16, prec=prec, kernel=hip.KERNEL_PP)
        assert torch.equal(o3, o2)
    with pytest.raises(hip.GavaError):       # K % 128 != 0
        hip.gemm(A[:, :192].contiguous(), W[:, :192].contiguous(), None, o2, epilogue=hip.EPI_H16, prec=prec, kernel=hip.KERNEL_PP)


@pytest.mark.parametrize("prec", PRECS)
# (the last one: the form's minimum K = 256 (and 1024) on 8 workgroups - 24 tiles, three per workgroup through the tile switch)
@pytest.mark.parametrize("M,D,cu_reserve", [(45000, 768, 0), (300, 768, 0), (20000, 1024, 0), (100864, 768, 0), (6000, 256, EIGHT_WORKGROUPS)],
                         ids=["45000-768", "300-768", "20000-1024", "100864-768", "6000-256-wg8"])
def test_gemm_residual_stream_as_16_bit_pair(prec, M, D, cu_reserve):
    """gava_gemm_args.resid16 (gemm256_kernel<..., HL>): the residual producers reading and writing the stream as hi = h16(x),
    lo = fp16(x - hi).  Against the fp32-stream kernel on the same inputs (resid = hi + lo, exact in fp32): the hi half is its
    x16 copy bit for bit (same k order, same fp32 x), the row sums are its row sums to fp32 rounding, hi + lo is its fp32 output to 2^-21 |x|
    (2^-19 with bf16 operands; never better than 2^-24 absolute: fp16 subnormals), lo bit for bit fp16(x - hi); rows beyond M untouched; in place (out pair = in pair) equals out of place; the aligned and the
    plain tile walk (M = 100864 / the smaller ones); both K of the forward; the weight-lo pass; what the ABI rejects."""
    d = dev()
    dt = hip.h16_dtype(prec)
    Mp = (M + 255) // 256 * 256
    rel = 2.0 ** -21 if prec == hip.PREC_F16 else 2.0 ** -19
    for K in (D, 4 * D):
        A = rnd((M, K), 1.0, 1).to(d).to(dt)
        W = rnd((D, K), K ** -0.5, 2).to(d).to(dt)
        b = rnd((D,), 0.3, 3).to(d)
        X0 = ((rnd((M, D), 1.0, 4) + 0.5) * 3).to(d)
        hi0 = X0.to(dt)
        lo0 = (X0 - hi0.float()).half()
        Xp = hi0.float() + lo0.float()                      # the stream the pair represents
        Y = torch.zeros(M, D, device=d)
        x16 = torch.zeros(Mp, D, dtype=dt, device=d)
        part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
        hip.gemm(A, W, b, Y, epilogue=hip.EPI_F32, prec=prec, resid=Xp, x16_out=x16, rowsum_out=part, rowsum_reduced=True, kernel=hip.KERNEL_PP, cu_reserve=cu_reserve)
        hi = torch.full((Mp + 8, D), 7.0, dtype=dt, device=d)
        lo = torch.full((Mp + 8, D), 7.0, dtype=torch.float16, device=d)
        part2 = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
        hip.gemm(A, W, b, None, epilogue=hip.EPI_F32, prec=prec, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo, rowsum_out=part2,
                 rowsum_reduced=True, cu_reserve=cu_reserve)
        assert torch.equal(hi[:M], x16[:M]), K
        # (a lane adds its 16 columns in another order than the fp32-output layout's lane does: equal to fp32 rounding, not bit for bit)
        assert torch.allclose(part2[:M, :D // 256], part[:M, :D // 256], rtol=2e-6, atol=1e-4), K
        assert torch.all(hi[M:].float() == 7.0) and torch.all(lo[M:].float() == 7.0)
        back = hi[:M].float() + lo[:M].float()
        # (fp16 subnormals below 6.1e-5 are 2^-24 apart: the lo of an |x| < 0.06 carries an absolute error of up to 2^-25)
        assert bool(((back - Y).abs() <= torch.maximum(rel * Y.abs(), torch.full_like(Y, 2.0 ** -24))).all()), K
        assert torch.equal(lo[:M], (Y - x16[:M].float()).half()), K
        # in place
        hi_ip, lo_ip = hi0.clone(), lo0.clone()
        if hi_ip.shape[0] < Mp:
            hi_ip = torch.cat([hi_ip, torch.zeros(Mp - M, D, dtype=dt, device=d)]); lo_ip = torch.cat([lo_ip, torch.zeros(Mp - M, D, dtype=torch.float16, device=d)])
        hip.gemm(A, W, b, None, epilogue=hip.EPI_F32, prec=prec, resid16=hi_ip, resid_lo=lo_ip, x16_out=hi_ip, xlo_out=lo_ip, rowsum_out=part2,
                 rowsum_reduced=True, M=M, cu_reserve=cu_reserve)
        assert torch.equal(hi_ip[:M], hi[:M]) and torch.equal(lo_ip[:M], lo[:M]), K
    # weight-lo pass (w_lo = 1) with the pair: against the fp32-stream kernel with the same packed weight
    K = D
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    Wf = rnd((D, K), K ** -0.5, 2).to(d)
    Wh = Wf.to(dt)
    Wp = torch.cat([Wh, (Wf - Wh.float()).to(dt)], 1).contiguous()
    hip.gemm(A, Wp, b, Y, epilogue=hip.EPI_F32, prec=prec, resid=Xp, x16_out=x16, rowsum_out=part, rowsum_reduced=True, kernel=hip.KERNEL_PP, w_lo=1, cu_reserve=cu_reserve)
    hip.gemm(A, Wp, b, None, epilogue=hip.EPI_F32, prec=prec, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo, rowsum_out=part2, rowsum_reduced=True, w_lo=1, cu_reserve=cu_reserve)
    assert torch.equal(hi[:M], x16[:M]) and torch.allclose(part2[:M, :D // 256], part[:M, :D // 256], rtol=2e-6, atol=1e-4)
    # rejected: an fp32 output or residual beside the pair, a missing half, a kernel that does not implement it, K % 128
    kw = dict(epilogue=hip.EPI_F32, prec=prec, rowsum_out=part2, rowsum_reduced=True)
    for bad in (dict(out=Y, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo), dict(out=None, resid=Xp, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo),
                dict(out=None, resid16=hi0, x16_out=hi, xlo_out=lo), dict(out=None, resid16=hi0, resid_lo=lo0, x16_out=hi),
                dict(out=None, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo, kernel=hip.KERNEL_256),
                dict(out=Y, resid=Xp, x16_out=hi, xlo_out=lo)):
        with pytest.raises(hip.GavaError):
            bad = dict(bad); o = bad.pop("out")
            hip.gemm(A, Wh, b, o, **kw, **bad)
    with pytest.raises(hip.GavaError):
        hip.gemm(A[:, :192].contiguous(), Wh[:, :192].contiguous(), b, None, resid16=hi0, resid_lo=lo0, x16_out=hi, xlo_out=lo, **kw)


def test_layernorm_and_join_rows_of_the_16_bit_pair():
    """gava_layernorm_args.out_hi / out_lo: the pair of the FIRST LayerNorm's result beside the fused second one (ln_pre + norm1 of
    block 0), and of a plain LayerNorm; hi = h16(y) bit for bit, hi + lo = y to 2^-21."""
    d = dev()
    for prec in PRECS:
        dt = hip.h16_dtype(prec)
        x = (rnd((1000, 768), 2.0, 1) + 0.3).to(d)
        g1, b1, g2, b2 = ((1 + rnd((768,), 0.2, 2)).to(d), rnd((768,), 0.2, 3).to(d), (1 + rnd((768,), 0.2, 4)).to(d), rnd((768,), 0.2, 5).to(d))
        y32 = torch.zeros_like(x); o16 = torch.zeros(1000, 768, dtype=dt, device=d)
        hip.layernorm(x, g1, b1, out16=o16, out32=y32, prec=prec, gamma2=g2, beta2=b2)
        hi = torch.zeros(1000, 768, dtype=dt, device=d); lo = torch.zeros(1000, 768, dtype=torch.float16, device=d)
        o16b = torch.zeros_like(o16)
        hip.layernorm(x, g1, b1, out16=o16b, prec=prec, gamma2=g2, beta2=b2, out_hi=hi, out_lo=lo)
        assert torch.equal(o16, o16b)
        assert torch.equal(hi, y32.to(dt))
        rel = 2.0 ** -21 if prec == hip.PREC_F16 else 2.0 ** -19
        assert bool(((hi.float() + lo.float() - y32).abs() <= torch.maximum(rel * y32.abs(), torch.full_like(y32, 2.0 ** -24))).all())
        hi2 = torch.zeros_like(hi); lo2 = torch.zeros_like(lo)
        hip.layernorm(x, g1, b1, prec=prec, out_hi=hi2, out_lo=lo2)
        assert torch.equal(hi2, hi) and torch.equal(lo2, lo)
        with pytest.raises(hip.GavaError):
            hip.layernorm(x, g1, b1, prec=prec, out_hi=hi2)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,D", [(45000, 768), (300, 768), (20000, 1024)])
def test_ping_pong_loop_in_the_forward_forms_is_bit_identical(prec, M, D):
    """The forms the inference driver launches on the ping-pong loop - residual producers with the 16-bit copy and the
    pre-reduced row sums (out_proj: K = D, fc2: K = 4D), LayerNorm-folded consumers in partials and stats mode (qkv with the
    scaled columns, fc1 with QuickGELU), the weight-lo pass (w_lo = 1) - against the default loop on the same inputs: every
    output bit for bit (same k order, same epilogue code), ragged last tile, several tiles per workgroup."""
    d = dev()
    dt = hip.h16_dtype(prec)
    Mp = (M + 255) // 256 * 256
    for K in (D, 4 * D):
        A = rnd((M, K), 1.0, 1).to(d).to(dt)
        W = rnd((D, K), K ** -0.5, 2).to(d).to(dt)
        b = rnd((D,), 0.3, 3).to(d)
        X0 = (rnd((M, D), 1.0, 4) + 0.5).to(d)
        res = []
        for kern in (hip.KERNEL_256, hip.KERNEL_PP):
            X = X0.clone()
            x16 = torch.zeros(Mp, D, dtype=dt, device=d)
            part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
            hip.gemm(A, W, b, X, epilogue=hip.EPI_F32, prec=prec, resid=X, x16_out=x16, rowsum_out=part, rowsum_reduced=True, kernel=kern)
            Y = torch.zeros(M, D, device=d)
            hip.gemm(A, W, b, Y, epilogue=hip.EPI_F32, prec=prec, resid=X0, kernel=kern)      # out of place, no producer extras
            res.append((X, x16, part[:M, :D // 256].clone(), Y))
        for a_, b_ in zip(*res):
            assert torch.equal(a_, b_), K
        assert torch.allclose(res[1][0], X0 + A.float() @ W.float().t() + b, rtol=1e-4, atol=1e-4)
    X, x16, part_, _ = res[1]
    part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d); part[:M, :D // 256] = part_
    stats = torch.zeros(Mp, 2, device=d)
    stats[:M, 0], stats[:M, 1] = X.mean(1), (X.var(1, unbiased=False) + 1e-5).rsqrt()
    gamma = (1 + rnd((D,), 0.2, 5)).to(d)
    for N, epi in ((3 * D, hip.EPI_H16), (4 * D, hip.EPI_H16_QGELU)):
        Wf = (rnd((N, D), D ** -0.5, 7).to(d) * gamma).to(dt)
        fs, ft = Wf.float().sum(1).contiguous(), rnd((N,), 0.3, 8).to(d)
        kw = dict(scale_cols=N // 3, scale=0.125) if epi == hip.EPI_H16 else {}
        for mode in (dict(fold_partials=part), dict(fold_stats=stats)):
            outs = []
            for kern in (hip.KERNEL_256, hip.KERNEL_PP):
                o = torch.zeros(M, N, dtype=dt, device=d)
                hip.gemm(x16[:M], Wf, None, o, epilogue=epi, prec=prec, fold_s=fs, fold_t=ft, kernel=kern, **mode, **kw)
                outs.append(o)
            assert torch.equal(outs[0], outs[1]), (N, list(mode))
        # weight-lo pass on the ping-pong loop
        lo = (rnd((N, D), D ** -0.5, 7).to(d) * gamma - Wf.float()).to(dt)
        Wp = torch.cat([Wf, lo], 1).contiguous()
        outs = []
        for kern in (hip.KERNEL_256, hip.KERNEL_PP):
            o = torch.zeros(M, N, dtype=dt, device=d)
            hip.gemm(x16[:M], Wp, None, o, epilogue=epi, prec=prec, fold_partials=part, fold_s=fs, fold_t=ft, w_lo=1, kernel=kern, **kw)
            outs.append(o)
        assert torch.equal(outs[0], outs[1])


def test_ping_pong_loop_race_screen_under_load():
    """A new synchronisation structure is screened, not trusted after one clean run (cdna_hip_programming.md: an early read of a
    staged buffer passes whenever the DMA happens to land first): 40 rounds over several row counts and depths - ragged and
    full tiles, one and many tiles per workgroup, K = 256 (the shortest pipeline: prologue and tile switch back to back) to
    3072 - while a second stream streams 256 MB through HBM to perturb every latency; every output compared bit for bit with
    the default loop's."""
    d = dev()
    prec, dt = hip.PREC_F16, torch.float16
    shapes = [(70000, 768, 768), (45000, 768, 3072), (257, 256, 256), (66000, 512, 256), (30000, 1024, 1024)]
    noise_a = torch.empty(64 * 2 ** 20, device=d)
    noise_b = torch.empty_like(noise_a)
    side = torch.cuda.Stream()
    cases = []
    for (M, N, K) in shapes:
        A = rnd((M, K), 1.0, M % 97).to(d).to(dt)
        W = rnd((N, K), K ** -0.5, 2).to(d).to(dt)
        X0 = rnd((M, N), 1.0, 4).to(d)
        ref = X0.clone()
        hip.gemm(A, W, None, ref, epilogue=hip.EPI_F32, prec=prec, resid=ref, kernel=hip.KERNEL_256)
        cases.append((A, W, X0, ref))
    torch.cuda.synchronize()
    for it in range(40):
        with torch.cuda.stream(side):
            noise_b.copy_(noise_a)
            noise_a.copy_(noise_b)
        A, W, X0, ref = cases[it % len(cases)]
        X = X0.clone()
        hip.gemm(A, W, None, X, epilogue=hip.EPI_F32, prec=prec, resid=X, kernel=hip.KERNEL_PP)
        assert torch.equal(X, ref), (it, tuple(A.shape))
    torch.cuda.synchronize()
