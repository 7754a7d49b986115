"""GPU: the kernel forms that only the training path runs, op by op against float64 references.

Every reference is computed in float64 from the exact 16-bit operands the kernel receives, so what is left is the
kernel's own rounding: one output rounding (eps16 = 2^-11 fp16, 2^-8 bf16) and the fp32 accumulation, bounded by
2^-18 of |A|.|W|^T (64 fp32 units of the largest possible partial sum).  Operands are asymmetric and non-identity: a
symmetric operand hides a transposed fragment map.

Covered: the QuickGELU'-fused dgrad epilogue (EPI_H16_QGELU_BWD) with kept fp16 or bf16 pre-activations, the training
forward's pre-activation copy (aux_out) on every kernel that stores it, the fp32 dgrad GEMMs without a residual on the
persistent kernel and on sliced operands, the summary-attention weight gradient (training._wgrad), the LayerNorm
backward's 16-bit dx copy / aliasing / partial float4 lanes / many-row dgamma, and the activations the training
forwards keep for the backward (gava_vision_forward_keep, gava_vision_forward_train, gava_text_forward_train), each
slot recomputed one stage deep from the kept input of its stage.  Worst ratios to the bounds are printed ("RATIO ...").
A 16-bit output whose error is its own rounding sits near 1 at its worst element by construction: eps16 is the largest
relative error of one round-to-nearest (a value just above a power of two)."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import VitaCLIP, hip, synth, training  # noqa: E402
from gava_clip_amd.config import TINY, VIT_B16_T8  # noqa: E402
from oracle.vita_oracle import Oracle  # noqa: E402  (checker only)
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

PRECS = [hip.PREC_F16, hip.PREC_BF16]
EPS16 = {hip.PREC_F16: 2 ** -11, hip.PREC_BF16: 2 ** -8}
ACC = 2 ** -18          # fp32 accumulation, relative to |A|.|W|^T
F64 = torch.float64


def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def rnd(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale)


def ratio(name, got, ref, bound):
    """max |got - ref| / bound over the elements (<= 1 passes); printed so that a run records the margins."""
    r = float(((got.double() - ref.double()).abs() / bound).max())
    print(f"RATIO {name}: {r:.3f}")
    return r


def row_ratio(name, got, ref, rel):
    """row-wise ||got - ref|| / (rel * ||ref||), the worst row."""
    g, r = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    v = float(((g - r).norm(dim=1) / (rel * r.norm(dim=1))).max())
    print(f"RATIO {name}: {v:.3f}")
    return v


def rnd_dev(shape, scale=1.0, seed=0):
    """rnd for the big operands, drawn on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda") * scale


def qgelu_grad64(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


def aux_values(M, N, seed):
    """Pre-activations that cover the sign change of qgelu' (x ~ -0.7514), both saturation ends (|x| ~ 12) and exact zeros."""
    a = rnd((M, N), 2.0, seed) + 0.3
    f = a.view(-1)
    f[::5] = torch.linspace(-13.0, 13.0, f[::5].numel())
    f[1::17] = torch.linspace(-0.8, -0.7, f[1::17].numel())
    f[2::13] = 0.0
    return a


# =====================================================================================================================
# A. backward GEMM forms
# =====================================================================================================================

QGELU_BWD_SHAPES = [(231, 2048, 512, hip.KERNEL_AUTO),       # text c_proj^T: 128^2 kernel
                    (16, 3072, 768, hip.KERNEL_AUTO),        # CLS rows of the CLS-only last block: 128^2 kernel
                    (231, 2048, 512, hip.KERNEL_256),        # the persistent kernel named at small M
                    (3152, 3072, 768, hip.KERNEL_AUTO),      # persistent 256^2 kernel
                    (25217, 3072, 768, hip.KERNEL_AUTO)]     # ragged M, several tiles per workgroup


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("aux_prec", PRECS)
@pytest.mark.parametrize("M,N,K,kern", QGELU_BWD_SHAPES)
def test_gemm_qgelu_backward_epilogue(prec, aux_prec, M, N, K, kern):
    """out = (A . W^T) * qgelu'(aux), aux kept in its own 16-bit type (fp16 activations of the forward under bf16
    gradients take the aux_f16 decode); ldo > N with aux sharing it; rows beyond M and columns beyond N untouched."""
    d = dev()
    dt, at = hip.h16_dtype(prec), hip.h16_dtype(aux_prec)
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = (rnd((N, K), K ** -0.5, 2) + 0.01).to(d).to(dt)
    ldo, Mp = N + 64, M + 40
    aux = torch.zeros(Mp, ldo, dtype=at, device=d)
    aux[:M, :N] = aux_values(M, N, 3).to(d).to(at)
    out = torch.full((Mp, ldo), 3.0, dtype=dt, device=d)
    hip.gemm(A, W, None, out[:M, :N], epilogue=hip.EPI_H16_QGELU_BWD, prec=prec, aux=aux[:M], aux_prec=aux_prec, kernel=kern)
    torch.cuda.synchronize()
    acc = A.to(F64) @ W.to(F64).t()
    ref = acc * qgelu_grad64(aux[:M, :N].to(F64))
    bound = EPS16[prec] * ref.abs() + ACC * (A.to(F64).abs() @ W.to(F64).abs().t())
    assert ratio(f"qgelu_bwd {M}x{N}x{K} k{kern} p{prec} a{aux_prec}", out[:M, :N], ref, bound) <= 1
    assert bool((out[M:] == 3.0).all()) and bool((out[:M, N:] == 3.0).all())


def test_gemm_qgelu_backward_rejects():
    d = dev()
    prec, dt = hip.PREC_BF16, torch.bfloat16
    M, N, K = 300, 256, 128
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = rnd((N, K), 0.1, 2).to(d).to(dt)
    flat = torch.zeros(M * N + 8, dtype=dt, device=d)
    aux, aux_mis = flat[:M * N].view(M, N), flat[1:1 + M * N].view(M, N)
    out = torch.zeros(M, N, dtype=dt, device=d)
    kw = dict(epilogue=hip.EPI_H16_QGELU_BWD, prec=prec)
    hip.gemm(A, W, None, out, aux=aux, **kw)                 # the valid call
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, out, aux=None, **kw)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, out, aux=aux_mis, **kw)         # 2-byte misaligned
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, out, aux=aux, aux_prec=2, **kw)
    W2 = rnd((N, 2 * K), 0.1, 2).to(d).to(dt)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W2, None, out, aux=aux, w_lo=1, K=K, **kw)
    wide = torch.zeros(M, N + 4, dtype=dt, device=d)          # ldo % 8 != 0 (aux shares ldo)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, wide[:, :N], aux=torch.zeros(M, N + 4, dtype=dt, device=d)[:, :N], **kw)


def _fold_operands(M, D, prec, seed=0):
    """x16 / row-sum partials / (mean, rstd) of a residual stream, as in test_ping_pong_loop_in_the_forward_forms_is_bit_identical."""
    d = dev()
    dt = hip.h16_dtype(prec)
    Mp = (M + 255) // 256 * 256
    K = D
    A = rnd((M, K), 1.0, 1 + seed).to(d).to(dt)
    W = rnd((D, K), K ** -0.5, 2 + seed).to(d).to(dt)
    b = rnd((D,), 0.3, 3).to(d)
    X = (rnd((M, D), 1.0, 4) + 0.5).to(d)
    x16 = torch.zeros(Mp, D, dtype=dt, device=d)
    part = torch.zeros(Mp + 32, 4, 2, dtype=torch.float32, device=d)
    hip.gemm(A, W, b, X, epilogue=hip.EPI_F32, prec=prec, resid=X, x16_out=x16, rowsum_out=part, rowsum_reduced=True)
    stats = torch.zeros(Mp, 2, device=d)
    stats[:M, 0], stats[:M, 1] = X.mean(1), (X.var(1, unbiased=False) + 1e-5).rsqrt()
    return x16[:M], part, stats


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", ["128", "256", "fold_stats", "fold_partials"])
def test_gemm_qgelu_pre_activation_copy(prec, form):
    """aux_out (the training forward keeps fc1's pre-activation): the QuickGELU output is bit-identical to the launch
    without aux_out, the copy bit-identical to EPI_H16 (scale_cols = 0) on the same operands and fold, and the rows
    behind a ragged M stay untouched.  Forms: 128^2 kernel, plain persistent kernel, LayerNorm-folded persistent kernel
    in stats and in partials mode (c2 training: R >= 8192)."""
    d = dev()
    dt = hip.h16_dtype(prec)
    D = 768
    N = 4 * D
    M = 300 if form == "128" else (3000 if form == "256" else 20000)
    kern = hip.KERNEL_AUTO if form == "128" else hip.KERNEL_256
    W = (rnd((N, D), D ** -0.5, 7) + 0.005).to(d).to(dt)
    if form.startswith("fold"):
        A, part, stats = _fold_operands(M, D, prec)
        fs, ft = W.float().sum(1).contiguous(), rnd((N,), 0.3, 8).to(d)
        kw = dict(fold_s=fs, fold_t=ft, **(dict(fold_stats=stats) if form == "fold_stats" else dict(fold_partials=part)))
        bias = None
    else:
        A = rnd((M, D), 1.0, 1).to(d).to(dt)
        bias, kw = rnd((N,), 0.5, 3).to(d), {}
    Mp = M + 200
    plain = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, bias, plain, epilogue=hip.EPI_H16_QGELU, prec=prec, kernel=kern, **kw)
    out = torch.zeros(M, N, dtype=dt, device=d)
    pre = torch.full((Mp, N), -5.0, dtype=dt, device=d)
    hip.gemm(A, W, bias, out, epilogue=hip.EPI_H16_QGELU, prec=prec, kernel=kern, aux_out=pre, **kw)
    lin = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, bias, lin, epilogue=hip.EPI_H16, prec=prec, kernel=kern, scale_cols=0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    assert torch.equal(pre[:M], lin)
    assert bool((pre[M:] == -5.0).all())
    assert float(lin.float().abs().max()) > 0.5


def test_gemm_pre_activation_copy_rejects():
    d = dev()
    prec, dt = hip.PREC_F16, torch.float16
    M, N, K = 3000, 1024, 256
    A = rnd((M, K), 1.0, 1).to(d).to(dt)
    W = rnd((N, K), 0.1, 2).to(d).to(dt)
    pre = torch.zeros(M, N, dtype=dt, device=d)
    hip.gemm(A, W, None, torch.zeros(M, N, dtype=dt, device=d), epilogue=hip.EPI_H16_QGELU, prec=prec, aux_out=pre)   # valid
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, torch.zeros(M, 3 * N, dtype=dt, device=d), epilogue=hip.EPI_H16_QGELU, prec=prec, aux_out=pre, split_out=True)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, torch.zeros(M, N, dtype=dt, device=d), epilogue=hip.EPI_H16, prec=prec, aux_out=pre)
    with pytest.raises(hip.GavaError):
        hip.gemm(A, W, None, torch.zeros(M, N, dtype=dt, device=d), epilogue=hip.EPI_H16_QGELU, prec=prec, aux_out=pre,
                 kernel=hip.KERNEL_PP)


# c2 training rows (64 clips x 8 frames x 197 tokens) and c5-like ViT-L/14 rows: AUTO takes the persistent kernel
DGRAD_SHAPES = [(64 * 8 * 197, 768, 3072), (64 * 8 * 197, 768, 2304), (4 * 32 * 257, 1024, 4096)]


@pytest.mark.parametrize("M,N,K", DGRAD_SHAPES)
def test_dgrad_gemm_fp32_without_residual(M, N, K):
    """The dgrad GEMMs of the backward (EPI_F32, no residual) on the persistent kernel's aligned walk: AUTO, KERNEL_256
    and KERNEL_PP bit for bit, and the fp64 reference within the fp32 accumulation bound."""
    d = dev()
    prec, dt = hip.PREC_BF16, torch.bfloat16
    assert hip.load().gava_gemm_aligned_walk(M, N, 0) == 1
    A = (rnd_dev((M, K), 0.02, 11) + 0.001).to(dt)
    W = (rnd_dev((N, K), K ** -0.5, 12) + 0.002).to(dt)
    outs = []
    for kern in (hip.KERNEL_AUTO, hip.KERNEL_256, hip.KERNEL_PP):
        o = torch.full((M, N), float("nan"), device=d)
        hip.gemm(A, W, None, o, epilogue=hip.EPI_F32, prec=prec, kernel=kern)
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    A64, W64 = A.to(F64), W.to(F64)
    ref = A64 @ W64.t()
    bound = ACC * (A64.abs() @ W64.abs().t())
    assert ratio(f"dgrad {M}x{N}x{K}", outs[0], ref, bound) <= 1


@pytest.mark.parametrize("M", [3152, 231])
def test_dgrad_gemm_fp32_plain_walk_and_small_m(M):
    """The same epilogue on the persistent kernel's plain walk (few tiles) and, for the text tower's row count, the 128^2
    kernel: text c_fc^T (231, 512, 2048) and in_proj^T (231, 512, 1536)."""
    d = dev()
    prec, dt = hip.PREC_BF16, torch.bfloat16
    shapes = [(768, 3072)] if M > 2048 else [(512, 2048), (512, 1536)]
    for N, K in shapes:
        A = (rnd((M, K), 0.02, 13) + 0.001).to(d).to(dt)
        W = (rnd((N, K), K ** -0.5, 14) + 0.002).to(d).to(dt)
        kerns = (hip.KERNEL_256, hip.KERNEL_PP) if M > 2048 else (hip.KERNEL_AUTO,)
        if M > 2048:
            assert hip.load().gava_gemm_aligned_walk(M, N, 0) == 0
        outs = []
        for kern in kerns:
            o = torch.full((M, N), float("nan"), device=d)
            hip.gemm(A, W, None, o, epilogue=hip.EPI_F32, prec=prec, kernel=kern)
            outs.append(o)
        assert all(torch.equal(outs[0], o) for o in outs)
        A64, W64 = A.to(F64), W.to(F64)
        assert ratio(f"dgrad {M}x{N}x{K}", outs[0], A64 @ W64.t(), ACC * (A64.abs() @ W64.abs().t())) <= 1


def test_dgrad_gemm_on_sliced_operands():
    """The CLS-only last block's dgrad (training.vision_backward): [dK dV] . [Wk; Wv] with A = dqkv[:, D:] (lda = 3D,
    K = 2D), and + dQ . Wq with W = w_qkv_t[:, :D] (ldw = 3D) into the CLS rows of dxn (ldo = n1*D) aliasing the residual;
    no other row of dxn changes."""
    d = dev()
    prec, dt = hip.PREC_BF16, torch.bfloat16
    BT, n1, D = 48, 197, 768
    R = BT * n1
    dqkv = (rnd((R, 3 * D), 0.01, 21) + 0.0005).to(d).to(dt)
    w_qkv_t = (rnd((D, 3 * D), D ** -0.5, 22) + 0.001).to(d).to(dt)
    w_kv_t = w_qkv_t[:, D:].contiguous()
    dxn = torch.full((R, D), float("nan"), device=d)
    hip.gemm(dqkv[:, D:], w_kv_t, None, dxn, epilogue=hip.EPI_F32, prec=prec)
    A64, W64 = dqkv[:, D:].to(F64), w_kv_t.to(F64)
    assert ratio("dgrad sliced A", dxn, A64 @ W64.t(), ACC * (A64.abs() @ W64.abs().t())) <= 1
    before = dxn.clone()
    dq = (rnd((BT, D), 0.01, 23) - 0.0003).to(d).to(dt)
    cls = dxn.view(BT, n1 * D)[:, :D]
    hip.gemm(dq, w_qkv_t[:, :D], None, cls, epilogue=hip.EPI_F32, prec=prec, resid=cls)
    torch.cuda.synchronize()
    Wq = w_qkv_t[:, :D].to(F64)
    b_cls = before.view(BT, n1, D)[:, 0].to(F64)
    ref = b_cls + dq.to(F64) @ Wq.t()
    bound = ACC * (dq.to(F64).abs() @ Wq.abs().t()) + 2 ** -23 * ref.abs()
    assert ratio("dgrad sliced W, aliased residual", dxn.view(BT, n1, D)[:, 0], ref, bound) <= 1
    assert torch.equal(dxn.view(BT, n1, D)[:, 1:], before.view(BT, n1, D)[:, 1:])


@pytest.mark.parametrize("rows", [1, 8, 13, 70, 512])
def test_wgrad_against_fp64(rows):
    """training._wgrad (summary attention weight gradients, reduction over B*T rows zero-padded to 64): fp64 dy^T . x;
    the padding contributes nothing (it is built from zeros, and a non-zero pad would show as an error here)."""
    d = dev()
    D = 768
    dy = (rnd((rows, 3 * D), 0.05, 31) + 0.01).to(d).to(torch.bfloat16)
    x = (rnd((rows, D), 1.0, 32) - 0.2).to(d).to(torch.bfloat16)
    A = training._pad_k(dy.t())
    assert A.shape[1] % 64 == 0 and bool((A[:, rows:] == 0).all())
    got = training._wgrad(dy, x)
    torch.cuda.synchronize()
    dy64, x64 = dy.to(F64), x.to(F64)
    ref = dy64.t() @ x64
    assert got.shape == (3 * D, D)
    assert ratio(f"wgrad rows={rows}", got, ref, ACC * (dy64.abs().t() @ x64.abs()) + 2 ** -23 * ref.abs()) <= 1


# =====================================================================================================================
# B. LayerNorm backward
# =====================================================================================================================

def _ln_bwd_ref(x, gamma, dy):
    x, gamma, dy = x.to(F64), gamma.to(F64), dy.to(F64)
    mu = x.mean(1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(1, keepdim=True) + 1e-5).rsqrt()
    xh = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_layernorm_backward_dx16_copy(prec, accumulate):
    """dx16 (the A operand of the next dgrad) is exactly h16 of the FINAL dx (after the accumulate), with padded strides."""
    d = dev()
    rows, D = 777, 768
    x = (rnd((rows, D + 12), 1.5, 41) + 0.4).to(d)[:, :D]
    dy = rnd((rows, D + 4), 1.0, 42).to(d)[:, :D]
    gamma = (1 + rnd((D,), 0.3, 43)).to(d)
    base = rnd((rows, D + 8), 2.0, 44).to(d)
    dx = base.clone()[:, :D] if accumulate else torch.full((rows, D + 8), 9.0, device=d)[:, :D]
    dx16 = torch.full((rows, D + 16), 5.0, dtype=hip.h16_dtype(prec), device=d)
    hip.layernorm_backward(x, gamma, dy, dx, accumulate=accumulate, dx16=dx16[:, :D], prec=prec)
    torch.cuda.synchronize()
    assert torch.equal(dx16[:, :D], dx.to(hip.h16_dtype(prec)))
    assert bool((dx16[:, D:] == 5.0).all())
    ref, _, _ = _ln_bwd_ref(x, gamma, dy)
    if accumulate:
        ref = ref + base[:, :D].to(F64)
    assert float((dx.to(F64) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_layernorm_backward_dy_aliasing_dx():
    """training.py: ln_pre' runs with dy == dx (no accumulate) - bit-identical to the out-of-place call."""
    d = dev()
    rows, D = 1001, 768
    x = (rnd((rows, D), 1.0, 51) - 0.3).to(d)
    dy = rnd((rows, D), 1.0, 52).to(d)
    gamma = (1 + rnd((D,), 0.3, 53)).to(d)
    out = torch.empty_like(dy)
    hip.layernorm_backward(x, gamma, dy, out)
    inplace = dy.clone()
    hip.layernorm_backward(x, gamma, inplace, inplace)
    torch.cuda.synchronize()
    assert torch.equal(out, inplace)


@pytest.mark.parametrize("D", [4, 260, 1020])
def test_layernorm_backward_partial_lanes(D):
    """D not a multiple of 256: the last float4 group of the wave is partly active."""
    d = dev()
    rows = 37
    x = (rnd((rows, D), 1.0, 61) + 0.2).to(d)
    dy = (rnd((rows, D), 1.0, 62) - 0.1).to(d)
    gamma = (1 + rnd((D,), 0.3, 63)).to(d)
    dx = torch.full((rows, D), float("nan"), device=d)
    dg, db = torch.zeros(D, device=d), torch.zeros(D, device=d)
    dx16 = torch.zeros(rows, D, dtype=torch.bfloat16, device=d)
    hip.layernorm_backward(x, gamma, dy, dx, dgamma=dg, dbeta=db, dx16=dx16)
    torch.cuda.synchronize()
    rdx, rdg, rdb = _ln_bwd_ref(x, gamma, dy)
    assert float((dx.to(F64) - rdx).abs().max()) <= 1e-5 * float(rdx.abs().max())
    assert float((dg.to(F64) - rdg).abs().max()) <= 1e-5 * float(rdg.abs().max())
    assert float((db.to(F64) - rdb).abs().max()) <= 1e-5 * float(rdb.abs().max())
    assert torch.equal(dx16, dx.to(torch.bfloat16))


def test_layernorm_backward_many_row_dgamma_dbeta():
    """dgamma / dbeta over ~25k rows of D = 768 (the full-batch summary_ln / norm' pattern), accumulated into non-zero
    buffers.  Atomic fp32 sums of 25216 terms in any order: the rounding error of a sum whose partial sums grow like
    the result is about sqrt(n/3) u |sum| = 5e-6 |sum| (u = 2^-24); the dy / xhat correlation below makes every column's
    sum grow linearly, so the norm-wise bound 1e-5 holds with room."""
    d = dev()
    rows, D = 64 * 197 * 2, 768
    x = (rnd((rows, D), 1.0, 71) + rnd((1, D), 0.5, 72)).to(d)
    xh = (x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True)
    dy = (0.5 + 0.3 * xh + rnd((rows, D), 0.3, 73).to(d)).contiguous()
    gamma = (1 + rnd((D,), 0.3, 74)).to(d)
    g0, b0 = rnd((D,), 10.0, 75).to(d), rnd((D,), 10.0, 76).to(d)
    dg, db = g0.clone(), b0.clone()
    dx = torch.empty_like(x)
    hip.layernorm_backward(x, gamma, dy, dx, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    _, rdg, rdb = _ln_bwd_ref(x, gamma, dy)
    rdg, rdb = rdg + g0.to(F64), rdb + b0.to(F64)
    eg = float((dg.to(F64) - rdg).norm() / rdg.norm())
    eb = float((db.to(F64) - rdb).norm() / rdb.norm())
    print(f"RATIO ln_bwd dgamma 25k rows: {eg / 1e-5:.3f}")
    print(f"RATIO ln_bwd dbeta 25k rows: {eb / 1e-5:.3f}")
    assert eg <= 1e-5 and eb <= 1e-5


def test_layernorm_backward_rejects():
    d = dev()
    x = rnd((8, 1028), 1.0, 81).to(d)
    gamma = torch.ones(1028, device=d)
    with pytest.raises(hip.GavaError):
        hip.layernorm_backward(x, gamma, x.clone(), torch.zeros_like(x))                    # D > 1024
    x6 = rnd((8, 130), 1.0, 82).to(d)
    with pytest.raises(hip.GavaError):
        hip.layernorm_backward(x6, torch.ones(130, device=d), x6.clone(), torch.zeros_like(x6))   # D % 4
    x8 = rnd((8, 128), 1.0, 83).to(d)
    idx = torch.arange(8, dtype=torch.int32, device=d)
    with pytest.raises(hip.GavaError):
        hip.layernorm_backward(x8, torch.ones(128, device=d), x8.clone(), torch.zeros_like(x8), dx_row_index=idx,
                               dx16=torch.zeros(8, 128, dtype=torch.bfloat16, device=d))


# =====================================================================================================================
# C. kept and saved activations, one stage deep
# =====================================================================================================================

class Oracle64(Oracle):
    """The oracle's primitives in float64 (its LayerNorm casts to fp32)."""

    @staticmethod
    def layer_norm(x, w, b):
        return torch.nn.functional.layer_norm(x.to(F64), (x.shape[-1],), w.to(F64), b.to(F64), 1e-5)


def ln_mag(x, g, b):
    """fp64 LayerNorm of the rows of x and the operand magnitude its consumer GEMM sees: rstd (|x| + |mean|) |gamma| + |beta|
    bounds both the normalised row (unfolded form) and the folded form's rstd |x16| |gamma W| + rstd |mean| |gamma W|."""
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    y = (x - mu) * rstd * g.to(F64) + b.to(F64)
    return y, rstd * (x.abs() + mu.abs()) * g.to(F64).abs() + b.to(F64).abs()


def gemm_check(name, got, a, mag, W, b, eps, scale_cols=0, scale=1.0):
    """single-GEMM slot: |got - ref| <= eps |ref| + 2 eps (|a| . |W|^T), ref = a W^T + b (first scale_cols columns x scale)."""
    W = W.to(F64)
    ref = a @ W.t() + (b.to(F64) if b is not None else 0)
    prod = mag @ W.abs().t()
    if scale_cols:
        ref[:, :scale_cols] *= scale
        prod[:, :scale_cols] *= scale
    return ratio(name, got, ref, eps * ref.abs() + 2 * eps * prod + 1e-30)


def attn64(q, k, v, heads):
    """softmax(q k^T) v per head; q already scaled.  q (N, Lq, D), k / v (N, Lk, D)."""
    N, Lq, D = q.shape
    dh = D // heads
    qh = q.view(N, Lq, heads, dh).transpose(1, 2)
    kh = k.view(N, -1, heads, dh).transpose(1, 2)
    vh = v.view(N, -1, heads, dh).transpose(1, 2)
    p = (qh @ kh.transpose(-1, -2)).softmax(-1)
    return (p @ vh).transpose(1, 2).reshape(N, Lq, D)


def _make(cfg, B, seed=0):
    d = dev()
    sd = synth_torch_state(cfg, 3, seed)
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3), operand_dtype="fp16")
    m.load_state_dict(sd, strict=True)
    m = m.to(d).train()
    m._attach_encoders()
    m._pack()
    x = torch.from_numpy(synth.synth_clip(B, cfg.num_frames, cfg.input_size, seed=seed + 5)).to(d)
    p64 = {k: v.to(d).to(F64) for k, v in sd.items()}
    return m, sd, p64, x


CAN = 4096      # canary elements behind every kept buffer (inside its allocation)


def _padded_kept(m, B, T, d, last=True):
    """training.alloc_kept's shapes, each buffer NaN-filled (an unwritten element fails its check) and followed by a canary."""
    ref = training.alloc_kept(m, B, T, d)
    if not last:
        NL = m._shape["layers"]
        ref["x1"] = torch.empty(NL, *ref["x1"].shape[1:], device=d)
        ref["pre"] = torch.empty(NL, *ref["pre"].shape[1:], dtype=ref["pre"].dtype, device=d)
        for k in ("last_q", "last_x1", "last_pre"):
            del ref[k]
    kept, flat = {}, {}
    for k, t in ref.items():
        buf = torch.empty(t.numel() + CAN, dtype=t.dtype, device=d)
        buf.fill_(float("nan"))
        buf[t.numel():] = -7.0
        flat[k] = buf
        kept[k] = buf[:t.numel()].view(t.shape)
    return kept, flat


def _check_canaries(kept, flat):
    for k, buf in flat.items():
        n = kept[k].numel()
        assert bool((buf[n:] == -7.0).all()), f"kept[{k!r}]: the driver wrote behind the buffer"


def _check_kept(cfg, B, last=True):
    d = dev()
    m, sd, p, x = _make(cfg, B)
    sh = m._shape
    T, D, H, G, NL, F = cfg.num_frames, sh["D"], sh["H"], sh["G"], sh["layers"], sh["F"]
    n1 = (sh["size"] // sh["P"]) ** 2 + 1
    BT = B * T
    R, Bm = BT * n1, BT // T
    eps = EPS16[m.prec]
    kept, flat = _padded_kept(m, B, T, d, last)
    if last:
        # the slot count of the header (gava_vision_saved: x1 / pre have no slot for the CLS-only last block)
        assert kept["x1"].shape[0] == max(NL - 1, 1) and kept["pre"].shape[0] == max(NL - 1, 1)
    with torch.no_grad():
        cls_x, summary = m.encode_video(x, kept=kept)
    torch.cuda.synchronize()
    _check_canaries(kept, flat)
    assert bool(torch.isfinite(cls_x).all()) and bool(torch.isfinite(summary).all())
    o = Oracle64(cfg, p, torch.cat(m.tokenized_prompts))
    tag = f"{'vitb3' if D == 768 else 'tiny'} B={B}{'' if last else ' no-last'}"
    worst = {}

    def note(slot, r):
        worst[slot] = max(worst.get(slot, 0.0), r)

    # ---- e0 (patch embedding + cls / pos / time) and x[0] = ln_pre(e0)
    xf = x.permute(0, 2, 1, 3, 4).flatten(0, 1).to(F64)
    P_, g = cfg.patch_size, cfg.grid
    cols = xf.view(BT, 3, g, P_, g, P_).permute(0, 2, 4, 1, 3, 5).reshape(BT, g * g, 3 * P_ * P_)
    wp = p["visual.patch_embed.proj.weight"].reshape(D, -1)
    pe = cols @ wp.t() + p["visual.patch_embed.proj.bias"]
    e0 = torch.cat([p["visual.cls_token"].view(1, 1, D).expand(BT, 1, D), pe], 1) + p["visual.pos_embed"]
    e0 = (e0.view(B, T, n1, D) + o.time_embed(T).view(1, T, 1, D)).view(BT, n1, D)
    prod = torch.cat([torch.zeros(BT, 1, D, device=d, dtype=F64), cols.abs() @ wp.abs().t()], 1)
    # (+ the fp32 additions of cls token, bias, position and time embedding)
    prod = prod + ACC / (2 * eps) * (p["visual.cls_token"].abs() + p["visual.patch_embed.proj.bias"].abs() + p["visual.pos_embed"].abs()
                                     + o.time_embed(T).abs().view(1, T, 1, D)).expand(B, T, n1, D).reshape(BT, n1, D)
    note("e0", ratio(f"{tag} e0", kept["e0"].view(BT, n1, D), e0, eps * e0.abs() + 2 * eps * prod + 1e-30))
    x0, mag0 = ln_mag(kept["e0"], p["visual.ln_pre.weight"], p["visual.ln_pre.bias"])
    note("x[0]", ratio(f"{tag} x[0]", kept["x"][0], x0, ACC * mag0))
    for i in range(NL):
        pre_ = f"visual.blocks.{i}."
        w = lambda n: p[pre_ + n]
        Wqkv = torch.cat([w("attn.q_proj.weight"), w("attn.k_proj.weight"), w("attn.v_proj.weight")], 0)
        bqkv = torch.cat([w("attn.q_proj.bias"), w("attn.k_proj.bias"), w("attn.v_proj.bias")], 0)
        Xin = kept["x"][i]
        last_blk = last and i == NL - 1
        # ---- qkv[i] (the last block: K/V columns for every row, the CLS queries in last_q)
        a, mag = ln_mag(Xin, w("norm1.weight"), w("norm1.bias"))
        if last_blk:
            note("qkv", gemm_check(f"{tag} qkv[{i}] kv", kept["qkv"][i][:, D:], a, mag, Wqkv[D:], bqkv[D:], eps))
            ac, magc = a.view(BT, n1, D)[:, 0], mag.view(BT, n1, D)[:, 0]
            note("last_q", gemm_check(f"{tag} last_q", kept["last_q"], ac, magc, Wqkv[:D], bqkv[:D], eps, D, 0.125))
        else:
            note("qkv", gemm_check(f"{tag} qkv[{i}]", kept["qkv"][i], a, mag, Wqkv, bqkv, eps, D, 0.125))
        # ---- sidekv[i]: the prompt rows [global | CP + local | summary] through norm1 and the K/V GEMM.  CP and the
        #      summary token are recomputed with the forward's own kernels from the kept stream (the driver does not keep
        #      them), the LayerNorm + GEMM of the slot in fp64
        h = lambda t: hip.convert_h16(t.float().contiguous(), m.prec)
        cls16 = h(Xin.view(BT, n1, D)[:, 0])
        CP = torch.empty(BT, D, device=d)
        hip.gemm(cls16, h(w("cls_proj.weight")), w("cls_proj.bias").float().contiguous(), CP, epilogue=hip.EPI_F32, prec=m.prec)
        CPn = torch.empty(BT, D, dtype=hip.h16_dtype(m.prec), device=d)
        hip.layernorm(CP, w("summary_ln.weight").float().contiguous(), w("summary_ln.bias").float().contiguous(), out16=CPn, prec=m.prec)
        sa = "summary_attn_layer."
        Ws = torch.cat([w(sa + "q_proj.weight"), w(sa + "k_proj.weight"), w(sa + "v_proj.weight")], 0)
        bs = torch.cat([w(sa + "q_proj.bias"), w(sa + "k_proj.bias"), w(sa + "v_proj.bias")], 0)
        SQKV = torch.empty(BT, 3 * D, dtype=hip.h16_dtype(m.prec), device=d)
        hip.gemm(CPn, h(Ws), bs.float().contiguous(), SQKV, epilogue=hip.EPI_H16, prec=m.prec, scale_cols=D, scale=0.125)
        SMIX = torch.empty(BT, D, dtype=hip.h16_dtype(m.prec), device=d)
        hip.attention(SQKV[:, :D], SQKV[:, D:2 * D], SQKV[:, 2 * D:], SMIX, batch=Bm, heads=H, n_q=T, n_kmain=T, prec=m.prec)
        SUMM = torch.empty(BT, D, device=d)
        hip.gemm(SMIX, h(w(sa + "out_proj.weight")), w(sa + "out_proj.bias").float().contiguous(), SUMM, epilogue=hip.EPI_F32,
                 prec=m.prec, resid=CP)
        SIDE = torch.cat([p["visual.global_prompts"][i], (CP.to(F64).view(Bm, T, D) + w("local_prompts")[0]).view(BT, D),
                          SUMM.to(F64)], 0)
        a_s, mag_s = ln_mag(SIDE, w("norm1.weight"), w("norm1.bias"))
        note("sidekv", gemm_check(f"{tag} sidekv[{i}]", kept["sidekv"][i], a_s, mag_s, Wqkv[D:], bqkv[D:], eps))
        # ---- attention branch x1 - x, from the kept q / k / v and prompt K/V (fp64 attention + out_proj)
        qkv = kept["qkv"][i].to(F64).view(BT, n1, 3 * D)
        skv = kept["sidekv"][i].to(F64)
        fr = torch.arange(BT, device=d)
        sidx = torch.cat([torch.arange(G, device=d).expand(BT, G), G + (fr // T * T).view(BT, 1) + torch.arange(T, device=d),
                          (G + BT + fr).view(BT, 1)], 1)
        keys = torch.cat([qkv[:, :, D:2 * D], skv[sidx, :D]], 1)
        vals = torch.cat([qkv[:, :, 2 * D:], skv[sidx, D:]], 1)
        q = kept["last_q"].to(F64).view(BT, 1, D) if last_blk else qkv[:, :, :D]
        br = attn64(q, keys, vals, H) @ w("attn.out_proj.weight").t() + w("attn.out_proj.bias")
        if last_blk:
            X1 = kept["last_x1"]
            got = X1.to(F64) - Xin.view(BT, n1, D)[:, 0].to(F64)
        else:
            X1 = kept["x1"][i]
            got = (X1.to(F64) - Xin.to(F64)).view(BT, n1, D)
        note("attn branch", row_ratio(f"{tag} x1[{i}] - x[{i}]", got, br.view(got.shape), 8 * eps))
        # ---- pre[i] = fc1(norm2(x1)), and the MLP branch x[i+1] - x1 from the kept pre-activation
        a2, mag2 = ln_mag(X1, w("norm2.weight"), w("norm2.bias"))
        PRE = kept["last_pre"] if last_blk else kept["pre"][i]
        note("last_pre" if last_blk else "pre", gemm_check(f"{tag} {'last_pre' if last_blk else f'pre[{i}]'}", PRE, a2, mag2,
                                                           w("mlp.fc1.weight"), w("mlp.fc1.bias"), eps))
        brm = o.quick_gelu(PRE.to(F64)) @ w("mlp.fc2.weight").t() + w("mlp.fc2.bias")
        Xout = kept["x"][i + 1].view(BT, n1, D)[:, 0] if last_blk else kept["x"][i + 1]
        note("mlp branch", row_ratio(f"{tag} x[{i + 1}] - x1[{i}]", Xout.to(F64) - X1.to(F64), brm, 8 * eps))
    print(f"RATIO {tag} worst per slot: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1}
    assert not bad, bad
    return m, x, kept


@pytest.mark.parametrize("setup", ["vitb3", "tiny", "tiny_no_last"])
def test_vision_forward_keep_slots(setup):
    """gava_vision_forward_keep: every kept slot against its stage recomputed in fp64 from the kept input of that stage.
    vitb3: ViT-B/16 with 3 blocks, 6 clips x 8 frames = 9456 rows (the fused-partials fold path of c2 training); tiny: the
    stats fold path and the 128^2 kernels; tiny_no_last: without last_* (every block full-width, [layers] x1 / pre slots)."""
    if setup == "vitb3":
        _check_kept(dataclasses.replace(VIT_B16_T8, num_layers=3), 6)
    else:
        _check_kept(TINY, 2, last=setup == "tiny")


@pytest.mark.parametrize("setup", ["vitb3", "tiny"])
def test_vision_forward_train_saved_stream(setup):
    """gava_vision_forward_train's saved_x (embedding, block inputs, final stream) against the keep driver's e0 / x:
    the embedding and ln_pre run the same kernels in both (bit for bit); the blocks do not (the keep driver folds the
    LayerNorms), so x[i] agree within the branch bound of the blocks before, row-wise."""
    cfg, B = (dataclasses.replace(VIT_B16_T8, num_layers=3), 6) if setup == "vitb3" else (TINY, 2)
    d = dev()
    m, sd, p, x = _make(cfg, B)
    sh = m._shape
    T, D, NL = cfg.num_frames, sh["D"], sh["layers"]
    n1 = (sh["size"] // sh["P"]) ** 2 + 1
    BT, R = B * T, B * T * n1
    kept = training.alloc_kept(m, B, T, d)
    saved = torch.full((NL + 2 + 1, R, D), float("nan"), device=d)
    with torch.no_grad():
        m.encode_video(x, kept=kept)
        m.encode_video(x, saved=saved[:NL + 2])
    torch.cuda.synchronize()
    assert bool(torch.isnan(saved[NL + 2]).all()), "gava_vision_forward_train wrote behind saved_x"
    assert torch.equal(saved[0], kept["e0"]) and torch.equal(saved[1], kept["x"][0])
    eps = EPS16[m.prec]
    acc = torch.zeros(R, device=d, dtype=F64)
    for i in range(NL):
        X, X1 = kept["x"][i].to(F64), (kept["x1"][i] if i < NL - 1 else None)
        if i < NL - 1:
            acc = acc + (X1.to(F64) - X).norm(dim=1) + (kept["x"][i + 1].to(F64) - X1.to(F64)).norm(dim=1)
            got, ref, bound = saved[2 + i].to(F64), kept["x"][i + 1].to(F64), 8 * eps * acc
        else:   # final stream: the CLS rows (the keep driver's last block runs on them only)
            c = torch.arange(BT, device=d) * n1
            acc_c = acc[c] + (kept["last_x1"].to(F64) - X[c]).norm(dim=1) + (kept["x"][NL][c].to(F64) - kept["last_x1"].to(F64)).norm(dim=1)
            got, ref, bound = saved[NL + 1][c].to(F64), kept["x"][NL][c].to(F64), 8 * eps * acc_c
        r = float(((got - ref).norm(dim=1) / bound).max())
        print(f"RATIO {setup} saved_x[{i + 2}] vs keep x[{i + 1}]: {r:.3f}")
        assert r <= 1, i


def test_text_forward_train_saved_blocks():
    """gava_text_forward_train's saved_x: saved[i+1] against Oracle.text_block(i, saved[i]) in fp64 on the rows up to each
    prompt's EOT (causal: the rows behind it do not reach them), row-wise within 8 eps16 of the block's branch."""
    d = dev()
    cfg = TINY
    m, sd, p, x = _make(cfg, 1)
    ctx = m.prompt_learner.full_context()
    with torch.no_grad():
        out, saved = training.text_forward_train(m, ctx)
    torch.cuda.synchronize()
    n, L, W = m._pack()["tokens"].shape[0], m.text_rows_per_prompt, cfg.text_width
    tok = torch.cat(m.tokenized_prompts).to(d)
    eot = (tok == cfg.text_vocab_size - 1).nonzero()[:, 1]
    p_cpu = {k: v.to(F64) for k, v in sd.items()}
    o = Oracle64(cfg, p_cpu, tok.cpu())       # (the oracle builds its causal mask on the host)
    saved = saved.cpu()
    eps = EPS16[m.prec]
    worst = 0.0
    for i in range(cfg.text_layers):
        X = saved[i].view(n, L, W).to(F64)
        ref = o.text_block(i, X)
        got = saved[i + 1].view(n, L, W).to(F64)
        for c in range(n):
            e = int(eot[c]) + 1
            r = float(((got[c, :e] - ref[c, :e]).norm(dim=1) / (8 * eps * (ref[c, :e] - X[c, :e]).norm(dim=1))).max())
            worst = max(worst, r)
    print(f"RATIO text saved_x blocks: {worst:.3f}")
    assert worst <= 1
