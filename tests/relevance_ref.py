"""Reference side of the relevance-map tests (test_relevance_host.py, test_gpu_relevance.py); nothing here touches a GPU.
Cases, score regimes and the prompt-row gather come from attention_ref.py.

  * fp64 reference of gava_attention_relevance on the 16-bit operands, with the conversion of V the kernel applies and with
    the MUTATIONS that apply to it;
  * the relevance chain two ways: the vector chain the device runs and the matrix product it stands for;
  * a torch emulation of the kernel's rounding points in fp32, in the kernel's own summation order;
  * the bound, the forms, the kinds of dout and the shape table of the GPU test.

What is computed, per (frame, head):   out[j] = sum_i w_i max(0, P[i][j] G[i][j]),   j over the frame's own n keys,
    P = softmax_j(q_i . k_j) over ALL keys (prompt rows included, no renormalisation),   G[i][j] = dout_i . v_j.
The forms of a Case:  n_q = 1  "cls"    w = NULL (the last block's step; its queries may sit in a buffer of their own)
                      n_q = n  "chain"  w = r of the chain: 1 on the CLS token plus a non-negative vector
Precisions (prec, act_prec): (f16, f16), (bf16, bf16) and (bf16, f16) - fp16 activations under bf16 gradients.  In the last
one q / k / v are genuine fp16 values; the kernel converts v to bf16 as it loads it and so does `values`.
Kinds of dout: "random"    N(0, 1);
               "negative"  v >= 0 and dout <= 0: every product P G <= 0, the result is EXACTLY 0 (the MFMA adds
                           non-positive terms, the clamp returns 0, 0 is added to 0);
               "mixed"     v >= 0 and dout_i = s_i |dout_i| with one sign per query: whole rows of P G vanish.

The bound, per (frame, head) block:   max_j |got - ref| <= C * 2^-23 * f(Smax, n_q) * A,
    A = max_j sum_i |w_i| P[i][j] sum_c |dout_ic v_jc|          (the ABSOLUTE sum: the output itself can cancel to 0)
    f(Smax, n_q) = 1 + Smax + n_q / 16 + 64 / 16,   C = 4,
Smax the largest |score| of the block (fp64).  Where it comes from: a term is c_i exp2(s log2 e - M log2 e) g.  As in
attention_maps_ref, the score leaves the MFMA with a relative error of a few 2^-24 which the exponential turns into an
absolute error |s| 2^-24 of the exponent: the Smax term.  The constant part (exp2, the division by the row sum, the product
with g, the clamp - which never increases an error -, the product with c_i) is the 1.  g is a 64-term dot product accumulated
in fp32 by two chained MFMAs; its error is relative to sum_c |dout_ic v_jc|, not to |g| - which is why A carries that sum -
and grows with the length of the accumulation chain, counted like the query sum at one rounding per sixteen terms: 64 / 16.
A column is the sum of n_q terms: a lane adds every sixteenth query in ascending order (n_q / 16 additions) and four levels
combine sixteen lanes: the n_q / 16 term.  The emulation below, in units of 2^-23 f A over every shape, form, regime, kind and
precision pair of TABLE, reaches 1.2 (the worst: `ramp`, one query; test_relevance_host.py asserts half the bound); C = 4 leaves the other half for what
the emulation does not model - the MFMA's own summation order, the hardware exp2, the fused multiply-add of the accumulation.

The chain: r <- e_cls; for l = L ... 1: r <- r + r A_l, A_l = mean_h max(0, P G) of block l - row 0 of (I + A_L) ... (I + A_1).
A step's error is bounded by the step bound with w = r; over L steps the errors add, each carried through the remaining
factors (I + A_l): chain_from_buffers.

Mutations and where they apply (mutation_applies): a mutation counts where it changes the fp64 result by construction.
  no_clamp      the sum without max(0, .): wherever a product is negative - every kind of dout, but "mixed" with one query
                (its one query is the positive one).
  abs           |.| in place of max(0, .): likewise.
  renorm_own    P renormalised over the frame's own keys, as the ROLLOUT does and this kernel must not: wherever the prompt rows
                carry probability - not `ramp_down` (they are the last keys, e^-55 and below) - and the result is not 0.
  head_swap     heads >= 2 and a non-zero result (G differs between heads in every regime, `uniform` included).
  k_for_v       K in V's place: always (K has both signs, so even the "negative" kind gives a non-zero result).
  drop_last     the last key of the softmax - a prompt row - left out: every remaining probability grows by 1 / (1 - p_last).
                Needs a non-zero result; not `ramp_down` (p_last = e^-60); not `peaked` with n_q = 1 (one near-one-hot row on
                a random key); `hot_side` only where the last key is the hot row of some frame.
"""
import math

import torch

import attention_ref as ar
from attention_ref import F16, BF16, Case, gather, vision, n_keys, n_side, n_queries, DTYPE   # noqa: F401

MAX_KEYS = 640
BOUND_C = 4.0
LOG2E = 1.4426950408889634
REGIMES = ("randn", "peaked", "uniform", "ramp", "ramp_down", "hot_side")
KINDS = ("random", "negative", "mixed")
PAIRS = ((F16, F16), (BF16, BF16), (BF16, F16))            # (prec of dout, act_prec of q / k / v)
MUTATIONS = ("no_clamp", "abs", "renorm_own", "head_swap", "k_for_v", "drop_last")


def forms(c):
    return ("cls",) if n_queries(c) == 1 else ("chain",)


def weights(c, form, seed):
    """fp32 [BT][n_q] for the chain form, else None: r after some steps - 1 on the CLS token plus a non-negative vector."""
    if form != "chain":
        return None
    g = torch.Generator().manual_seed(seed + 7)
    w = torch.randn(c.BT, c.n, generator=g).abs() * 0.05
    w[:, 0] += 1.0
    return w.contiguous()


def make_inputs(c, regime, seed, prec, act, kind):
    """ar.Inputs with q / k / v / side rounded to `act` and dout to `prec` (no pre-rounding of the activations to prec)."""
    q, k, v, sk, sv, do = ar.make_operands(c, regime, seed)
    D, nq = c.heads * 64, n_queries(c)
    if kind in ("negative", "mixed"):
        v = v.abs()
        do = -do.abs()
        if kind == "mixed":
            g = torch.Generator().manual_seed(seed + 13)
            sign = torch.where(torch.rand(c.BT, nq, 1, 1, generator=g) < 0.5, -1.0, 1.0)
            sign[:, 0] = 1.0                                       # the first query is positive: n_q = 1 has something to show
            do = do.abs() * sign
    at = DTYPE[act]
    rows = lambda x, r: x.reshape(r, -1).to(at)
    side = torch.cat([rows(sk, sk.shape[0]), rows(sv, sv.shape[0])], 1) if c.side else None
    return ar.Inputs(rows(q, c.BT * nq), rows(k, c.BT * c.n), rows(v, c.BT * c.n), side, do.reshape(c.BT * nq, D).to(DTYPE[prec]))


def values(c, x, prec):
    """V fp64 [BT][H][n][64] of the frame's own rows as the kernel multiplies it: converted to dout's type."""
    v = x.v.to(DTYPE[prec]).double()
    return v.view(c.BT, c.n, c.heads, 64).transpose(1, 2)


def _parts(c, x, prec, mutate=None):
    K, _ = gather(c, x)
    nq = n_queries(c)
    Q = x.q.double().view(c.BT, nq, c.heads, 64).transpose(1, 2)
    S = Q @ K.transpose(-1, -2)
    smax = S.abs().amax(dim=(2, 3))
    if mutate == "drop_last":
        S = S.clone()
        S[..., -1] = -math.inf
    if mutate == "renorm_own":
        S = S[..., :c.n]
    P = S.softmax(-1)[..., :c.n]
    V = K[:, :, :c.n] if mutate == "k_for_v" else values(c, x, prec)
    dO = x.dout.double().view(c.BT, nq, c.heads, 64).transpose(1, 2)
    return P, V, dO, smax


def reference(c, x, prec, w=None, mutate=None):
    """-> (out fp64 [BT][H][n], Smax fp64 [BT][H], A fp64 [BT][H]: the absolute sum the bound is relative to)."""
    P, V, dO, smax = _parts(c, x, prec, mutate)
    G = dO @ V.transpose(-1, -2)
    PG = P * G
    term = PG if mutate == "no_clamp" else PG.abs() if mutate == "abs" else PG.clamp(min=0)
    wd = torch.ones(c.BT, n_queries(c), dtype=torch.float64) if w is None else w.double()
    out = torch.einsum("fi,fhij->fhj", wd, term)
    if mutate == "head_swap":
        out = out.roll(1, 1)
    A = torch.einsum("fi,fhij->fhj", wd.abs(), P * (dO.abs() @ V.abs().transpose(-1, -2))).amax(-1)
    return out, smax, A


def f_of(smax, nq):
    return 1.0 + smax + nq / 16.0 + 4.0


def bound(c, smax, A):
    """[BT][H]: the bound of each (frame, head) block."""
    return BOUND_C * 2.0 ** -23 * f_of(smax, n_queries(c)) * A


def ratio(c, got, ref, smax, A):
    """max over the blocks of max_j |got - ref| / bound (<= 1 passes); a block with a zero bound must match exactly."""
    err, b = (got.double() - ref).abs().amax(-1), bound(c, smax, A)
    r = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def _last_key_is_hot(c):
    last = (lambda f: c.G + c.BT + f) if c.has_summary else (lambda f: c.G + f // c.T * c.T + c.T - 1)
    return any(ar.hot_row(c, f) == last(f) for f in range(c.BT))


def mutation_applies(c, regime, kind, m):
    zero = kind == "negative"
    if m in ("no_clamp", "abs"):
        return not (kind == "mixed" and n_queries(c) == 1)      # that one query is the positive one
    if m == "k_for_v":
        return True
    if m == "renorm_own":
        return not zero and c.side and regime != "ramp_down"
    if m == "head_swap":
        return not zero and c.heads >= 2
    if m == "drop_last":
        if zero or not c.side or regime == "ramp_down" or (regime == "peaked" and n_queries(c) == 1):
            return False
        return regime != "hot_side" or _last_key_is_hot(c)
    raise ValueError(m)


def emulate(c, x, prec, w=None):
    """The kernel in fp32 torch: fp32 scores and fp32 G (V converted as the kernel converts it), M log2 e rounded once, exp2 of
    the fused s log2 e - M log2 e, a lane's row sum over its four keys of every tile in key order and the four lane groups as
    (g0 + g1) + (g2 + g3), c_i = w_i / sum, a term as max(0, e g) c_i, a column as sixteen per-lane sums over every sixteenth
    query in ascending order, combined as the xor butterfly 8, 4, 2, 1."""
    K, _ = gather(c, x)
    nq, nk, n = n_queries(c), K.shape[2], c.n
    Q = x.q.float().view(c.BT, nq, c.heads, 64).transpose(1, 2)
    S = Q @ K.float().transpose(-1, -2)
    m2 = (S.amax(-1, keepdim=True) * torch.tensor(LOG2E, dtype=torch.float32))
    l2 = torch.tensor(LOG2E, dtype=torch.float32).double()
    e = torch.exp2((S.double() * l2 - m2.double()).float())
    kp = (nk + 15) // 16 * 16
    ep = torch.zeros(*e.shape[:-1], kp)
    ep[..., :nk] = e
    ep = ep.view(*e.shape[:-1], kp // 16, 4, 4)                           # [tile][lane group][r]
    lane = torch.zeros(*e.shape[:-1], 4)
    for t in range(kp // 16):
        for r in range(4):
            lane = lane + ep[..., t, :, r]
    tot = (lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])
    wf = torch.ones(c.BT, nq) if w is None else w.float()
    coef = wf[:, None, :] / tot                                           # [BT][H][nq]
    dO = x.dout.float().view(c.BT, nq, c.heads, 64).transpose(1, 2)
    G = dO @ values(c, x, prec).float().transpose(-1, -2)
    term = (e[..., :n] * G).clamp(min=0) * coef[..., None]
    qp = (nq + 15) // 16 * 16
    tp = torch.zeros(c.BT, c.heads, qp, n)
    tp[:, :, :nq] = term
    tp = tp.view(c.BT, c.heads, qp // 16, 16, n)
    acc = torch.zeros(c.BT, c.heads, 16, n)
    for t in range(qp // 16):
        acc = acc + tp[:, :, t]
    for half in (8, 4, 2, 1):
        acc = acc[:, :, :half] + acc[:, :, half:2 * half]
    return acc[:, :, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the relevance chain
def relevance_matrix(A):
    """A: fp64 [L][n][n], block l's mean_h max(0, P G) over the frame's own tokens -> row 0 of (I + A_L) ... (I + A_1)."""
    n = A.shape[-1]
    eye = torch.eye(n, dtype=A.dtype)
    M = eye
    for l in range(A.shape[0]):                                          # M = (I + A_l) M: block 1 is the rightmost factor
        M = (eye + A[l]) @ M
    return M[0]


def relevance_chain(A):
    """The same row as a vector chain from the last block to the first: r <- r + r A_l - what the device runs, r A_l = mean
    over the heads of gava_attention_relevance(w = r)."""
    r = torch.zeros(A.shape[-1], dtype=A.dtype)
    r[0] = 1
    for l in range(A.shape[0] - 1, -1, -1):
        r = r + r @ A[l]
    return r


def chain_from_buffers(steps, BT, T, G, n, heads, prec):
    """The chain in fp64 from the operands the device's steps ran on, with the bound of the device's r.
    steps: one dict per block in the order the backward visits them (last block first), CPU tensors q [BT*rows][D] (rows =
    1 or n per frame), k, v [BT*n][D], side_k [G + 2 BT][D], dmix [BT*rows][D].  The first step is the one-query form on the
    frame's first row.  -> (r fp64 [BT][n], bound fp64 [BT][n]).
    The bound, element by element: the device's r enters the next step as its weight, and a step is linear in the weight, so
    an error e of r becomes e + e A-_l; to that the step adds the kernel's own error - the per-(frame, head) bound above
    with w = r + e, averaged over the heads as the results are - and the fp32 roundings of the torch ops that follow it,
    the head mean (H additions and a division, each 2^-24 of the running value) and the sum r + mean (2^-24 of the result)."""
    u = 2.0 ** -24
    r = torch.zeros(BT, n, dtype=torch.float64)
    r[:, 0] = 1
    e = torch.zeros(BT, n, dtype=torch.float64)
    for l, st in enumerate(steps):
        rows = st["q"].shape[0] // BT
        D = heads * 64
        if l == 0:            # only the CLS query carries a gradient
            q, dmix, nq = st["q"].view(BT, rows, D)[:, :1].reshape(BT, D), st["dmix"].view(BT, rows, D)[:, :1].reshape(BT, D), 1
        else:
            assert rows == n
            q, dmix, nq = st["q"], st["dmix"], n
        c = vision(BT, T, G, n, heads, n_q=(1 if nq == 1 else 0), qbr=(1 if nq == 1 else 0))
        side = torch.cat([st["side_k"], torch.zeros_like(st["side_k"])], 1)
        x = ar.Inputs(q, st["k"], st["v"], side, dmix)
        P, V, dO, smax = _parts(c, x, prec)
        M = (P * (dO @ V.transpose(-1, -2))).clamp(min=0)                       # [BT][H][nq][n]
        Aabs = P * (dO.abs() @ V.abs().transpose(-1, -2))
        ones = torch.ones(BT, 1, dtype=torch.float64)
        w, we = (ones, ones) if nq == 1 else (r, r + e)
        out = torch.einsum("fi,fhij->fhj", w, M)
        A = torch.einsum("fi,fhij->fhj", we, Aabs).amax(-1)
        kern = (BOUND_C * 2.0 ** -23 * f_of(smax, nq) * A).mean(1)              # [BT]
        step = out.mean(1)
        carried = torch.zeros_like(e) if nq == 1 else torch.einsum("fi,fij->fj", e, M.mean(1))
        if nq == 1:
            r = step.clone()
            r[:, 0] += 1
        else:
            r = r + step
        e = e + carried + kern[:, None] + u * ((heads + 1) * out.abs().mean(1) + r)
    return r, e


# ---------------------------------------------------------------------------------------------------------------------
# the GPU test's table, one case per key-tile class of the kernel (4 | 14 | 26 | 40 tiles), two clips each:
# TINY (17 + 4 + 4 + 1 = 26 keys), ViT-B/16 at T = 8 (214), ViT-L/14 at T = 32 (298), 384 px at P = 16 (594)
def cls(c, qbr=1):
    return c._replace(n_q=1, qbr=qbr)


_FULL = [vision(8, 4, 4, 17), vision(16, 8, 8, 197), vision(64, 32, 8, 257), vision(16, 8, 8, 577)]
TABLE = _FULL + [cls(c) for c in _FULL] + [cls(_FULL[0], qbr=17), cls(_FULL[1], qbr=197)]
TOO_MANY = vision(2, 2, 8, 630)                                          # 641 keys: GAVA_EINVAL


def regimes(c):
    return [r for r in REGIMES if r != "hot_side" or c.G + 2 * c.BT <= 64]


def kinds(regime):
    """Every kind in `randn`; the other score regimes run the random kind."""
    return KINDS if regime == "randn" else ("random",)


def params():
    return [(c, form, r, kind, pair) for c in TABLE for form in forms(c) for r in regimes(c) for kind in kinds(r) for pair in PAIRS]


def param_id(c, form, regime, kind, pair):
    return f"{ar.case_id(c)}-{form}-{regime}-{kind}-{ar.PREC_NAME[pair[1]]}act-{ar.PREC_NAME[pair[0]]}"


def seed_of(c, regime):
    return ar.seed_of(c._replace(n_q=0, qbr=0), regime) + (1 if c.n_q else 0)
