"""Reference side of the attention-map tests (test_attention_maps_host.py, test_gpu_attention_maps.py); nothing here touches
a GPU.  Shapes, operands, regimes and the prompt-row gather come from attention_ref.py.

  * fp64 reference of gava_attention_mass on the 16-bit operands, with the MUTATIONS that apply to it;
  * attention rollout two ways: the vector chain the device runs (row 0 only) and the matrix product it stands for;
  * a torch emulation of the kernel's rounding points in fp32, in the kernel's own summation order;
  * the bound, the forms and the shape table of the GPU test.

The forms of a Case
  n_q = 1   "cls"         w = NULL, renorm = 0: the CLS row over all keys
            "cls_renorm"  w = NULL, renorm = 1: the first step of the rollout chain
  n_q = n   "chain"       w = a probability vector (half of it on the CLS token, as the chain's r), renorm = 1
            "mass"        w = NULL, renorm = 0: the column sums of P over all keys

The bound, per (frame, head) block:   max_j |got - ref| <= C * 2^-23 * f(Smax, n_q) * max_j |ref|,
    f(Smax, n_q) = 1 + Smax + n_q / 16,   C = 4,
Smax the largest |score| of the block (fp64).  Where it comes from: a probability is exp2(s log2 e - M log2 e) / sum; the
score s leaves the MFMA with a relative error of a few 2^-24, which the exponential turns into an ABSOLUTE error of the
exponent, |s| 2^-24: the Smax term.  The constant part (the exp2 itself, the division, the product with w) is the 1.  A
column is then the sum of n_q such terms; a lane adds every sixteenth query in ascending order (n_q / 16 additions, each
rounding at 2^-24 of the running sum) and four more levels combine sixteen lanes: the n_q / 16 term.  In `uniform` (Smax = 0,
every term equal) that term is the whole error.  The emulation below, in units of 2^-23 f max|ref|, over every shape,
form, regime and precision of TABLE: 0.07 to 0.96 in the two n_q = n forms, 0.22 to 1.87 in the CLS forms (the worst: `ramp`,
210 keys, fp16 - one query, so nothing averages the exponent's error out); C = 4 leaves the factor 2 over 1.87 for what the
emulation does not model - the MFMA's own summation order, the hardware exp2 and the fused multiply-add of the column
accumulation.  At every shape of TABLE the bound stays below 1e-4 of max|ref| (test_attention_maps_host.py checks both).

renorm = 1 needs no second row sum: P restricted to the frame's own keys and renormalised IS the softmax over those keys
alone, which is how the kernel and this reference compute it (the prompt rows are not read).

Mutations and where they apply (mutation_applies): a mutation counts where it changes the fp64 result by construction, not
by the luck of a random score.
  drop_last / last_is_key0   act on the last key the form reads (renorm forms: the frame's last own key).  drop_last does
                             not apply in `ramp_down`, where that key's probability is e^-60 of the row; last_is_key0 does
                             not apply in `uniform`, where q = 0 and no key's VALUE reaches the result.
  neighbour_local / _summary another clip's / frame's prompt row: the forms that read prompt rows (cls, mass) only; not in
                             `uniform` (q = 0) and not in `ramp_down` (the prompt rows are the last keys, e^-55 and below).
  head_swap                  heads >= 2; not in `uniform`, where every head has the same probabilities.
  one key, one query         drop_last, last_is_key0 and neighbour_summary touch ONE key.  In `peaked` with n_q = 1 a block
                             is one near-one-hot row on a random key (score deviation 8), so that key carries nothing
                             unless chance puts the maximum there: they do not apply.  In `hot_side` the forms that read
                             prompt rows put 0.9 of every row on the frame's hot prompt row: they apply where that row is
                             the touched key for some frame (attention_ref.hot_row: with two frames no summary row is hot).
"""
import math

import torch

import attention_ref as ar
from attention_ref import F16, BF16, Case, make_inputs, gather, MUTATIONS, vision, n_keys, n_side, n_queries   # noqa: F401

MAX_KEYS = 640
BOUND_C = 4.0
LOG2E = 1.4426950408889634
REGIMES = ("randn", "peaked", "uniform", "ramp", "ramp_down", "hot_side")
MASS_MUTATIONS = ("drop_last", "last_is_key0", "neighbour_local", "neighbour_summary", "head_swap")
assert set(MASS_MUTATIONS) <= set(MUTATIONS)


def forms(c):
    return ("cls", "cls_renorm") if n_queries(c) == 1 else ("chain", "mass")


def renorm_of(form):
    return form in ("cls_renorm", "chain")


def n_out(c, form):
    return c.n if renorm_of(form) else n_keys(c)


def weights(c, form, seed):
    """fp32 [BT][n_q] for the forms that pass w, else None: r of the rollout chain after a step - half on the CLS token, the
    other half a probability vector over all tokens."""
    if form != "chain":
        return None
    g = torch.Generator().manual_seed(seed + 7)
    w = 0.5 * torch.randn(c.BT, c.n, generator=g).softmax(-1)
    w[:, 0] += 0.5
    return w.contiguous()


def _last_key_is_hot(c):
    """hot_side, forms that read prompt rows: is the last key the hot row of some frame?"""
    last = (lambda f: c.G + c.BT + f) if c.has_summary else (lambda f: c.G + f // c.T * c.T + c.T - 1)
    return any(ar.hot_row(c, f) == last(f) for f in range(c.BT))


def mutation_applies(c, form, regime, m):
    one_key = m in ("drop_last", "last_is_key0", "neighbour_summary")
    if one_key and regime == "peaked" and n_queries(c) == 1:
        return False
    if one_key and regime == "hot_side" and not renorm_of(form) and not (_last_key_is_hot(c) and (c.has_summary or m != "neighbour_summary")):
        return False
    if m in ("drop_last", "last_is_key0"):
        if (c.n if renorm_of(form) else n_keys(c)) < 2:
            return False
        return regime != ("ramp_down" if m == "drop_last" else "uniform")
    if m in ("neighbour_local", "neighbour_summary"):
        return not renorm_of(form) and regime not in ("uniform", "ramp_down") and ar.mutation_applies(c, m)
    if m == "head_swap":
        return c.heads >= 2 and regime != "uniform"
    return False


def scores(c, x, form, mutate=None):
    """fp64 S [BT][H][n_q][keys the form reads], the mutation applied."""
    K, _ = gather(c, x, mutate if mutate in ("neighbour_local", "neighbour_summary") else None)
    if renorm_of(form):
        K = K[:, :, :c.n]
    if mutate == "last_is_key0":
        K = torch.cat([K[:, :, :-1], K[:, :, :1]], 2)
    Q = x.q.double().view(c.BT, n_queries(c), c.heads, 64).transpose(1, 2)
    S = Q @ K.transpose(-1, -2)
    if mutate == "drop_last":
        S = S.clone()
        S[..., -1] = -math.inf
    return S


def reference(c, x, form, w=None, mutate=None):
    """-> (out fp64 [BT][H][n_out], Smax fp64 [BT][H])."""
    S = scores(c, x, form, mutate)
    P = S.softmax(-1)
    wd = torch.ones(c.BT, n_queries(c), dtype=torch.float64) if w is None else w.double()
    out = torch.einsum("fi,fhij->fhj", wd, P)
    if mutate == "head_swap":
        out = out.roll(1, 1)
    return out, S.masked_fill(S.isinf(), 0).abs().amax(dim=(2, 3))


def f_of(smax, nq):
    return 1.0 + smax + nq / 16.0


def bound(c, ref, smax):
    """[BT][H]: the bound of each (frame, head) block."""
    return BOUND_C * 2.0 ** -23 * f_of(smax, n_queries(c)) * ref.abs().amax(-1)


def ratio(c, got, ref, smax):
    """max over the blocks of max_j |got - ref| / bound (<= 1 passes)."""
    return float(((got.double() - ref).abs().amax(-1) / bound(c, ref, smax)).max())


def emulate(c, x, form, w=None):
    """The kernel in fp32 torch: fp32 scores, M log2 e rounded once, exp2 of the fused s log2 e - M log2 e, a lane's row sum
    over its four keys of every tile in key order and the four lane groups as (g0 + g1) + (g2 + g3), c_i = w_i / sum, a
    column as sixteen per-lane sums over every sixteenth query in ascending order, combined as the xor butterfly 8, 4, 2, 1."""
    K, _ = gather(c, x)
    if renorm_of(form):
        K = K[:, :, :c.n]
    nq, nk = n_queries(c), K.shape[2]
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
    term = e * coef[..., None]
    qp = (nq + 15) // 16 * 16
    tp = torch.zeros(c.BT, c.heads, qp, nk)
    tp[:, :, :nq] = term
    tp = tp.view(c.BT, c.heads, qp // 16, 16, nk)
    acc = torch.zeros(c.BT, c.heads, 16, nk)
    for t in range(qp // 16):
        acc = acc + tp[:, :, t]
    for half in (8, 4, 2, 1):
        acc = acc[:, :, :half] + acc[:, :, half:2 * half]
    return acc[:, :, 0]


# ---------------------------------------------------------------------------------------------------------------------
# attention rollout
def rollout_matrix(A):
    """A: fp64 [L][n][n], block l's probabilities over the frame's own tokens, averaged over the heads, rows summing to 1
    -> row 0 of A^_L ... A^_1, A^_l = (I + A_l) / 2, by the matrix products."""
    n = A.shape[-1]
    eye = torch.eye(n, dtype=A.dtype)
    M = eye
    for l in range(A.shape[0]):                                          # M = A^_l M: block 1 is the rightmost factor
        M = 0.5 * (eye + A[l]) @ M
    return M[0]


def rollout_chain(A):
    """The same row as a vector chain from the last block to the first: r <- r / 2 + (r A_l) / 2 - what the device runs,
    r A_l = mean over the heads of gava_attention_mass(w = r, renorm = 1)."""
    r = torch.zeros(A.shape[-1], dtype=A.dtype)
    r[0] = 1
    for l in range(A.shape[0] - 1, -1, -1):
        r = 0.5 * r + 0.5 * (r @ A[l])
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the GPU test's table: vision(BT, T, G, n, heads, n_q, qbr, has_summary)
def cls(c, qbr=1):
    return c._replace(n_q=1, qbr=qbr)


TABLE = [
    vision(4, 2, 8, 20), vision(4, 2, 8, 21), vision(4, 2, 8, 22),      # 31 | 32 | 33 keys, two clips, two heads
    cls(vision(4, 2, 8, 21)), cls(vision(4, 2, 8, 22), qbr=3),           # the CLS row, its queries in a buffer of their own
    vision(4, 2, 0, 32),                                                 # n a tile multiple, G = 0
    vision(4, 2, 8, 48, has_summary=False),                              # n a tile multiple, no summary row
    vision(2, 2, 0, 61), vision(2, 2, 0, 62),                            # 64 | 65 keys: the first LDS class's edge
    vision(4, 4, 8, 197), cls(vision(4, 4, 8, 197)),                     # ViT-B/16 at T = 4: 210 keys
    vision(2, 2, 8, 213), vision(2, 2, 8, 214),                          # 224 | 225 keys
    vision(2, 2, 6, 401),                                                # 410 keys / 401 queries
    vision(2, 2, 8, 405), vision(2, 2, 8, 406),                          # 416 | 417 keys
    vision(2, 2, 8, 629), cls(vision(2, 2, 8, 629)),                     # 640 keys: the limit
]
# renorm = 1 scores the frame's own keys only, so its LDS classes turn on n: the chain form at 64 | 65, 224 | 225, 416 | 417
TABLE_CHAIN = [vision(2, 2, 8, n) for n in (64, 65, 224, 225, 416, 417)]
TOO_MANY = vision(2, 2, 8, 630)                                          # 641 keys: GAVA_EINVAL


def regimes(c):
    return [r for r in REGIMES if r != "hot_side" or c.G + 2 * c.BT <= 64]


def params():
    return ([(c, form, r, p) for c in TABLE for form in forms(c) for r in regimes(c) for p in (F16, BF16)] +
            [(c, "chain", r, p) for c in TABLE_CHAIN for r in ("randn", "peaked") for p in (F16, BF16)])


def param_id(c, form, regime, prec):
    return f"{ar.case_id(c)}-{form}-{regime}-{ar.PREC_NAME[prec]}"


def seed_of(c, regime):
    return ar.seed_of(c._replace(n_q=0, qbr=0), regime) + (1 if c.n_q else 0)
