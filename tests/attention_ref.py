"""Reference side of the attention edge tests (test_attention_ref_host.py, test_gpu_attention_edges.py); nothing here
touches a GPU.

  * fp64 reference of gava_attention / gava_attention_backward on the 16-bit-rounded operands: plain, causal, prompt
    rows (n_g | T | summary), n_q < n with the queries in their own buffer; forward, dq / dk / dv and the prompt rows'
    gradients, with optional MUTATIONS (the bugs the bounds must catch);
  * the scale tensors of the bounds;
  * a plain torch emulation of the kernels' rounding points, from which the bounds' constants are checked on the CPU;
  * the value regimes;
  * a restatement of the two host dispatchers (attention.hip launch_attn, attention_bwd.hip launch) and the shape
    tables of the GPU tests, so that the host test can check that the tables reach every instantiation.

The bounds
  forward   |out - ref| <= 4 eps * scale + floor,  scale = sum_k p_k |v_k| per output element.  The kernel rounds P to 16
            bits, sums the ROUNDED P for the denominator and rounds the output: to first order 3 eps * scale; one more eps
            for the fp32 summation order and the hardware exp2 / rcp.  floor (fp16 only) = n_keys * 2^-25 * max|v|: P below
            the fp16 normal range is rounded with an absolute, not a relative, error.
  backward  per (problem, head) block  max|got - ref| <= 3 eps * max|ref| over that block (3 eps is the constant of the
            existing backward tests; the block replaces their whole tensor).  Where the inputs make dq or dk a
            cancelling sum, its size says nothing about its error and the scale is the block's maximum of
            q_scale * sum_k |dS_ik| |K_kd| resp. sum_q |dS_qk| |Q_qd|: which regimes and why is written at CANCEL_DQ /
            CANCEL_DK.  The prompt rows' partials are first summed over the frames sharing a row, then bounded per row
            group (global | one clip's local rows | one clip's summary rows) and head.  No absolute floor, with one
            exception: fp16 gradients of the prompt rows in `ramp_down` (see backward_ratios).
"""
import math
from collections import namedtuple

import torch

F16, BF16 = 0, 1                                  # hip.PREC_F16 / hip.PREC_BF16
DTYPE = {F16: torch.float16, BF16: torch.bfloat16}
EPS = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
PREC_NAME = {F16: "f16", BF16: "bf16"}
FWD_C, BWD_C = 4.0, 3.0                           # the bounds' constants (see above)

# A problem set: BT frames (or sequences) of n rows, `heads` heads of 64; side = prompt rows (G global | T local | summary);
# n_q queries per frame (0 = all n); qbr = rows per frame of the separate query buffer (0 = q lives beside k and v)
Case = namedtuple("Case", "BT T G n heads n_q qbr causal has_summary side split", defaults=(0, 0, False, True, True, False))


def plain(B, L, heads=2, causal=False, split=False):
    return Case(B, 1, 0, L, heads, 0, 0, causal, False, False, split)


def vision(BT, T, G, n, heads=2, n_q=0, qbr=0, has_summary=True, split=False):
    return Case(BT, T, G, n, heads, n_q, qbr, False, has_summary, True, split)


def n_side(c):
    return c.G + c.T + int(c.has_summary) if c.side else 0


def n_keys(c):
    return c.n + n_side(c)


def n_queries(c):
    return c.n_q or c.n


def case_id(c):
    s = f"keys{n_keys(c)}-q{n_queries(c)}-b{c.BT}h{c.heads}"
    if c.side:
        s += f"-T{c.T}G{c.G}" + ("" if c.has_summary else "-nosum")
    if c.causal:
        s += "-causal"
    if c.qbr:
        s += f"-qbr{c.qbr}"
    if c.split:
        s += "-split"
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the gather (moved here from test_gpu_long_attention.py, which imports it back)
def side_index(BT, T, G, device):
    """[BT][G + T + 1] rows of the side matrix that frame f attends to (gava_attention's layout)."""
    f = torch.arange(BT, device=device)
    glob = torch.arange(G, device=device).expand(BT, G)
    loc = G + (f // T * T)[:, None] + torch.arange(T, device=device)[None]
    return torch.cat([glob, loc, (G + BT + f)[:, None]], 1)


def ref_attention(q, k, v, side, BT, T, G, n, heads, nq):
    """fp64: q [BT][nq][D] (pre-scaled), k / v [BT][n][D], side [G + 2 BT][2D] or None -> [BT][nq][D]."""
    D = heads * 64
    if side is not None:
        idx = side_index(BT, T, G, q.device)
        k = torch.cat([k, side[idx, :D]], 1)
        v = torch.cat([v, side[idx, D:]], 1)
    qh = q.double().view(BT, nq, heads, 64).transpose(1, 2)
    kh = k.double().view(BT, -1, heads, 64).transpose(1, 2)
    vh = v.double().view(BT, -1, heads, 64).transpose(1, 2)
    return ((qh @ kh.transpose(-1, -2)).softmax(-1) @ vh).transpose(1, 2).reshape(BT, nq, D)


# ---------------------------------------------------------------------------------------------------------------------
# regimes: functions of (case, seed) -> fp32 q [BT][nq][H][64] (scaled), k, v [BT][n][H][64], sk, sv [R][H][64], dout
REGIMES = ("randn", "peaked", "uniform", "offset", "ramp", "ramp_down", "hot_side")
# Where the backward bound's scale is not the block's max|ref| (emulation figures in units of eps * scale, bound 3):
#   dq against q_scale * sum_k |dS_ik| |K_kd| in `offset` and the ramps (ramp_down is ramp mirrored): dq is a cancelling
#       sum there, 8 to 15 under max|ref|;
#   dk and the prompt rows' K half against sum_q |dS_qk| |Q_qd| in the ramps and in `hot_side`: every query carries the same
#       large component (1 in head dim 0; 3 along the hot row's head dim - that shared direction is what puts the maximum
#       of every query of a frame on one prompt row, so it cannot be taken out of the input), which makes that column of
#       dk a sum over the queries of dS of either sign: up to 3.3 under max|ref|, the K half of the prompt rows 2.6.
#       That scale is 15 to 116 times max|ref| and the emulation reaches only 0.05 to 0.36 of 3 under it: in these three
#       regimes dk and the K half are bounded against gross errors only (a wrong maximum or rescale), and a wrong gather
#       there is caught through dv, dq and the prompt rows' V half (the hot_side mutation tests), not through dk.
# Everything else - dk and the prompt rows in `offset` (1.37, 1.02), dq in `hot_side` (1.45), the prompt rows' V half
# everywhere - keeps max|ref|.
CANCEL_DQ = ("offset", "ramp", "ramp_down")
CANCEL_DK = ("ramp", "ramp_down", "hot_side")


def _key_ramp(c, lo, hi):
    """Column 0 of every head's K row = linspace(lo, hi) along the key order the kernel sees (prompt rows last).  A prompt
    row has the same key position in every frame that sees it, so the shared side matrix can carry the ramp."""
    nk = n_keys(c)
    ramp = torch.linspace(lo, hi, nk)
    main = ramp[:c.n]
    side = torch.zeros(c.G + 2 * c.BT)
    if c.side:
        side[:c.G] = ramp[c.n:c.n + c.G]
        side[c.G:c.G + c.BT] = ramp[c.n + c.G:c.n + c.G + c.T].repeat(c.BT // c.T)
        if c.has_summary:
            side[c.G + c.BT:] = ramp[nk - 1]
    return main, side


def hot_row(c, f):
    """hot_side: the side-matrix row on which frame f's row maximum sits - a global row, the frame's own local row and
    its summary row in turn."""
    kinds = ([0] if c.G else []) + [1] + ([2] if c.has_summary else [])
    kind = kinds[f % len(kinds)]
    return (f % c.G) if kind == 0 else (c.G + f if kind == 1 else c.G + c.BT + f)


def make_operands(c, regime, seed):
    g = torch.Generator().manual_seed(seed)
    H, nq, R = c.heads, n_queries(c), c.G + 2 * c.BT
    q = torch.randn(c.BT, nq, H, 64, generator=g)
    k = torch.randn(c.BT, c.n, H, 64, generator=g)
    v = torch.randn(c.BT, c.n, H, 64, generator=g)
    sk = torch.randn(R, H, 64, generator=g)
    sv = torch.randn(R, H, 64, generator=g)
    do = torch.randn(c.BT, nq, H, 64, generator=g)
    if regime == "randn":
        q *= 0.125
    elif regime == "peaked":
        pass                                                         # q * 8: score standard deviation 8
    elif regime == "uniform":
        q.zero_()
    elif regime == "offset":
        q = q.abs() * 0.125
        k += 4
        sk += 4
    elif regime in ("ramp", "ramp_down"):
        q *= 0.125
        q[..., 0] = 1
        main, side = _key_ramp(c, -30, 30) if regime == "ramp" else _key_ramp(c, 30, -30)
        k[..., 0] = main[None, :, None]
        sk[..., 0] = side[:, None]
    elif regime == "hot_side":
        assert c.side and R <= 64
        # side row r points along head-dim r: frame f's queries point at hot_row(f) (score 9 there, about N(0, 1) elsewhere:
        # P = 0.9 to 0.97 on that row, and gradients that do not all underflow); V of side row r is the constant (r + 1) / 8,
        # so another frame's or clip's row is an O(1) error
        q *= 0.125
        k *= 0.25
        sk *= 0.25
        for r in range(R):
            sk[r, :, r] = 3
            sv[r] = (r + 1) / 8
        for f in range(c.BT):
            q[f, :, :, hot_row(c, f)] = 3
    else:
        raise ValueError(regime)
    return q, k, v, sk, sv, do


Inputs = namedtuple("Inputs", "q k v side dout")     # 16-bit tensors: q [BT*nq][D], k / v [BT*n][D], side [R][2D] | None, dout


def make_inputs(c, regime, seed, prec, act_prec=None):
    """The operands rounded to 16 bits.  act_prec != prec (fp16 activations under bf16 gradients): the values are rounded to
    `prec` and stored as act_prec, as the existing mixed test does - the kernel's conversion on load is then exact."""
    q, k, v, sk, sv, do = make_operands(c, regime, seed)
    D, dt = c.heads * 64, DTYPE[prec]
    at = DTYPE[prec if act_prec is None else act_prec]

    def act(x, rows):
        return x.reshape(rows, -1).to(dt).float().to(at)
    side = torch.cat([act(sk, sk.shape[0]), act(sv, sv.shape[0])], 1) if c.side else None
    nq = n_queries(c)
    return Inputs(act(q, c.BT * nq), act(k, c.BT * c.n), act(v, c.BT * c.n), side, do.reshape(c.BT * nq, D).to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference, with mutations
MUTATIONS = ("drop_last", "last_is_key0", "neighbour_local", "neighbour_summary", "causal_plus", "causal_minus", "head_swap")


def mutation_applies(c, m):
    if m == "drop_last":
        return n_keys(c) >= 2
    if m == "last_is_key0":           # an unmasked padding row; causal: the padding lies behind the diagonal of every query
        return n_keys(c) >= 2 and not c.causal
    if m == "neighbour_local":
        return c.side and c.BT > c.T
    if m == "neighbour_summary":
        return c.side and c.has_summary and c.BT > 1
    if m in ("causal_plus", "causal_minus"):
        return c.causal and c.n >= 2
    return c.heads >= 2                                              # head_swap


def gather(c, x, mutate=None):
    """-> K, V fp64 [BT][H][keys][64] as frame f sees them."""
    D, BT = c.heads * 64, c.BT
    k = x.k.double().view(BT, c.n, D)
    v = x.v.double().view(BT, c.n, D)
    if c.side:
        idx = side_index(BT, c.T, c.G, "cpu")
        if mutate == "neighbour_local":
            idx[:, c.G:c.G + c.T] = c.G + ((idx[:, c.G:c.G + c.T] - c.G + c.T) % BT)
        if mutate == "neighbour_summary":
            idx[:, -1] = c.G + BT + (torch.arange(BT) + 1) % BT
        if not c.has_summary:
            idx = idx[:, :-1]
        s = x.side.double()
        k = torch.cat([k, s[idx, :D]], 1)
        v = torch.cat([v, s[idx, D:]], 1)
    if mutate == "last_is_key0":
        k = torch.cat([k[:, :-1], k[:, :1]], 1)
        v = torch.cat([v[:, :-1], v[:, :1]], 1)
    split = lambda t: t.view(BT, -1, c.heads, 64).transpose(1, 2)
    return split(k), split(v)


Ref = namedtuple("Ref", "out scale floor_v dq dk dv dside dq_cancel dk_cancel dside_cancel floors")


def reference(c, x, backward=False, mutate=None, q_scale=0.125):
    """fp64.  out, scale: [BT*nq][D].  Backward: dq [BT*nq][D] (times q_scale), dk, dv [BT*n][D], dside [BT][n_side][2D] (the
    per-frame partials, k | v), dq_cancel = q_scale * sum_k |dS| |K|."""
    BT, H, nq, nk = c.BT, c.heads, n_queries(c), n_keys(c)
    D = H * 64
    K, V = gather(c, x, mutate)
    Q = x.q.double().view(BT, nq, H, 64).transpose(1, 2)
    S = Q @ K.transpose(-1, -2)
    vis = torch.ones(nq, nk, dtype=torch.bool)
    if c.causal:
        off = {"causal_plus": 1, "causal_minus": -1}.get(mutate, 0)
        i, j = torch.arange(nq)[:, None], torch.arange(nk)[None]
        vis = j <= (i + off).clamp(min=0)
    if mutate == "drop_last":
        vis = vis.clone()
        vis[:, nk - 1] = False
        if c.causal:
            vis[0, 0] = True
    S = S.masked_fill(~vis, -math.inf)
    P = S.softmax(-1)
    rows = lambda t: t.transpose(1, 2).reshape(BT * t.shape[2], D)
    swap = (lambda t: t.view(t.shape[0], H, 64).roll(1, 1).reshape(t.shape[0], D)) if mutate == "head_swap" else (lambda t: t)
    out, scale = swap(rows(P @ V)), rows(P @ V.abs())
    floor_v = V.abs().amax(dim=(2, 3))[:, None, :, None].expand(BT, nq, H, 64).reshape(BT * nq, D)
    if not backward:
        return Ref(out, scale, floor_v, *[None] * 8)
    dO = x.dout.double().view(BT, nq, H, 64).transpose(1, 2)
    dP = dO @ V.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dq = rows(dS @ K) * q_scale
    dq_cancel = rows(dS.abs() @ K.abs()) * q_scale
    # (with last_is_key0 the stand-in's gradient lands on the last key and none of it on key 0, as it would in the kernel)
    dK, dV, dKc = dS.transpose(-1, -2) @ Q, P.transpose(-1, -2) @ dO, dS.abs().transpose(-1, -2) @ Q.abs()
    dk, dv, dk_cancel = rows(dK[:, :, :c.n]), rows(dV[:, :, :c.n]), rows(dKc[:, :, :c.n])
    dside = dside_cancel = None
    if c.side:
        ns = nk - c.n
        side_rows = lambda a, b: torch.cat([a[:, :, c.n:].transpose(1, 2).reshape(BT, ns, D), b[:, :, c.n:].transpose(1, 2).reshape(BT, ns, D)], 2)
        dside, dside_cancel = side_rows(dK, dV), side_rows(dKc, dV.abs())
        if mutate == "head_swap":
            dside = torch.cat([swap(dside[..., :D].reshape(-1, D)), swap(dside[..., D:].reshape(-1, D))], 1).view(BT, ns, 2 * D)
    # per-frame floor of the prompt rows' partials, used for fp16 gradients in `ramp_down` only (see backward_ratios): P and dS
    # below the fp16 normal range carry an absolute error of 2^-25 each, times the other operand and the n_q queries summed
    u = 2.0 ** -25
    floors = {"k": nq * u * float(Q.abs().max()), "v": nq * u * float(dO.abs().max())}
    return Ref(out, scale, floor_v, swap(dq), swap(dk), swap(dv), dside, dq_cancel, dk_cancel, dside_cancel, floors)


def sum_side_partials(c, part):
    """Per-frame partials [BT][n_side][W] -> the rows' gradients {group name: [rows][W]}: global rows summed over every
    frame, a clip's local rows over its T frames, summary rows as they are; one group per clip for the last two."""
    BT, T, G = c.BT, c.T, c.G
    pv = part.view(BT // T, T, -1, part.shape[-1])
    groups = {}
    if G:
        groups["global"] = pv[:, :, :G].sum(dim=(0, 1))
    for clip in range(BT // T):
        groups[f"local{clip}"] = pv[clip, :, G:G + T].sum(0)
        if c.has_summary:
            groups[f"summary{clip}"] = pv[clip, :, G + T]
    return groups


# ---------------------------------------------------------------------------------------------------------------------
# bounds
def forward_bound(c, ref, prec):
    b = FWD_C * EPS[prec] * ref.scale
    if prec == F16:
        b = b + n_keys(c) * 2.0 ** -25 * ref.floor_v
    return b


def forward_ratio(c, got, ref, prec):
    """max over the elements of |got - ref| / bound (<= 1 passes); elements with a zero bound must match exactly."""
    err, b = (got.double() - ref.out).abs(), forward_bound(c, ref, prec)
    r = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def _blocks(t, rows_per_block, heads):
    """[B * rows][heads*64] -> [B][heads] maxima of |t|."""
    return t.abs().view(-1, rows_per_block, heads, 64).amax(dim=(1, 3))


def block_ratio(got, ref, scale, rows_per_block, heads, prec, floor=0.0):
    """max over the (problem, head) blocks of  max|got - ref| / (3 eps max|scale| + floor)."""
    err = _blocks(got.double() - ref, rows_per_block, heads)
    b = BWD_C * EPS[prec] * _blocks(scale, rows_per_block, heads) + floor
    r = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def backward_ratios(c, got, ref, prec, regime):
    """got: (dq, dk, dv, dside partials or None) -> {name: ratio}; every ratio <= 1 passes.  Scales per regime: CANCEL_DQ,
    CANCEL_DK; everything else against the block's max|ref|."""
    dq, dk, dv, dside = got
    nq = n_queries(c)
    out = {"dq": block_ratio(dq, ref.dq, ref.dq_cancel if regime in CANCEL_DQ else ref.dq, nq, c.heads, prec),
           "dk": block_ratio(dk, ref.dk, ref.dk_cancel if regime in CANCEL_DK else ref.dk, c.n, c.heads, prec),
           "dv": block_ratio(dv, ref.dv, ref.dv, c.n, c.heads, prec)}
    if c.side:
        gs, rs = sum_side_partials(c, dside.double()), sum_side_partials(c, ref.dside)
        ss = sum_side_partials(c, ref.dside_cancel) if regime in CANCEL_DK else rs
        D = c.heads * 64
        half = lambda t, o: t[:, o:o + D].reshape(-1, D)
        # fp16 gradients in `ramp_down`: the prompt rows are the LAST keys, P there is about e^-60 and its fp16 rounding is 0,
        # so the whole group is below what fp16 P and dS can carry and a relative bound means nothing: the one place with
        # an absolute floor, per group (frames summed: all for a global row, T for a local one, 1 for a summary row) and
        # per half (K: dS times Q, V: P times dO)
        def floor(g, o):
            if prec != F16 or regime != "ramp_down":
                return 0.0
            frames = c.BT if g == "global" else (c.T if g.startswith("local") else 1)
            return frames * ref.floors["k" if o == 0 else "v"]
        # the other scale for the K half only (o == 0): the V half, P^T dO, never needs it (at most 0.91 of 3 under max|ref|)
        out["dside"] = max(block_ratio(half(gs[g], o), half(rs[g], o), half(ss[g] if o == 0 else rs[g], o), rs[g].shape[0], c.heads,
                                       prec, floor(g, o)) for g in rs for o in (0, D))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# emulation of the kernels' rounding points (fp32 torch)
def _visible(c):
    nq, nk = n_queries(c), n_keys(c)
    if not c.causal:
        return torch.ones(nq, nk, dtype=torch.bool)
    return torch.arange(nk)[None] <= torch.arange(nq)[:, None]


def emulate_forward(c, x, prec):
    """fp32 scores from the 16-bit operands, P rounded to the operand type, denominator from the rounded P, output rounded;
    past 320 keys the streaming kernel's order: 128-key blocks, P relative to the running maximum, accumulators rescaled."""
    dt = DTYPE[prec]
    K, V = gather(c, x)
    K, V = K.float(), V.float()
    Q = x.q.float().view(c.BT, n_queries(c), c.heads, 64).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)).masked_fill(~_visible(c), -math.inf)
    nk = n_keys(c)
    if nk <= 320 or c.causal:
        P = (S - S.amax(-1, keepdim=True)).exp().to(dt).float()
        o = (P @ V) / P.sum(-1, keepdim=True)
    else:
        m = torch.full(S.shape[:-1] + (1,), -math.inf)
        o, den = torch.zeros(S.shape[:-1] + (64,)), torch.zeros_like(m)
        for b0 in range(0, nk, 128):
            sb = S[..., b0:b0 + 128]
            mn = torch.maximum(m, sb.amax(-1, keepdim=True))
            alpha = (m - mn).exp()
            P = (sb - mn).exp().to(dt).float()
            o = o * alpha + P @ V[..., b0:b0 + 128, :]
            den = den * alpha + P.sum(-1, keepdim=True)
            m = mn
        o = o / den
    return o.transpose(1, 2).reshape(-1, c.heads * 64).to(dt)


def emulate_backward(c, x, prec, q_scale=0.125):
    """The two kernels: dQ from dS = P (dP - delta) formed in fp32 and rounded once to the gradient type; dK / dV from P and dS
    recomputed with the dQ kernel's row statistics and rounded to the gradient type between the products; fp32 prompt-row
    partials.  Operands stored in another type are converted to the gradient type on load."""
    dt = DTYPE[prec]
    BT, H, nq, D = c.BT, c.heads, n_queries(c), c.heads * 64
    K, V = gather(c, x)
    K, V = K.float().to(dt).float(), V.float().to(dt).float()
    Q = x.q.float().to(dt).float().view(BT, nq, H, 64).transpose(1, 2)
    dO = x.dout.float().view(BT, nq, H, 64).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)).masked_fill(~_visible(c), -math.inf)
    m = S.amax(-1, keepdim=True)
    e = (S - m).exp()
    l = e.sum(-1, keepdim=True)
    P = e / l
    dP = dO @ V.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS16 = (P * (dP - delta)).to(dt).float()
    rows = lambda t: t.transpose(1, 2).reshape(BT * t.shape[2], D)
    dq = rows((dS16 @ K) * q_scale).to(dt)
    P2 = (S - (m + l.log())).exp()                                   # the dK/dV kernel: exp2(s log2e - L2)
    P16, dS2 = P2.to(dt).float(), (P2 * (dP - delta)).to(dt).float()
    dK, dV = dS2.transpose(-1, -2) @ Q, P16.transpose(-1, -2) @ dO
    dk, dv = rows(dK[:, :, :c.n]).to(dt), rows(dV[:, :, :c.n]).to(dt)
    dside = None
    if c.side:
        ns = n_keys(c) - c.n
        dside = torch.cat([dK[:, :, c.n:].transpose(1, 2).reshape(BT, ns, D), dV[:, :, c.n:].transpose(1, 2).reshape(BT, ns, D)], 2)
    return dq, dk, dv, dside


# ---------------------------------------------------------------------------------------------------------------------
# the dispatchers, restated.  Names are what a test report shows; the sets below are what the host code can launch with no
# environment switch set.
FWD_CLASSES = ((2, 0), (6, 2), (14, 6), (20, 14))                    # (key tiles N, tiles of the class below)


def forward_form(keys, n_q, causal, split, prec):
    """attention.hip launch_attn (the persistent kernel aside: it needs 4 problems per CU)."""
    p, tiles = PREC_NAME[prec], (keys + 15) // 16
    if not causal and tiles > 20:
        return f"stream<{p}>"
    if causal and keys > 320:
        return None                                                  # GAVA_EINVAL
    N, low = next((N, low) for N, low in FWD_CLASSES if tiles <= N)
    if causal:
        return f"attn<{p},{N},causal>"
    if not split and n_q >= 64 and N >= 14:
        return f"attn<{p},{N},pair,full{N - 1 if tiles == N else low}>"
    return f"attn<{p},{N},one>"


def forward_forms_all():
    forms = set()
    for p in PREC_NAME.values():
        forms.add(f"stream<{p}>")
        for N, low in FWD_CLASSES:
            forms |= {f"attn<{p},{N},causal>", f"attn<{p},{N},one>"}
            if N >= 14:
                forms |= {f"attn<{p},{N},pair,full{N - 1}>", f"attn<{p},{N},pair,full{low}>"}
    return forms


PERSISTENT_FORMS = {f"persist<{p},14,13>" for p in PREC_NAME.values()}   # run by test_gpu_ops.test_attention_plain_and_causal
BWD_PRECS = ((BF16, BF16), (BF16, F16), (F16, F16))                       # (gradients, activations)


def backward_forms(keys, n_q, causal, prec, act_prec):
    """attention_bwd.hip launch: the dQ and the dK/dV instantiation, or None where the entry point refuses."""
    if causal and (prec != act_prec or keys > 320 or n_q > 288):
        return None
    tag = f"{PREC_NAME[prec]},{PREC_NAME[act_prec]},{'causal' if causal else 'full'}"
    kt, qt2 = (keys + 15) // 16, ((n_q + 15) // 16 + 1) // 2 * 2
    dq = "dq_stream" if not causal and kt > 20 else f"dq{next(N for N in (2, 6, 14, 20) if kt <= N)}"
    dkv = "dkv_stream" if not causal and qt2 > 18 else f"dkv{next(N for N in (2, 6, 14, 18) if qt2 <= N)}"
    return f"{dq}<{tag}>", f"{dkv}<{tag}>"


def backward_forms_all():
    forms = set()
    for prec, act in BWD_PRECS + ((F16, F16), (BF16, BF16)):
        for causal in (False, True):
            if causal and prec != act:
                continue
            tag = f"{PREC_NAME[prec]},{PREC_NAME[act]},{'causal' if causal else 'full'}"
            forms |= {f"dq{N}<{tag}>" for N in (2, 6, 14, 20)} | {f"dkv{N}<{tag}>" for N in (2, 6, 14, 18)}
            if not causal:
                forms |= {f"dq_stream<{tag}>", f"dkv_stream<{tag}>"}
    return forms


# ---------------------------------------------------------------------------------------------------------------------
# the GPU tests' tables (test_gpu_attention_edges.py parametrises over them, test_attention_ref_host.py checks them)
FWD_PLAIN = [plain(3, L, heads=3 if L in (17, 97, 305) else 2) for L in (1, 16, 17, 32, 33, 96, 97, 224, 225, 304, 305, 320, 321)]
FWD_CAUSAL = [plain(3, L, heads=3 if L in (17, 97) else 2, causal=True) for L in (1, 2, 17, 32, 33, 96, 97, 224, 225, 320)]
# few queries in their own buffer, prompt rows: 214 keys (ViT-B/16 at T = 8) and 298 (ViT-L/14 at T = 32), here with T = 4
FWD_FEW = ([vision(4, 4, 8, 201, n_q=nq, qbr=201) for nq in (1, 15, 17, 63, 64, 65)] +
           [vision(4, 4, 8, 285, n_q=nq, qbr=285) for nq in (1, 15, 17, 63, 64, 65)])
FWD_CLS = [vision(4, 4, 8, 201, n_q=1, qbr=1), vision(4, 4, 8, 209, n_q=1, qbr=1), vision(4, 4, 8, 285, n_q=1, qbr=1),
           vision(4, 2, 8, 309, n_q=1, qbr=1)]                       # 214, 222, 298, 320 keys
FWD_VISION = [vision(4, 2, 0, 29), vision(4, 2, 1, 29), vision(4, 4, 8, 83), vision(4, 4, 8, 84, heads=3), vision(4, 2, 8, 213),
              vision(4, 2, 8, 214), vision(4, 1, 0, 303), vision(22, 11, 8, 300), vision(24, 12, 8, 300),
              vision(4, 4, 8, 257), vision(8, 4, 8, 257)]
FWD_EXTRA = [vision(4, 2, 8, 215, has_summary=False),               # 225 keys without a summary row
             vision(4, 4, 8, 84, split=True), vision(4, 1, 0, 303, split=True)]   # split_out at 97 and 305 keys
FWD_ALL = FWD_PLAIN + FWD_CAUSAL + FWD_FEW + FWD_CLS + FWD_VISION + FWD_EXTRA

BWD_CAUSAL = [plain(2, n, causal=True) for n in (1, 17, 33, 96, 97, 224, 225, 288)]
BWD_PLAIN = [plain(2, n, heads=3 if n == 97 else 2) for n in (32, 33, 96, 97, 224, 225, 288, 289, 320, 321)]
BWD_VISION = [vision(4, 2, 0, 29), vision(4, 2, 1, 29), vision(4, 2, 8, 213), vision(4, 2, 8, 214), vision(22, 11, 8, 300),
              vision(24, 12, 8, 300)]                                # 32, 33, 224, 225, 320, 321 keys
BWD_CLS = [vision(4, 4, 8, 209, n_q=1, qbr=1), vision(4, 2, 8, 309, n_q=1, qbr=1)]   # 222 and 320 keys
BWD_EXTRA = [vision(4, 2, 8, 215, has_summary=False)]
BWD_ALL = BWD_CAUSAL + BWD_PLAIN + BWD_VISION + BWD_CLS + BWD_EXTRA


def _edge(c, keys):
    return n_keys(c) in keys and not c.split          # the CLS-only shapes (own query buffer) at a class edge included


def forward_regimes(c):
    """randn everywhere; the other six on the class edges 33 | 225 | 320 | 321 keys and on the 257-query shapes; hot_side only
    with prompt rows."""
    if not (_edge(c, (33, 225, 320, 321)) or (c.side and c.n == 257 and not c.qbr)):
        return ["randn"]
    return [r for r in REGIMES if r != "hot_side" or (c.side and c.G + 2 * c.BT <= 64)]


# fp16 gradients with `peaked` can underflow dS; the emulation stays within its share of the plain relative bound on every such
# case (at most 1.65 of 3: test_attention_ref_host.py::test_backward_emulation_within_its_share), so the pair stays in
# One pair is dropped, on the emulation's word: `peaked` with fp16 gradients on the CLS-only shapes.  With ONE query per frame
# a near one-hot row leaves whole prompt-row groups below what fp16 P and dS can carry (dside all zero against a reference
# of 1e-9), so no relative bound holds.  Every other regime and precision on those shapes is within its share (worst 1.55
# of 3; `peaked` in bf16 1.40) and stays in.
def backward_regimes(c):
    if not c.has_summary and c.side or not _edge(c, (33, 97, 225, 288, 320, 321)):
        return ["randn"]
    return [r for r in REGIMES if r != "hot_side" or (c.side and c.G + 2 * c.BT <= 64)]


def backward_dropped(c, regime, prec):
    return bool(c.qbr) and regime == "peaked" and prec == F16


def forward_params():
    return [(c, r, p) for c in FWD_ALL for r in forward_regimes(c) for p in (F16, BF16)]


def backward_params():
    return [(c, r, p, a) for c in BWD_ALL for r in backward_regimes(c) for p, a in BWD_PRECS
            if not (c.causal and p != a) and not backward_dropped(c, r, p)]


def seed_of(c, regime):
    return 1000 * n_keys(c) + 10 * c.BT + REGIMES.index(regime)
