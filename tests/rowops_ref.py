"""Reference side of the row-kernel edge tests (test_rowops_ref_host.py, test_gpu_rowops_edges.py); nothing here touches a
GPU.  The kernels: gava_layernorm, gava_convert_h16, gava_row_stats, gava_similarity_head (csrc/rowops.hip),
gava_layernorm_backward and gava_qgelu_backward (csrc/backward.hip).

  * the value regimes and the case tables of the GPU tests;
  * fp64 references computed from the operands the kernel really receives (fp32 rows, 16-bit values widened; the fp32
    partial sums for row_stats), with optional MUTATIONS - the bugs the bounds must catch;
  * the per-element bounds (no whole-tensor norm or maximum anywhere);
  * emulate_*: fp32 restatements of the kernels' rounding points - float4-per-lane partial sums, the 64-lane xor butterfly,
    two passes, 1 / sqrt, the packed 16-bit conversions - written from the kernels' structure, never calling the library.

u = 2^-24; eps16 = 2^-11 (fp16) / 2^-8 (bf16): the largest relative error of one rounding to that type.  Every ratio below is
|got - ref| / bound per element, and <= 1 passes.

The bounds
  LayerNorm forward, fp32 result   C_LN u [ (|mean| rstd + 2 |xhat|) |gamma| + |beta| ].
      The rounded mean (a sum of D terms of size about |mean|, then a division) is off by a few u |mean|; x - mean carries that
      into every element, times rstd |gamma|: the first term.  rstd comes out of a sum of squares, a division, an add, a square
      root and a division: a few u, relative, on xhat; two more roundings in xhat = d * rstd and xhat * gamma: the second term.
      The add of beta rounds the result, |y| <= |xhat gamma| + |beta|: the third.
  second LayerNorm (gamma2)        the same form on the first one's result y1, plus the first one's error e_j <= b1_j carried
      through d y2_i / d y1_j = rstd2 gamma2_i (delta_ij - 1/D - xhat2_i xhat2_j / D):
      rstd2 |gamma2_i| [ b1_i + mean_j b1_j + |xhat2_i| mean_j (b1_j |xhat2_j|) ].
  16-bit copies                    where the fp32 result is also stored (and is the same LayerNorm): h16(out32) bit for bit.
      Otherwise the fp32 bound b, plus one rounding of a value within b of ref: eps16 (|ref| + b), and FLOOR16 (half the
      smallest subnormal) where the result is below the normal range.
  pair (out_hi / out_lo)           hi as a 16-bit copy; r = y - hi is exact in fp32 and |r| <= eps16 |y|; lo = fp16(r) whatever
      the operand type: |hi + lo - y| <= max(eps16 2^-11 |y|, 2^-25) - 2^-22 |y| for fp16 operands, 2^-19 |y| for bf16.
      split_out rows [hi | lo | hi] round lo in the operand type: max(eps16^2 |y|, FLOOR16).
  LayerNorm backward, dx           C_LNB u rstd [ |g| + |mean g| + |xhat| |mean(g xhat)| + |mean| rstd (|mean(g xhat)| + |xhat| mean|g|) ],
      g = dy gamma.  The first three are the terms of dx = rstd (g - mean g - xhat mean(g xhat)), each rounded; the last is the
      forward form's d_xhat = u |mean| rstd reaching dx through xhat mean(g xhat), once through the factor and once through
      the mean.  accumulate: one more rounding of the sum, u (|base + ref| + bound).  dx16 = h16(dx) bit for bit.
      The error of a rounded mean is u times the mean of the MAGNITUDES, not of the values: where g_i is small and mean g
      cancels (every regime has such elements; `tiny` and `const`, where xhat adds nothing, most of all) the form above is
      small for no reason of the kernel's, and the emulation reaches 79 times it: C_LNB = 256.  So dx is held to a second
      form as well, with mean|g| and mean|g xhat| in place of |mean g| and |mean(g xhat)|, whose constant comes out at
      C_LNB_SUMS = 8 (worst emulated ratio 3.9); it is the one that catches a subtly wrong kernel, and both are asserted.
      dgamma, dbeta                atomic sums over the rows in any order: C_ACC u (|start| + sum_rows |dy| (|xhat| + |mean| rstd))
      and C_ACC u (|start| + sum_rows |dy|) (the second term of dgamma is d_xhat again: dy * xhat inherits it).
  QuickGELU backward               eps16 |ref| + FLOOR16 (the final rounding) + |dh| (C_QG u T + 2^-126 (1 + |a|)), a = 1.702 x,
      s = sigmoid(a), ref = dh s (1 + a (1 - s)), T = |1 + a (1 - 2 s)| (2 (1 + |a|) s (1 - s) + 2 s) + 4 (s + |a| s (1 - s)).
      __expf(-a) = exp2(fl(fl(-1.702 x) log2 e)) is off by an ulp of its own and by the two roundings of its argument:
      relative (1 + |a|) 2^-23, which reaches s = 1 / (1 + e) times (1 - s); the add and the division round s itself, 2 u s.
      Both reach the derivative through d/ds [s + a s (1 - s)] = 1 + a (1 - 2 s): the first part of T (for large positive x
      it is the rounding of s next to 1 that 1 - s then multiplies by a).  The four operations of
      s * (1 + 1.702 x (1 - s)) each round something no larger than s + |a| s (1 - s): the second part, which does not vanish
      where the derivative changes sign (x ~ -0.75).  Where exp overflows fp32 (a < -88.7) or 1 / (1 + e) is an fp32 subnormal
      the kernel's s is 0 and the truth is below 2^-126 (1 + |a|): the last term.
  convert_h16                      the bits of torch's CPU conversion (round to nearest even); NaN -> NaN.
  row_stats                        |d mean| <= C_RS u sum|s1| / D;  |d var| <= C_RS u (sum|s2| / D + mean^2 + eps);
      |d rstd| <= rstd^3 |d var| / 2 + u rstd.  eps counts among the terms of the variance: the add var + eps rounds, the
      square root takes its share, and 1e-5f is not 1e-5 - where eps dominates (`tiny`, `const`) the fp32 emulation is 1.7 u rstd
      off, which u rstd alone does not hold.  The kernel computes E[x^2] - mean^2: on a large common offset the bound on rstd
      is loose by construction, and stays so.
  similarity_head                  worst-case rounding counts, no fitted constant: see similarity_bounds().

The constants C_LN, C_LNB, C_LNB_SUMS, C_ACC, C_RS, C_QG: each is the smallest power of two that is at least twice the worst
ratio the emulation reaches against the form with C = 1 over the whole table of its family
(test_rowops_ref_host.py::test_constants_are_the_smallest_powers_of_two asserts both sides of that: the emulation stays
within half of every such bound, and above a quarter of it somewhere).  C_QG is set on the fp32 value in front of the final
rounding.  The 16-bit roundings themselves (eps16 |ref|, the pair's and the split's lo) are no fitted constants: a correct
rounding reaches them, so the emulation is only required to stay within them.  What the GPU reaches is recorded in
profiles/rowops_edges_errors.txt and sets nothing.
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

F16, BF16 = 0, 1                                  # hip.PREC_F16 / hip.PREC_BF16
DTYPE = {F16: torch.float16, BF16: torch.bfloat16}
EPS = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
FLOOR16 = {F16: 2.0 ** -25, BF16: 2.0 ** -134}    # half the smallest subnormal
PREC_NAME = {F16: "f16", BF16: "bf16"}
PRECS = (F16, BF16)
U = 2.0 ** -24
LN_EPS = 1e-5
F32, F64 = torch.float32, torch.float64
INF = math.inf

C_LN, C_LNB, C_LNB_SUMS, C_ACC, C_RS, C_QG = 8.0, 256.0, 8.0, 16.0, 16.0, 2.0
# the checks (names as the *_ratios functions give them) that each constant governs
GOVERNS = {"C_LN": ("ln", ("out32",)), "C_LNB": ("lnb", ("dx",)), "C_LNB_SUMS": ("lnb", ("dx (sums)",)),
           "C_ACC": ("lnb", ("dgamma", "dbeta")), "C_RS": ("rs", ("mean", "rstd")), "C_QG": ("qg", ("fp32",))}
CONSTANTS = {"C_LN": C_LN, "C_LNB": C_LNB, "C_LNB_SUMS": C_LNB_SUMS, "C_ACC": C_ACC, "C_RS": C_RS, "C_QG": C_QG}

REGIMES = ("randn", "offset", "const", "tiny", "big", "outlier")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_rows(regime, rows, D, g):
    """fp64 from the seeded generator, stored as fp32."""
    z = torch.randn(rows, D, generator=g, dtype=F64)
    if regime == "randn":
        x = z * 3 + 1.5
    elif regime == "offset":                      # tells two-pass statistics from E[x^2] - mean^2
        x = 1000 + z
    elif regime == "const":                       # mean exact, variance 0: xhat = 0, rstd = 1 / sqrt(eps)
        x = torch.full_like(z, 7.25)
    elif regime == "tiny":                        # variance 1e-8 << eps
        x = 1e-4 * z
    elif regime == "big":                         # squares reach 1e9, the sums stay finite
        x = 3e4 * z
    elif regime == "outlier":
        x = z
        x[:, D // 3] = 500
    else:
        raise ValueError(regime)
    return x.float()


def make_affine(D, g):
    return (1 + 0.2 * torch.randn(D, generator=g, dtype=F64)).float(), (0.2 * torch.randn(D, generator=g, dtype=F64)).float()


def ratio(err, bound):
    """max over the elements of err / bound; an element with a zero bound must match exactly."""
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, INF, 0.0))
    return float(r.max())


def same_bits(a, b):
    """0 when two 16-bit tensors hold the same bits, inf otherwise (a ratio, like every other check)."""
    return 0.0 if a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)) else INF


def copy16_bound(ref, b, prec):
    return b + EPS[prec] * (ref.abs() + b) + FLOOR16[prec]


def pair_bound(y, prec):
    return torch.clamp(EPS[prec] * 2.0 ** -11 * y.abs(), min=2.0 ** -25)


def split_bound(y, prec):
    return torch.clamp(EPS[prec] ** 2 * y.abs(), min=FLOOR16[prec])


# ---------------------------------------------------------------------------------------------------------------------
# the wave: lane l holds float4 i at columns 4 (l + 64 i) .. + 3, active while that is below D
def lane_sum(t):
    """fp32 [rows][D] -> [rows][1]: per lane s += (x + y) + (z + w) over its active float4, then the xor butterfly 32 .. 1.
    (Adding the zeros of the inactive float4 is exact, and after a butterfly of commutative adds every lane holds the same
    bits.)"""
    rows, D = t.shape
    p = torch.zeros(rows, 1024, dtype=F32)
    p[:, :D] = t
    v = p.view(rows, 4, 64, 4)
    s = torch.zeros(rows, 64, dtype=F32)
    for i in range(4):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def act_pattern(D):
    """(float4 groups the row reaches, whether the last one is partly active): the act[] pattern of lane 0 and whether some
    lane's differs."""
    return -(-D // 256), D % 256 != 0


LN_MUTATIONS = ("eps6", "d_minus_1", "single_pass", "gamma_shift", "beta_drop_last", "stale_lane", "ln2_unaffined", "pair_lo_optype")
LNB_MUTATIONS = ("no_xhat_term", "mean_over_1024")


def _ln(x, gamma, beta, emulate, mutate=None):
    """One LayerNorm -> (y, xhat): fp64, or the kernel's fp32 order when `emulate`."""
    D = x.shape[1]
    eps = 1e-6 if mutate == "eps6" else LN_EPS
    div = D - 1 if mutate == "d_minus_1" else D
    if emulate:
        x = x.float()
        total = lane_sum(x)
    else:
        x = x.double()
        total = x.sum(1, keepdim=True)
    if mutate == "stale_lane" and D % 256:        # the inactive lanes of the last group add what they hold from the group before
        last = D // 256 * 256
        if last:
            total = total + x[:, last - 256 + D % 256:last].sum(1, keepdim=True)
        else:
            total = total + 1.0                   # (a single group: whatever the registers held)
    mean = total / float(D)
    if mutate == "single_pass":                   # E[x^2] - mean^2 in fp32
        x32 = x.float()
        m32 = x32.sum(1, keepdim=True) / float(D)
        var = ((x32 * x32).sum(1, keepdim=True) / float(D) - m32 * m32).clamp(min=0).to(x.dtype)
        d = x - mean
    else:
        d = x - mean
        var = (lane_sum(d * d) if emulate else (d * d).sum(1, keepdim=True)) / float(div)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=x.dtype))
    xh = d * rstd
    if gamma is None:
        return xh, xh
    gm, bt = gamma.to(x.dtype), beta.to(x.dtype)
    if mutate == "gamma_shift":
        gm = gm.roll(1)
    if mutate == "beta_drop_last":
        bt = bt.clone()
        bt[(D - 1) // 256 * 256:] = 0
    return xh * gm + bt, xh


def _ln_terms(x, gamma, beta):
    """fp64 (y, bound with C = 1, xhat, rstd, mean) of one LayerNorm."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
    xh = d * rstd
    g, b = gamma.double(), beta.double()
    return xh * g + b, U * ((mean.abs() * rstd + 2 * xh.abs()) * g.abs() + b.abs()), xh, rstd, mean


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward: forms and table
Form = namedtuple("Form", "out32 out16 split pair g2 cast alias gather pad16", defaults=(False,) * 8 + (8,))
LN_FORMS = {
    "out32": Form(out32=True),
    "out16": Form(out16=True),
    "both": Form(out32=True, out16=True),
    "alias": Form(out32=True, alias=True),                            # out32 is the input buffer
    "split": Form(out32=True, out16=True, split=True, pad16=0),       # rows [hi | lo | hi], out16 stride 3 D exactly
    "split_pad": Form(out16=True, split=True),                        # stride 3 D + 8, no fp32 copy
    "pair": Form(pair=True),
    "g2_out32": Form(out32=True, out16=True, g2=True),
    "g2_pair": Form(out16=True, pair=True, g2=True),
    "g2_both": Form(out32=True, out16=True, pair=True, g2=True),
    "cast16": Form(out16=True, cast=True),
    "cast_split": Form(out16=True, split=True, cast=True),
    "cast_pair": Form(pair=True, cast=True),
    "gather": Form(out32=True, out16=True, gather=True),
}
LN_WIDTHS = (4, 8, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024)
LN_ROWS = (1, 3, 4, 5, 9)                                             # the workgroup is 4 rows
LnCase = namedtuple("LnCase", "form D rows regime prec")


def ln_forward_cases():
    out = []
    for prec in PRECS:
        base = [("both", D, "randn") for D in LN_WIDTHS]
        base += [(f, D, "randn") for D in (260, 768, 1020) for f in LN_FORMS]
        base += [(f, D, r) for D in (4, 260, 1024) for f in ("both", "pair", "g2_both") for r in REGIMES]
        seen = set()
        for form, D, regime in base:
            if (form, D, regime) in seen:
                continue
            seen.add((form, D, regime))
            out.append(LnCase(form, D, LN_ROWS[len(seen) % len(LN_ROWS)], regime, prec))
    return out


def ln_case_id(c):
    return f"{c.form}-D{c.D}-r{c.rows}-{c.regime}-{PREC_NAME[c.prec]}"


def case_seed(c):
    return int.from_bytes(repr(tuple(c)).encode(), "little") % (2 ** 31 - 1)


def ln_forward_inputs(c):
    """x: the rows the kernel works on, in order (the GPU test lays them out: views into NaN-padded buffers, the gather's source
    and index)."""
    g = gen(case_seed(c))
    f = LN_FORMS[c.form]
    x = make_rows(c.regime, c.rows, c.D, g)
    inp = SimpleNamespace(x=x, gamma=None, beta=None, gamma2=None, beta2=None, src=None, index=None)
    if not f.cast:
        inp.gamma, inp.beta = make_affine(c.D, g)
    if f.g2:
        inp.gamma2, inp.beta2 = make_affine(c.D, g)
    if f.gather:                                                      # repeats, out of a source with more rows
        inp.src = make_rows(c.regime, c.rows + 4, c.D, g)
        inp.index = torch.randint(0, c.rows + 4, (c.rows,), generator=g, dtype=torch.int32)
        if c.rows > 1:
            inp.index[-1] = inp.index[0]
        inp.x = inp.src[inp.index.long()]
    return inp


def ln_forward_model(c, inp, emulate, mutate=None):
    """What the kernel leaves: {out32: fp32, out16: h16 [rows][D or 3 D], hi: h16, lo: fp16}.  fp64 arithmetic rounded once
    at the stores, or the kernel's own fp32 order when `emulate`."""
    f, P = LN_FORMS[c.form], DTYPE[c.prec]
    first = ("eps6", "d_minus_1", "single_pass", "gamma_shift", "beta_drop_last", "stale_lane")
    if f.cast:
        y1 = xh1 = inp.x.double()
    else:
        y1, xh1 = _ln(inp.x, inp.gamma, inp.beta, emulate, mutate if mutate in first else None)
    main = y1
    if f.g2:
        fed = xh1 if mutate == "ln2_unaffined" else y1
        main, _ = _ln(fed.float() if emulate else fed, inp.gamma2, inp.beta2, emulate)
    y1, main = y1.float(), main.float()
    out = {}
    if f.out32:
        out["out32"] = y1
    if f.out16:
        hi = main.to(P)
        out["out16"] = torch.cat([hi, (main - hi.float()).to(P), hi], 1) if f.split else hi
    if f.pair:
        hi = y1.to(P)
        r = y1 - hi.float()
        out["hi"], out["lo"] = hi, (r.to(P).to(torch.float16) if mutate == "pair_lo_optype" else r.to(torch.float16))
    return out


def ln_forward_ratios(c, inp, got):
    """{check name: ratio}; <= 1 passes.  `got` as ln_forward_model returns it."""
    f, P, D = LN_FORMS[c.form], DTYPE[c.prec], c.D
    res = {}
    if f.cast:                                    # the values themselves: every bit is determined
        hi = inp.x.to(P)
        r = inp.x - hi.float()
        if f.pair:
            res["hi bits"], res["lo bits"] = same_bits(got["hi"], hi), same_bits(got["lo"], r.to(torch.float16))
        elif f.split:
            res["out16 bits"] = same_bits(got["out16"], torch.cat([hi, r.to(P), hi], 1))
        else:
            res["out16 bits"] = same_bits(got["out16"], hi)
        return res
    y1, b1, _, _, _ = _ln_terms(inp.x, inp.gamma, inp.beta)
    b1 = C_LN * b1
    main, bm = y1, b1
    if f.g2:
        main, b2, xh2, rstd2, _ = _ln_terms(y1, inp.gamma2, inp.beta2)
        carried = rstd2 * inp.gamma2.double().abs() * (b1 + b1.mean(1, keepdim=True) + xh2.abs() * (b1 * xh2.abs()).mean(1, keepdim=True))
        bm = C_LN * b2 + carried
    y32 = None
    if f.out32:
        y32 = got["out32"].double()
        res["out32"] = ratio((y32 - y1).abs(), b1)
        if c.regime == "const":                   # xhat = 0 exactly: beta comes through bit for bit
            res["out32 is beta"] = 0.0 if torch.equal(got["out32"], inp.beta.expand(c.rows, D)) else INF
    known = y32 is not None and not f.g2          # the fp32 value the 16-bit copies were rounded from is in out32
    if f.out16:
        o = got["out16"]
        hi = o[:, :D]
        if known:
            res["out16 bits"] = same_bits(hi, got["out32"].to(P))
        else:
            res["out16"] = ratio((hi.double() - main).abs(), copy16_bound(main, bm, c.prec))
        if f.split:
            res["split hi twice"] = same_bits(hi, o[:, 2 * D:])
            s = hi.double() + o[:, D:2 * D].double()
            if known:
                res["split sum"] = ratio((s - y32).abs(), split_bound(y32, c.prec))
            else:
                res["split sum"] = ratio((s - main).abs(), bm + split_bound(main.abs() + bm, c.prec))
    if f.pair:
        s = got["hi"].double() + got["lo"].double()
        if y32 is not None:
            res["pair hi bits"] = same_bits(got["hi"], got["out32"].to(P))
            res["pair sum"] = ratio((s - y32).abs(), pair_bound(y32, c.prec))
        else:
            res["pair hi"] = ratio((got["hi"].double() - y1).abs(), copy16_bound(y1, b1, c.prec))
            res["pair sum"] = ratio((s - y1).abs(), b1 + pair_bound(y1.abs() + b1, c.prec))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
LNB_FORMS = ("plain", "accumulate", "dx16_f16", "dx16_bf16", "dgamma_1row", "dgamma_70rows", "gather")
LNB_WIDTHS = (4, 260, 1020, 1024)
LnbCase = namedtuple("LnbCase", "form D rows regime")


def ln_backward_cases():
    out = [LnbCase(f, D, {"dgamma_1row": 1, "dgamma_70rows": 70}.get(f, 5), r) for D in LNB_WIDTHS for r in REGIMES for f in LNB_FORMS]
    return out + [LnbCase("dy_wide", D, 5, "randn") for D in LNB_WIDTHS]   # dy over six orders of magnitude per row


def lnb_case_id(c):
    return f"{c.form}-D{c.D}-r{c.rows}-{c.regime}"


def ln_backward_inputs(c):
    g = gen(case_seed(c))
    x = make_rows(c.regime, c.rows, c.D, g)
    gamma, _ = make_affine(c.D, g)
    dy = torch.randn(c.rows, c.D, generator=g, dtype=F64)
    if c.form == "dy_wide":
        dy = dy * torch.pow(10.0, torch.rand(c.rows, c.D, generator=g, dtype=F64) * 6 - 3)
    inp = SimpleNamespace(x=x, gamma=gamma, dy=dy.float(), base=None, g0=None, b0=None, src=None, index=None)
    if c.form == "accumulate":
        inp.base = (2 * torch.randn(c.rows, c.D, generator=g, dtype=F64)).float()
    if c.form.startswith("dgamma"):                                   # the atomics start from known finite values
        inp.g0, inp.b0 = make_affine(c.D, g)
    if c.form == "gather":                                            # x gathered, dx scattered: distinct rows of a larger matrix
        inp.src = make_rows(c.regime, c.rows + 4, c.D, g)
        inp.index = torch.randperm(c.rows + 4, generator=g)[:c.rows].to(torch.int32)
        inp.x = inp.src[inp.index.long()]
    return inp


def lnb_prec(c):
    return F16 if c.form == "dx16_f16" else BF16


def ln_backward_model(c, inp, emulate, mutate=None):
    """{dx: fp32 (with the base when accumulating), dx16, dgamma, dbeta}."""
    D = c.D
    dt = F32 if emulate else F64
    x = inp.x.to(dt)
    ssum = lane_sum if emulate else (lambda t: t.sum(1, keepdim=True))
    inv = torch.tensor(1.0, dtype=dt) / float(D)                      # the backward multiplies by 1 / D where the forward divides
    d = x - ssum(x) * inv
    rstd = 1.0 / torch.sqrt(ssum(d * d) * inv + torch.tensor(LN_EPS, dtype=dt))
    xh = d * rstd
    dy = inp.dy.to(dt)
    g = inp.gamma.to(dt) * dy
    inv_g = torch.tensor(1.0 / 1024, dtype=dt) if mutate == "mean_over_1024" else inv
    mg, mgx = ssum(g) * inv_g, ssum(g * xh) * inv
    dx = rstd * (g - mg) if mutate == "no_xhat_term" else rstd * (g - mg - xh * mgx)
    if inp.base is not None:
        dx = dx + inp.base.to(dt)
    out = {"dx": dx.float()}
    if c.form.startswith("dx16"):
        out["dx16"] = out["dx"].to(DTYPE[lnb_prec(c)])
    if inp.g0 is not None:
        if emulate:                                                   # one of the orders the atomics can take: row by row
            dg, db = inp.g0.clone(), inp.b0.clone()
            for r in range(c.rows):
                dg, db = dg + dy[r] * xh[r], db + dy[r]
        else:
            dg, db = inp.g0.double() + (dy * xh).sum(0), inp.b0.double() + dy.sum(0)
        out["dgamma"], out["dbeta"] = dg.float(), db.float()
    return out


def ln_backward_ratios(c, inp, got):
    x = inp.x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
    xh = d * rstd
    dy = inp.dy.double()
    g = dy * inp.gamma.double()
    mg, mgx = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ref = rstd * (g - mg - xh * mgx)
    dxh = mean.abs() * rstd                                           # d_xhat / u
    ag, agx = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
    b = C_LNB * U * rstd * (g.abs() + mg.abs() + xh.abs() * mgx.abs() + dxh * (mgx.abs() + xh.abs() * ag))
    bs = C_LNB_SUMS * U * rstd * (g.abs() + ag + xh.abs() * agx + dxh * (agx + xh.abs() * ag))
    if inp.base is not None:
        ref = ref + inp.base.double()
        b, bs = b + U * (ref.abs() + b), bs + U * (ref.abs() + bs)
    err = (got["dx"].double() - ref).abs()
    # (accumulated: the rounding of the last add is no fitted constant and a correct kernel reaches it - a check of its own name)
    acc = " accumulated" if inp.base is not None else ""
    res = {"dx" + acc: ratio(err, b), "dx (sums)" + acc: ratio(err, bs)}
    if "dx16" in got:
        res["dx16 bits"] = same_bits(got["dx16"], got["dx"].to(DTYPE[lnb_prec(c)]))
    if inp.g0 is not None:
        rg, rb = inp.g0.double() + (dy * xh).sum(0), inp.b0.double() + dy.sum(0)
        bg = C_ACC * U * (inp.g0.double().abs() + (dy.abs() * (xh.abs() + dxh)).sum(0))
        bb = C_ACC * U * (inp.b0.double().abs() + dy.abs().sum(0))
        res["dgamma"], res["dbeta"] = ratio((got["dgamma"].double() - rg).abs(), bg), ratio((got["dbeta"].double() - rb).abs(), bb)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# QuickGELU backward
QG_SIZES = (4, 1020, 8192 * 256 * 4 + 4)          # the last: one more trip of the grid-stride loop (8192 blocks of 256 x 4 values)
QG_MUTATIONS = ("no_1702",)


def qgelu_cases():
    return [(n, p) for p in PRECS for n in QG_SIZES]


def qgelu_inputs(n, prec):
    """(pre, dh) as 16-bit tensors.  Pre-activations (the qgelu_tails idea of gemm_ref.py): a dense ramp over [-20, 20] across
    the derivative's sign change, exact zeros of either sign, bf16: |x| up to 1e4 (exp(1.702 |x|) overflows fp32 from 52 on),
    fp16: subnormals."""
    g = gen(7 * n + prec)
    a = torch.randn(n, generator=g) * 2 + 0.3
    m = a[::5].numel()
    a[::5] = torch.linspace(-20.0, 20.0, m) if m > 1 else -0.75
    a[2::13] = 0.0
    a[3::13] = -0.0
    k = a[4::17].numel()
    if k:
        sign = 1 - 2 * (torch.arange(k) % 2).float()
        if prec == BF16:
            a[4::17] = sign * torch.logspace(math.log10(30.0), 4.0, k)
        else:
            a[4::17] = sign * ((torch.arange(k) * 37) % 1023 + 1).float() * 2.0 ** -24
    if n == 4:
        a = torch.tensor([-0.75, 0.0, -0.0, 20.0])
    dh = torch.randn(n, generator=g)
    return a.to(DTYPE[prec]), dh.to(DTYPE[prec])


def qgelu_backward_model(pre, dh, prec, emulate, mutate=None, rounded=True):
    """rounded=False: the fp32 value in front of the final 16-bit rounding (what C_QG is set from)."""
    if emulate:
        x, d = pre.float(), dh.float()
        e = torch.exp2((-1.702 * x) * 1.4426950408889634)             # __expf: v_exp_f32 of the argument times log2 e
        s = 1.0 / (1.0 + e)
        out = d * (s * (1.0 + (1.702 * x) * (1.0 - s)))
    else:
        x, d = pre.double(), dh.double()
        s = torch.sigmoid(1.702 * x)
        k = 1.0 if mutate == "no_1702" else 1.702
        out = (d * s * (1 + k * x * (1 - s))).float()
    return out.to(DTYPE[prec]) if rounded else out


def qgelu_backward_ratio(pre, dh, got, prec, rounded=True):
    x, d = pre.double(), dh.double()
    a = 1.702 * x
    s = torch.sigmoid(a)
    ref = d * s * (1 + a * (1 - s))
    T = (1 + a * (1 - 2 * s)).abs() * (2 * (1 + a.abs()) * s * (1 - s) + 2 * s) + 4 * (s + a.abs() * s * (1 - s))
    b = d.abs() * (C_QG * U * T + 2.0 ** -126 * (1 + a.abs()))
    if rounded:
        b = b + EPS[prec] * (ref.abs() + b) + FLOOR16[prec]
    return ratio((got.double() - ref).abs(), b)


# ---------------------------------------------------------------------------------------------------------------------
# convert_h16
CVT_SIZES = (1, 255, 257, 4096 * 256 + 259)       # the last: past the grid cap of 4096 blocks, n % 256 != 0
CVT_MUTATIONS = ("truncate", "ties_away")
CVT_EXPONENTS = {F16: (0, 1, 2, 14, 15, 16, 29, 30), BF16: (0, 1, 2, 126, 127, 128, 253, 254)}   # 0: the subnormal range, 1: the lowest normal


def _next(t, step):
    """fp32 -> the fp32 `step` units in the last place further from zero (no zeros, infs or NaNs in t)."""
    return (t.view(torch.int32) + step).view(F32)


def convert_values(prec):
    """fp32: every 16-bit pattern widened (NaNs included); every exact tie between neighbouring 16-bit values over
    CVT_EXPONENTS with the fp32 on either side of it, both signs; the fp16 overflow edge; zeros, infs, NaN."""
    P = DTYPE[prec]
    allp = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(P).float()
    mant = 1 << (10 if prec == F16 else 7)
    pat = torch.cat([torch.arange(e * mant, (e + 1) * mant, dtype=torch.int32) for e in CVT_EXPONENTS[prec]]).to(torch.int16)
    lo, hi = pat.view(P).double(), (pat + 1).view(P).double()         # neighbours (the top mantissa's neighbour: the next exponent)
    lo, hi = lo[torch.isfinite(hi)], hi[torch.isfinite(hi)]           # (the largest finite value's neighbour is inf: the edge below)
    tie = ((lo + hi) / 2).float()                                     # one more bit than the 16-bit type: exact in fp32, subnormals too
    assert torch.equal(tie.double(), (lo + hi) / 2) and torch.isfinite(tie).all()
    ties = torch.cat([tie, _next(tie, 1), _next(tie, -1)])
    # the overflow tie: the largest finite value and the midpoint between it and the next power of two (fp16: 65504, 65520;
    # bf16: the fp32 patterns 0x7f7f0000, 0x7f7f8000, finite in fp32), which rounds to even = inf
    edge = torch.tensor([65504.0, 65520.0])                           # (plain data for bf16)
    if prec == BF16:
        edge = torch.cat([edge, torch.tensor([0x7f7f0000, 0x7f7f8000], dtype=torch.int32).view(F32)])
    edge = torch.cat([edge, _next(edge, 1), _next(edge, -1)])
    special = torch.tensor([0.0, -0.0, INF, -INF, math.nan])
    return torch.cat([special, edge, -edge, ties, -ties, allp])


def convert_input(n, prec):
    v = convert_values(prec)
    if n >= v.numel():
        return v.repeat(-(-n // v.numel()))[:n].contiguous()
    pick = torch.randperm(v.numel(), generator=gen(n))[:n]
    pick[0] = 5 + (n % 12)                                            # always one of the overflow edges
    return v[pick].contiguous()


def convert_model(x, prec, mutate=None):
    P = DTYPE[prec]
    if mutate is None:
        return x.to(P)
    if mutate == "truncate":                                          # toward zero
        r = x.to(P)
        over = r.float().abs() > x.abs()
        return torch.where(over & torch.isfinite(x), (r.view(torch.int16) - 1).view(P), r)
    if mutate == "ties_away":
        r = x.to(P)
        down = (r.view(torch.int16) + 1).view(P)                      # the neighbour further from zero
        tie = (x.double() - r.double()).abs() == (down.double() - x.double()).abs()
        return torch.where(tie & torch.isfinite(x) & torch.isfinite(r.float()) & (r.float().abs() < x.abs()), down, r)
    raise ValueError(mutate)


def convert_check(x, got, prec):
    """0 / inf: the bits of torch's CPU conversion wherever the input is no NaN, a NaN where it is."""
    want = x.to(DTYPE[prec])
    nan = torch.isnan(x)
    if not torch.isnan(got.float()[nan]).all():
        return INF
    return same_bits(got[~nan], want[~nan])


# ---------------------------------------------------------------------------------------------------------------------
# row_stats
RS_SLOTS, RS_ROWS = (1, 3, 4, 12, 16, 32), (1, 63, 64, 65, 130)
RsCase = namedtuple("RsCase", "slots rows D kind", defaults=("rows",))
RS_MUTATIONS = ("no_clamp", "next_slot")


def row_stats_cases():
    out = [RsCase(s, r, 64 * s) for s in RS_SLOTS for r in RS_ROWS]
    return out + [RsCase(12, 65, 64 * 12 - 4), RsCase(1, 2, 64, "negative")]


def rs_case_id(c):
    return f"slots{c.slots}-rows{c.rows}-D{c.D}-{c.kind}"


def row_stats_inputs(c):
    """fp32 partials [rows][slots][2]: (sum x, sum x^2) per 64-column group in fp64, rounded; row r is of regime r % 6."""
    if c.kind == "negative":
        # sum x^2 / D - mean^2 < 0 in fp32: a constant row whose sum of squares is one unit in the last place short.  Row 0
        # (7.25): -3.8e-6, above -eps; row 1 (1000): -0.0625, which without the clamp is the square root of a negative number
        p = torch.tensor([[[464.0, 3364.0]], [[64000.0, 64e6]]])
        p[:, :, 1] = _next(p[:, :, 1], -1)
        return p
    g = gen(case_seed(c))
    x = torch.zeros(c.rows, 64 * c.slots, dtype=F64)
    for r in range(c.rows):
        x[r, :c.D] = make_rows(REGIMES[r % len(REGIMES)], 1, c.D, g)[0].double()
    v = x.view(c.rows, c.slots, 64)
    return torch.stack([v.sum(2), (v * v).sum(2)], 2).float()


def row_stats_model(c, part, emulate, mutate=None):
    """-> (mean, rstd) [rows][2]."""
    dt = F32 if emulate else F64
    p = part.to(dt)
    if mutate == "next_slot":
        p = p.reshape(-1, 2).roll(-1, 0).view_as(p)
    s1, s2 = torch.zeros(c.rows, dtype=dt), torch.zeros(c.rows, dtype=dt)
    for k in range(c.slots):                                          # one thread per row, its slots in order
        s1, s2 = s1 + p[:, k, 0], s2 + p[:, k, 1]
    inv = torch.tensor(1.0, dtype=dt) / float(c.D)
    mean = s1 * inv
    var = s2 * inv - mean * mean
    if mutate != "no_clamp":
        var = var.clamp(min=0)
    return torch.stack([mean, 1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=dt))], 1).float()


def row_stats_ratios(c, part, got, regime=None):
    p = part.double()
    s1, s2 = p[:, :, 0].sum(1), p[:, :, 1].sum(1)
    mean = s1 / c.D
    var = (s2 / c.D - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    if c.kind == "negative":                                          # the clamped value itself, two roundings (sqrt, division)
        want = torch.full_like(rstd, 1.0 / math.sqrt(LN_EPS))
        r = ratio((got[:, 1].double() - want).abs(), 2 * U * want) if torch.isfinite(got).all() else INF
        return {"mean": ratio((got[:, 0].double() - mean).abs(), C_RS * U * mean.abs()), "rstd": r}
    bm = C_RS * U * p[:, :, 0].abs().sum(1) / c.D
    bv = C_RS * U * (p[:, :, 1].abs().sum(1) / c.D + mean * mean + LN_EPS)
    em, er, br = (got[:, 0].double() - mean).abs(), (got[:, 1].double() - rstd).abs(), 0.5 * rstd ** 3 * bv + U * rstd
    if regime is not None:                                            # the rows of one regime only (the recorded table)
        sel = torch.arange(c.rows) % len(REGIMES) == REGIMES.index(regime)
        em, er, bm, br = em[sel], er[sel], bm[sel], br[sel]
    return {"mean": ratio(em, bm), "rstd": ratio(er, br)}


# ---------------------------------------------------------------------------------------------------------------------
# similarity_head
ShCase = namedtuple("ShCase", "E B C n_kv bias")


def similarity_cases():
    return [ShCase(E, B, C, k, bias) for E in (4, 68, 132, 508) for B, C, k in ((1, 1, 1), (17, 33, 1), (5, 3, 5)) for bias in (False, True)]


def sh_case_id(c):
    return f"E{c.E}-B{c.B}-C{c.C}-kv{c.n_kv}" + ("-bias" if c.bias else "")


def similarity_inputs(c):
    """Rows with norms from 1e-6 to 1e4."""
    g = gen(case_seed(c))

    def rows(n):
        t = torch.randn(n, c.E, generator=g, dtype=F64)
        scale = torch.pow(10.0, torch.linspace(-6, 4, n)[torch.randperm(n, generator=g)]) if n > 1 else torch.tensor([1e-6])
        return (t / t.norm(dim=1, keepdim=True) * scale[:, None]).float()
    return SimpleNamespace(video=rows(c.B), text=rows(c.C * c.n_kv), scale=torch.tensor([math.log(20.0)]),
                           bias=torch.tensor([-1.5]) if c.bias else None)


def similarity_model(c, inp, emulate):
    """-> (logits [B][C], text_features [C][E], video_norm [B][E]).  Emulation: lanes stride the row by 64, the butterfly, the
    logits as one fma chain over E in order."""
    dt = F32 if emulate else F64
    E = c.E

    def sumsq(t):                                                     # [n][E] -> [n][1]
        if not emulate:
            return (t * t).sum(1, keepdim=True)
        p = torch.zeros(t.shape[0], -(-E // 64) * 64, dtype=F32)
        p[:, :E] = t
        s = torch.zeros(t.shape[0], 64, dtype=F32)
        for j in range(p.shape[1] // 64):
            s = s + p[:, 64 * j:64 * j + 64] * p[:, 64 * j:64 * j + 64]
        lanes = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, :1]
    v, t = inp.video.to(dt), inp.text.to(dt)
    vn = v * (1.0 / torch.sqrt(sumsq(v)))
    tn = t * (1.0 / torch.sqrt(sumsq(t)))
    if c.n_kv == 1:
        m = tn
    else:
        m = torch.zeros(c.C, E, dtype=dt)
        for k in range(c.n_kv):
            m = m + tn.view(c.C, c.n_kv, E)[:, k]
        m = m / float(c.n_kv)
    if emulate:
        acc = torch.zeros(c.B, c.C, dtype=F64)
        for e in range(E):                                            # fma: the product exact, one rounding per step
            acc = (acc + vn[:, e].double()[:, None] * m[:, e].double()[None]).float().double()
        dot = acc.float()
    else:
        dot = vn @ m.T
    logits = torch.exp(inp.scale.to(dt)) * dot + (inp.bias.to(dt) if inp.bias is not None else 0.0)
    tf = m * (1.0 / torch.sqrt(sumsq(m)))
    return logits.float(), tf.float(), vn.float()


def similarity_bounds(c, inp):
    """fp64 references and worst-case bounds.  k = E / 64 terms per lane (rounded up), 6 butterfly steps, the square: the sum of
    squares, all terms positive, is within (k + 7) u; its root halves that; the root, the division and the product round once
    each: a unit row is within n1 u of itself per element, n1 = (k + 7) / 2 + 3.
      class mean m      n_kv unit rows summed in order, then a division: (n1 + n_kv + 1) u mean_k |tn|
      logits            E fma steps, each within u of a partial sum that sum_e |vn_e m_e| bounds: E u sum |vn m|; the operands'
                        errors: sum_e (bvn_e |m_e| + |vn_e| bm_e); expf within 2 ulp, the product and the add of the bias
      text_features     m / |m|: the mean's error through the normalisation, (bm_e + |tf_e| sum_j |tf_j| bm_j) / |m|, and the
                        unit row's own n1 u |tf_e|."""
    E = c.E
    n1 = (-(-E // 64) + 7) / 2 + 3
    v, t = inp.video.double(), inp.text.double()
    vn = v / v.norm(dim=1, keepdim=True)
    tn = (t / t.norm(dim=1, keepdim=True)).view(c.C, c.n_kv, E)
    m = tn.mean(1)
    bvn = n1 * U * vn.abs()
    bm = (n1 + c.n_kv + 1) * U * tn.abs().mean(1) if c.n_kv > 1 else n1 * U * m.abs()
    ls = math.exp(float(inp.scale))
    dot, adot = vn @ m.T, vn.abs() @ m.abs().T
    logits = ls * dot + (float(inp.bias) if c.bias else 0.0)
    bl = ls * (E * U * adot + bvn @ m.abs().T + vn.abs() @ bm.T) * (1 + 8 * U) + 4 * U * ls * dot.abs() + U * logits.abs()
    nm = m.norm(dim=1, keepdim=True)
    tf = m / nm
    btf = (bm + tf.abs() * (tf.abs() * bm).sum(1, keepdim=True)) / nm + n1 * U * tf.abs()
    return (logits, bl), (tf, btf), (vn, bvn)


def similarity_ratios(c, inp, got):
    (l, bl), (tf, btf), (vn, bvn) = similarity_bounds(c, inp)
    return {"logits": ratio((got[0].double() - l).abs(), bl), "text_features": ratio((got[1].double() - tf).abs(), btf),
            "video_norm": ratio((got[2].double() - vn).abs(), bvn)}


# ---------------------------------------------------------------------------------------------------------------------
# the emulations by name: each *_model with emulate=True is the fp32 restatement of its kernel
def emulate_layernorm(c, inp):
    return ln_forward_model(c, inp, True)


def emulate_layernorm_backward(c, inp):
    return ln_backward_model(c, inp, True)


def emulate_qgelu_backward(pre, dh, prec, rounded=True):
    return qgelu_backward_model(pre, dh, prec, True, rounded=rounded)


def emulate_convert(x, prec):
    return convert_model(x, prec)                 # torch's CPU conversion is the restatement: round to nearest even


def emulate_row_stats(c, part):
    return row_stats_model(c, part, True)


def emulate_similarity_head(c, inp):
    return similarity_model(c, inp, True)
