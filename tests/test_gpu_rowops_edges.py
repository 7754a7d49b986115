"""The row kernels at their lane, stride and value edges, against the fp64 references of rowops_ref.py on the operands the
kernels really receive: gava_layernorm, gava_layernorm_backward, gava_qgelu_backward, gava_convert_h16, gava_row_stats,
gava_similarity_head.  The tables, the regimes and the bounds live in rowops_ref.py (with the reasoning behind every
constant); test_rowops_ref_host.py checks on the CPU that an emulation of the kernels' rounding points stays inside every
bound used here, that mutated references fall outside, and that the tables reach every branch.

Every output buffer is NaN-filled, 8 columns wider than the kernel's rows and 3 rows longer (flat buffers: a NaN tail): what
lies outside must still be NaN afterwards, what lies inside must be finite.  The input rows of both LayerNorm kernels are
views into NaN-padded buffers too: a lane that reads past D poisons its row.  Buffers that are accumulated into start from
known finite values inside the same padding.

GAVA_ROWOPS_EDGES_RECORD=<file>: also run the emulation and write the worst error per family, check and precision,
measured | emulated | bound (profiles/rowops_edges_errors.txt is such a file).
"""
import ctypes as C
import os

import pytest
import torch

from gava_clip_amd import hip
import rowops_ref as rr

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("GAVA_ROWOPS_EDGES_RECORD")
WORST = {}
PAD_COLS, PAD_ROWS, PAD_FLAT = 8, 3, 1024
NAN = float("nan")
CONST_OF = {(fam, name): rr.CONSTANTS[cn] for cn, (fam, names) in rr.GOVERNS.items() for name in names}
FAMILY = {"ln": "layernorm", "lnb": "layernorm_backward", "qg": "qgelu_backward", "cvt": "convert_h16", "rs": "row_stats",
          "sh": "similarity_head"}


def note(fam, check, prec_name, measured, emulated, where, key=None):
    """Ratios are fractions of the bound; the table shows them in units of the bound's form with C = 1."""
    const = CONST_OF.get((key or fam, check), 1.0)
    k = (FAMILY.get(fam, fam), check, prec_name)
    m, e, _, w = WORST.get(k, (-1.0, -1.0, const, ""))                # each column is the worst of its own
    WORST[k] = (max(m, measured * const), max(e, emulated * const), const, where if measured * const > m else w)


def note_all(fam, prec_name, ratios, emulated, where, key=None):
    for name, r in ratios.items():
        note(fam, name, prec_name, r, emulated.get(name, 0.0), where, key)


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    if RECORD and WORST:
        with open(RECORD, "w") as f:
            f.write("# worst error per test family, check and precision, in units of the bound's form with its constant set to 1\n"
                    "# (tests/rowops_ref.py); bound = the constant: GPU <= bound passes.  Checks named `bits` are 0 or inf.\n")
            f.write(f"# {'family':28s} {'check':24s} {'prec':5s} {'GPU':>8s} {'emul.':>8s} {'bound':>6s}  worst case on the GPU\n")
            for (fam, what, pn), (m, e, c, where) in sorted(WORST.items()):
                f.write(f"  {fam:28s} {what:24s} {pn:5s} {m:8.3f} {e:8.3f} {c:6.1f}  {where}\n")


def padded(rows, cols, dtype, pad_cols=PAD_COLS, fill=NAN):
    return torch.full((rows + PAD_ROWS, cols + pad_cols), fill, dtype=dtype, device="cuda")


def nan_view(t):
    """A device copy of the rows of t as a view into a NaN-padded buffer -> (view, buffer)."""
    buf = padded(t.shape[0], t.shape[1], t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t.cuda()
    return buf[:t.shape[0], :t.shape[1]], buf


def check_padding(buf, rows, cols, name, finite=True):
    buf = buf.cpu()
    assert torch.isnan(buf[:, cols:]).all() and torch.isnan(buf[rows:]).all(), f"{name}: written outside its rows"
    if finite:
        assert torch.isfinite(buf[:rows, :cols]).all(), f"{name}: not finite"
    return buf[:rows, :cols]


def flat(n, dtype):
    return torch.full((n + PAD_FLAT,), NAN, dtype=dtype, device="cuda")


def check_flat(buf, n, name, finite=True):
    buf = buf.cpu()
    assert torch.isnan(buf[n:]).all(), f"{name}: written past its end"
    if finite:
        assert torch.isfinite(buf[:n]).all(), f"{name}: not finite"
    return buf[:n]


def assert_ratios(ratios, what):
    print(what, {k: round(v, 3) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1, f"{what}: {name} reaches {r:.3g} of its bound"


# ---------------------------------------------------------------------------------------------------------------------
LN_CASES = rr.ln_forward_cases()


@pytest.mark.parametrize("c", LN_CASES, ids=rr.ln_case_id)
def test_layernorm_edges(c):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    inp, f, P, D, rows = rr.ln_forward_inputs(c), rr.LN_FORMS[c.form], rr.DTYPE[c.prec], c.D, c.rows
    src = inp.src if f.gather else inp.x
    x, xbuf = nan_view(src)
    dev = lambda t: None if t is None else t.cuda()
    W16 = 3 * D if f.split else D
    o16 = padded(rows, W16, P, f.pad16) if f.out16 else None
    o32 = None if not f.out32 else (xbuf if f.alias else padded(rows, D, torch.float32))
    ohi, olo = (padded(rows, D, P), padded(rows, D, torch.float16)) if f.pair else (None, None)
    view = lambda b, w: None if b is None else b[:rows, :w]
    hip.layernorm(x, dev(inp.gamma), dev(inp.beta), out16=view(o16, W16), out32=view(o32, D), prec=c.prec, rows=rows,
                  row_index=dev(inp.index), split_out=f.split, gamma2=dev(inp.gamma2), beta2=dev(inp.beta2),
                  out_hi=view(ohi, D), out_lo=view(olo, D))
    torch.cuda.synchronize()
    got = {}
    if f.out32:
        got["out32"] = check_padding(o32, rows, D, "out32")
    if not f.alias:                                                   # the input is as it was, padding included
        assert torch.equal(check_padding(xbuf, src.shape[0], D, "in"), src)
    if f.out16:
        got["out16"] = check_padding(o16, rows, W16, "out16")
    if f.pair:
        got["hi"], got["lo"] = check_padding(ohi, rows, D, "out_hi"), check_padding(olo, rows, D, "out_lo")
    ratios = rr.ln_forward_ratios(c, inp, got)
    if RECORD:
        note_all("ln", rr.PREC_NAME[c.prec], ratios, rr.ln_forward_ratios(c, inp, rr.emulate_layernorm(c, inp)), rr.ln_case_id(c))
    assert_ratios(ratios, "layernorm")


# ---------------------------------------------------------------------------------------------------------------------
LNB_CASES = rr.ln_backward_cases()


@pytest.mark.parametrize("c", LNB_CASES, ids=rr.lnb_case_id)
def test_layernorm_backward_edges(c):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    inp, D, rows, prec = rr.ln_backward_inputs(c), c.D, c.rows, rr.lnb_prec(c)
    gather = inp.index is not None
    src = inp.src if gather else inp.x
    x, _ = nan_view(src)
    dy, _ = nan_view(inp.dy)
    n_dx = src.shape[0]                                               # scattered: dx has the rows of the source matrix
    dxbuf = padded(n_dx, D, torch.float32)
    if inp.base is not None:
        dxbuf[:rows, :D] = inp.base.cuda()
    dx16 = padded(rows, D, rr.DTYPE[prec]) if c.form.startswith("dx16") else None
    dg = db = None
    if inp.g0 is not None:
        dg, db = torch.full((D + PAD_COLS,), NAN, device="cuda"), torch.full((D + PAD_COLS,), NAN, device="cuda")
        dg[:D], db[:D] = inp.g0.cuda(), inp.b0.cuda()
    idx = inp.index.cuda() if gather else None
    hip.layernorm_backward(x, inp.gamma.cuda(), dy, dxbuf[:n_dx, :D], accumulate=inp.base is not None, x_row_index=idx,
                           dx_row_index=idx, rows=rows, dgamma=dg, dbeta=db, dx16=None if dx16 is None else dx16[:rows, :D], prec=prec)
    torch.cuda.synchronize()
    got = {}
    if gather:                                                        # the rows the index names, and nothing else
        full = check_padding(dxbuf, n_dx, D, "dx", finite=False)
        named = torch.zeros(n_dx, dtype=torch.bool)
        named[inp.index.long()] = True
        assert torch.isnan(full[~named]).all(), "dx: a row outside the index written"
        got["dx"] = full[inp.index.long()]
        assert torch.isfinite(got["dx"]).all()
    else:
        got["dx"] = check_padding(dxbuf, rows, D, "dx")
    if dx16 is not None:
        got["dx16"] = check_padding(dx16, rows, D, "dx16")
    if dg is not None:
        got["dgamma"], got["dbeta"] = check_flat(dg, D, "dgamma"), check_flat(db, D, "dbeta")
    ratios = rr.ln_backward_ratios(c, inp, got)
    if RECORD:
        note_all("lnb", rr.PREC_NAME[prec] if dx16 is not None else "-", ratios,
                 rr.ln_backward_ratios(c, inp, rr.emulate_layernorm_backward(c, inp)), rr.lnb_case_id(c))
    assert_ratios(ratios, "layernorm_backward")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,prec", rr.qgelu_cases(), ids=[f"n{n}-{rr.PREC_NAME[p]}" for n, p in rr.qgelu_cases()])
def test_qgelu_backward_edges(n, prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pre, dh = rr.qgelu_inputs(n, prec)
    out = flat(n, rr.DTYPE[prec])
    hip.qgelu_backward(pre.cuda(), dh.cuda(), out[:n], prec)
    torch.cuda.synchronize()
    got = check_flat(out, n, "dpre")
    r = rr.qgelu_backward_ratio(pre, dh, got, prec)
    if RECORD:
        emu = rr.qgelu_backward_ratio(pre, dh, rr.emulate_qgelu_backward(pre, dh, prec), prec)
        note("qg", "out", rr.PREC_NAME[prec], r, emu, f"n{n}")
    assert_ratios({"out": r}, "qgelu_backward")


# ---------------------------------------------------------------------------------------------------------------------
CVT_CASES = [(n, p) for p in rr.PRECS for n in rr.CVT_SIZES]


@pytest.mark.parametrize("n,prec", CVT_CASES, ids=[f"n{n}-{rr.PREC_NAME[p]}" for n, p in CVT_CASES])
def test_convert_h16_edges(n, prec):
    """Every 16-bit pattern, every tie of the sampled exponents with its fp32 neighbours, the overflow edge, zeros, infs and
    NaN: the bits of torch's CPU conversion (round to nearest even, subnormal results kept)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    x = rr.convert_input(n, prec)
    out = flat(n, rr.DTYPE[prec])
    hip.convert_h16(x.cuda(), prec, out=out[:n])
    torch.cuda.synchronize()
    got = check_flat(out, n, "out", finite=False)
    want = x.to(rr.DTYPE[prec])
    bad = (got.view(torch.int16) != want.view(torch.int16)) & ~torch.isnan(x)
    if bad.any():                                                     # name the class of inputs that differs
        i = bad.nonzero()[:8, 0]
        print("differs at", [(float(x[j]), hex(int(got.view(torch.int16)[j]) & 0xffff), hex(int(want.view(torch.int16)[j]) & 0xffff)) for j in i])
    r = rr.convert_check(x, got, prec)
    if RECORD:
        note("cvt", "bits", rr.PREC_NAME[prec], r, rr.convert_check(x, rr.convert_model(x, prec), prec), f"n{n}")
    assert r == 0, f"{int(bad.sum())} of {n} values differ from round-to-nearest-even"


@pytest.mark.parametrize("prec", rr.PRECS, ids=lambda p: rr.PREC_NAME[p])
def test_split_pack_weight_carries_the_weight(prec):
    """[W_hi | W_hi | W_lo] out of two conversions: |hi + lo - w| <= max(eps16^2 |w|, half the smallest subnormal)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = rr.gen(11 + prec)
    w = torch.randn(12, 68, generator=g) * torch.pow(10.0, torch.randint(-7, 3, (12, 1), generator=g).float())
    w[0, :4] = torch.tensor([0.0, -0.0, 2.0 ** -24, 65504.0])
    packed = hip.split_pack_weight(w.cuda(), prec).cpu()
    assert packed.shape == (12, 3 * 68) and torch.equal(packed[:, :68], packed[:, 68:136])
    assert rr.same_bits(packed[:, :68], w.to(rr.DTYPE[prec])) == 0
    s = packed[:, :68].double() + packed[:, 136:].double()
    r = rr.ratio((s - w.double()).abs(), rr.split_bound(w.double(), prec))
    if RECORD:
        hi = w.to(rr.DTYPE[prec])
        emu = hi.double() + (w - hi.float()).to(rr.DTYPE[prec]).double()
        note("cvt", "split_pack_weight sum", rr.PREC_NAME[prec], r, rr.ratio((emu - w.double()).abs(), rr.split_bound(w.double(), prec)), "12 x 68")
    assert_ratios({"hi + lo": r}, "split_pack_weight")


# ---------------------------------------------------------------------------------------------------------------------
RS_CASES = rr.row_stats_cases()


def row_stats(part, c, stats):
    hip.check(hip.load().gava_row_stats(hip.ptr(part), c.slots, c.D, c.rows, hip.ptr(stats), hip.stream_ptr()), "gava_row_stats")


@pytest.mark.parametrize("c", RS_CASES, ids=rr.rs_case_id)
def test_row_stats_edges(c):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    part = rr.row_stats_inputs(c)
    pbuf = torch.full((c.rows + PAD_ROWS, c.slots, 2), NAN, device="cuda")      # the rows behind the last are no input
    pbuf[:c.rows] = part.cuda()
    stats = torch.full((c.rows + PAD_ROWS, 2), NAN, device="cuda")
    row_stats(pbuf, c, stats)
    torch.cuda.synchronize()
    stats = stats.cpu()
    assert torch.isnan(stats[c.rows:]).all(), "stats: written past the rows"
    got = stats[:c.rows]
    assert torch.isfinite(got).all(), "stats: not finite"
    ratios = rr.row_stats_ratios(c, part, got)
    if RECORD:
        emu = rr.emulate_row_stats(c, part)
        if c.kind == "negative":
            note_all("row_stats, negative variance", "-", ratios, rr.row_stats_ratios(c, part, emu), rr.rs_case_id(c))
        else:                                                         # per regime: `offset` is where E[x^2] - mean^2 cancels
            for i, regime in enumerate(rr.REGIMES[:c.rows]):
                note_all(f"row_stats / {regime}", "-", rr.row_stats_ratios(c, part, got, regime), rr.row_stats_ratios(c, part, emu, regime),
                         f"{rr.rs_case_id(c)} row {i} + 6 k", key="rs")
    assert_ratios(ratios, "row_stats")


# ---------------------------------------------------------------------------------------------------------------------
SH_CASES = rr.similarity_cases()


@pytest.mark.parametrize("c", SH_CASES, ids=rr.sh_case_id)
def test_similarity_head_edges(c):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    inp = rr.similarity_inputs(c)
    logits, tf, vn = flat(c.B * c.C, torch.float32), flat(c.C * c.E, torch.float32), flat(c.B * c.E, torch.float32)
    video, text, scale = inp.video.cuda(), inp.text.cuda(), inp.scale.cuda()      # (named: a pointer does not keep a tensor alive)
    bias = inp.bias.cuda() if c.bias else None
    hip.check(hip.load().gava_similarity_head(hip.ptr(video), hip.ptr(text), hip.ptr(scale), hip.ptr(bias),
                                              c.B, c.C, c.n_kv, c.E, hip.ptr(logits), hip.ptr(tf), hip.ptr(vn), hip.stream_ptr()),
              "gava_similarity_head")
    torch.cuda.synchronize()
    got = (check_flat(logits, c.B * c.C, "logits").view(c.B, c.C), check_flat(tf, c.C * c.E, "text_features").view(c.C, c.E),
           check_flat(vn, c.B * c.E, "video_norm").view(c.B, c.E))
    ratios = rr.similarity_ratios(c, inp, got)
    if RECORD:
        note_all("sh", "-", ratios, rr.similarity_ratios(c, inp, rr.emulate_similarity_head(c, inp)), rr.sh_case_id(c))
    assert_ratios(ratios, "similarity_head")


# ---------------------------------------------------------------------------------------------------------------------
def test_row_entry_points_refuse():
    """GAVA_EINVAL comes back before anything is launched: the output buffers of every refused call are still NaN."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hip.load()
    bad = lambda: pytest.raises(hip.GavaError, match="GAVA_EINVAL")
    D, rows = 64, 5
    z = lambda r, c, d=torch.float32: torch.zeros(r, c, dtype=d, device="cuda")
    nan = lambda r, c, d=torch.float32: torch.full((r, c), NAN, dtype=d, device="cuda")
    x, gm, bt = z(rows, 1100), torch.ones(1100, device="cuda"), z(1, 1100).view(-1)
    o16, o32, ohi, olo = nan(rows, 3 * 1100, torch.float16), nan(rows, 1100), nan(rows, 1100, torch.float16), nan(rows, 1100, torch.float16)

    def ln(**kw):
        args = dict(inp=x, in_stride=1100, gamma=gm, beta=bt, out16=o16, out16_stride=3300, out32=o32, out32_stride=1100,
                    rows=rows, D=D, prec=hip.PREC_F16, split_out=0)
        args.update(kw)
        a = hip.LayerNormArgs()
        for k, v in args.items():
            setattr(a, k, hip.ptr(v) if torch.is_tensor(v) else v)
        hip.check(lib.gava_layernorm(C.byref(a), hip.stream_ptr()), "gava_layernorm")

    pair = dict(out_hi=ohi, out_lo=olo, out_hl_stride=1100)
    second = dict(gamma2=gm, beta2=bt)
    for kw in (dict(D=66), dict(D=0), dict(D=1028), dict(rows=0), dict(in_stride=1102), dict(out16_stride=3302), dict(out32_stride=1098),
               dict(split_out=1, out16=None), dict(split_out=1, out16_stride=3 * D - 4), dict(out_hi=ohi, out_hl_stride=1100),
               dict(out_lo=olo, out_hl_stride=1100), dict(pair, out_hl_stride=D - 4), dict(pair, out_hl_stride=1102), dict(beta=None),
               dict(second, gamma=None, beta=None), dict(second, out16=None), dict(second, out32=None), dict(gamma2=gm),
               dict(out16=None, out32=None), dict(prec=2), dict(prec=-1), dict(inp=None)):
        with bad():
            ln(**kw)
    torch.cuda.synchronize()
    for name, b in (("out16", o16), ("out32", o32), ("out_hi", ohi), ("out_lo", olo)):
        assert torch.isnan(b).all(), f"gava_layernorm: a refused call wrote {name}"
    ln()                                                              # the baseline and the widest forms are accepted
    ln(D=1024, split_out=1, **pair, **second)
    ln(gamma=None, beta=None, out32=None)
    torch.cuda.synchronize()
    assert torch.isfinite(o32[:, :1024]).all() and torch.isnan(o32[:, 1024:]).all()

    stats, part = nan(8, 2), z(8, 33 * 2)
    for slots in (0, 33, -1):
        with bad():
            hip.check(lib.gava_row_stats(hip.ptr(part), slots, 64, 8, hip.ptr(stats), hip.stream_ptr()), "gava_row_stats")
    with bad():
        hip.check(lib.gava_row_stats(hip.ptr(part), 4, 256, 0, hip.ptr(stats), hip.stream_ptr()), "gava_row_stats")
    h = nan(1, 64, torch.bfloat16)
    for n in (1, 2, 3, 62):
        with bad():
            hip.check(lib.gava_qgelu_backward(hip.ptr(h), hip.ptr(h), hip.ptr(h), n, hip.PREC_BF16, hip.stream_ptr()), "gava_qgelu_backward")
    with bad():
        hip.check(lib.gava_qgelu_backward(hip.ptr(h), hip.ptr(h), hip.ptr(h), 64, 2, hip.stream_ptr()), "gava_qgelu_backward")
    src = z(1, 64)
    for prec in (2, -1):
        with bad():
            hip.check(lib.gava_convert_h16(hip.ptr(src), hip.ptr(h), 64, prec, hip.stream_ptr()), "gava_convert_h16")
    hip.check(lib.gava_convert_h16(hip.ptr(src), hip.ptr(h), 0, hip.PREC_BF16, hip.stream_ptr()), "gava_convert_h16")   # n = 0: accepted, nothing written
    lg, tf, vn, ls = nan(1, 16), nan(4, 64), nan(4, 64), z(1, 1)
    for E in (62, 63, 0):
        with bad():
            hip.check(lib.gava_similarity_head(hip.ptr(src), hip.ptr(src), hip.ptr(ls), None, 1, 1, 1, E, hip.ptr(lg), hip.ptr(tf), hip.ptr(vn),
                                               hip.stream_ptr()), "gava_similarity_head")
    torch.cuda.synchronize()
    for name, b in (("stats", stats), ("qgelu / convert", h), ("logits", lg), ("text_features", tf), ("video_norm", vn)):
        assert torch.isnan(b).all(), f"a refused call wrote {name}"
