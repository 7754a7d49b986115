"""gava_attention / gava_attention_backward at the edges of their dispatch tables and in hard softmax regimes, against the
fp64 reference of attention_ref.py on the same 16-bit operands.  The shape tables, the regimes and the bounds live there
(with the reasoning behind the constants); test_attention_ref_host.py checks on the CPU that an emulation of the kernels'
rounding points stays inside every bound used here, that mutated references fall outside, and that the tables reach
every instantiation the host dispatchers can launch.

Every output buffer is NaN-filled, 8 columns wider than the kernel's rows and 3 rows longer: what lies outside must still
be NaN afterwards, what lies inside must be finite.

GAVA_ATTENTION_EDGES_RECORD=<file>: also run the emulation and write the worst error / (eps * scale) per family and
precision, measured | emulated | bound (profiles/attention_edges_errors.txt is such a file).
"""
import os

import pytest
import torch

from gava_clip_amd import hip
import attention_ref as ar

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("GAVA_ATTENTION_EDGES_RECORD")
WORST = {}
PAD_COLS, PAD_ROWS = 8, 3


def family(c, tables):
    return next(name for name, t in tables.items() if c in t)


FWD_TABLES = {"fwd plain": ar.FWD_PLAIN, "fwd causal": ar.FWD_CAUSAL, "fwd few queries": ar.FWD_FEW, "fwd CLS only": ar.FWD_CLS,
              "fwd prompt rows": ar.FWD_VISION, "fwd no summary / split": ar.FWD_EXTRA}
BWD_TABLES = {"bwd causal": ar.BWD_CAUSAL, "bwd plain": ar.BWD_PLAIN, "bwd prompt rows": ar.BWD_VISION, "bwd CLS only": ar.BWD_CLS,
              "bwd no summary": ar.BWD_EXTRA}


def note(fam, what, prec_name, regime, const, measured, emulated, where):
    key = (fam, what, prec_name, "randn" if regime == "randn" else "regimes")
    m, e, _, w = WORST.get(key, (-1.0, -1.0, const, ""))            # each column is the worst of its own
    WORST[key] = (max(m, measured * const), max(e, emulated * const), const, where if measured * const > m else w)


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    if RECORD and WORST:
        with open(RECORD, "w") as f:
            f.write("# worst error / (eps * scale) per test family, output, precision; bound = the test's constant\n")
            f.write(f"# {'family':24s} {'output':6s} {'prec':9s} {'inputs':8s} {'GPU':>6s} {'emul.':>6s} {'bound':>5s}  worst case on the GPU\n")
            for (fam, what, pn, reg), (m, e, c, where) in sorted(WORST.items()):
                f.write(f"  {fam:24s} {what:6s} {pn:9s} {reg:8s} {m:6.2f} {e:6.2f} {c:5.1f}  {where}\n")


def padded(rows, cols, dtype):
    return torch.full((rows + PAD_ROWS, cols + PAD_COLS), float("nan"), dtype=dtype, device="cuda")


def check_padding(buf, rows, cols, name):
    assert torch.isnan(buf[:, cols:]).all() and torch.isnan(buf[rows:]).all(), f"{name}: written outside its rows"
    assert torch.isfinite(buf[:rows, :cols]).all(), f"{name}: not finite"


def query_buffer(c, t, fill):
    """[BT*nq][W] -> the separate query-side buffer of qbr rows per frame; rows that are no query hold `fill`."""
    nq, W = ar.n_queries(c), t.shape[1]
    buf = torch.full((c.BT, c.qbr, W), fill, dtype=t.dtype)
    buf[:, :nq] = t.view(c.BT, nq, W)
    return buf.view(c.BT * c.qbr, W).cuda()


FWD_PARAMS = ar.forward_params()


@pytest.mark.parametrize("c,regime,prec", FWD_PARAMS, ids=[f"{ar.case_id(c)}-{r}-{ar.PREC_NAME[p]}" for c, r, p in FWD_PARAMS])
def test_attention_forward_edges(c, regime, prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    x = ar.make_inputs(c, regime, ar.seed_of(c, regime), prec)
    ref = ar.reference(c, x)
    D, nq = c.heads * 64, ar.n_queries(c)
    if c.qbr:
        q = query_buffer(c, x.q, float("nan"))       # the clamped loads of a partial tile must not reach past the queries
        kv = torch.cat([x.k, x.v], 1).cuda()
        k, v = kv[:, :D], kv[:, D:]
    else:
        qkv = torch.cat([x.q, x.k, x.v], 1).cuda()
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    side = x.side.cuda() if c.side else None
    W = 3 * D if c.split else D
    buf = padded(c.BT * nq, W, x.q.dtype)
    hip.attention(q, k, v, buf, batch=c.BT, heads=c.heads, n_q=nq, n_kmain=c.n, prec=prec, causal=c.causal,
                  side_k=side[:, :D] if c.side else None, side_v=side[:, D:] if c.side else None,
                  n_g=c.G, T=c.T if c.side else 0, has_summary=c.has_summary, split_out=c.split, q_batch_rows=c.qbr)
    torch.cuda.synchronize()
    buf = buf.cpu()
    check_padding(buf, c.BT * nq, W, "out")
    out = buf[:c.BT * nq, :W]
    got = out[:, :D].double()
    if c.split:                                                      # rows [hi | lo | hi]: hi + lo carries the fp32 result
        assert torch.equal(out[:, :D], out[:, 2 * D:])
        assert ar.forward_ratio(c, got, ref, prec) <= 1
        got = got + out[:, D:2 * D].double()
    ratio = ar.forward_ratio(c, got, ref, prec)
    print(f"forward error / bound = {ratio:.3f}")
    if RECORD:
        emu = ar.forward_ratio(c, ar.emulate_forward(c, x, prec), ref, prec)
        note(family(c, FWD_TABLES), "out", ar.PREC_NAME[prec], regime, ar.FWD_C, ratio, emu, f"{ar.case_id(c)} {regime}")
    assert ratio <= 1, f"|out - ref| reaches {ratio:.2f} of 4 eps * sum p|v| (+ fp16 floor)"


BWD_PARAMS = ar.backward_params()


@pytest.mark.parametrize("c,regime,prec,act", BWD_PARAMS,
                         ids=[f"{ar.case_id(c)}-{r}-{ar.PREC_NAME[p]}-act{ar.PREC_NAME[a]}" for c, r, p, a in BWD_PARAMS])
def test_attention_backward_edges(c, regime, prec, act):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    x = ar.make_inputs(c, regime, ar.seed_of(c, regime), prec, act)
    ref = ar.reference(c, x, backward=True)
    D, nq, gt = c.heads * 64, ar.n_queries(c), ar.DTYPE[prec]
    dqkv = padded(c.BT * c.n, 3 * D, gt)
    if c.qbr:
        q, do = query_buffer(c, x.q, float("nan")), query_buffer(c, x.dout, float("nan"))
        kv = torch.cat([x.k, x.v], 1).cuda()
        k, v = kv[:, :D], kv[:, D:]
        dq_buf = padded(c.BT * c.qbr, D, gt)
        dq_arg = dq_buf
    else:
        qkv = torch.cat([x.q, x.k, x.v], 1).cuda()
        q, k, v, do = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], x.dout.cuda()
        dq_arg = dqkv[:, :D]
    side = x.side.cuda() if c.side else None
    ns = ar.n_side(c)
    part = torch.full((c.BT * ns + PAD_ROWS, 2 * D + PAD_COLS), float("nan"), dtype=torch.float32, device="cuda") if c.side else None
    hip.attention_backward(q, k, v, do, dq_arg, dqkv[:, D:2 * D], dqkv[:, 2 * D:], batch=c.BT, heads=c.heads, n=c.n, prec=prec,
                           causal=c.causal, q_scale=0.125, q_batch_rows=c.qbr, n_q=c.n_q,
                           side_k=side[:, :D] if c.side else None, side_v=side[:, D:] if c.side else None,
                           dside_k=part[:, :D] if c.side else None, dside_v=part[:, D:] if c.side else None,
                           n_g=c.G, T=c.T if c.side else 0, has_summary=c.has_summary, act_prec=act if act != prec else None)
    torch.cuda.synchronize()
    dqkv = dqkv.cpu()
    if c.qbr:
        dq_buf = dq_buf.cpu()
        assert torch.isnan(dq_buf[:, D:]).all() and torch.isnan(dq_buf[c.BT * c.qbr:]).all(), "dq: written outside its rows"
        rows = dq_buf[:c.BT * c.qbr, :D].reshape(c.BT, c.qbr, D)
        assert torch.isnan(rows[:, nq:]).all(), "dq: rows that are no query written"
        dq = rows[:, :nq].reshape(c.BT * nq, D)
        assert torch.isfinite(dq).all()
        assert torch.isnan(dqkv[:, :D]).all()
        dqkv[:c.BT * c.n, :D] = 0                                    # nothing is due there: dq has its own buffer
    else:
        dq = dqkv[:c.BT * c.n, :D]
    check_padding(dqkv, c.BT * c.n, 3 * D, "dqkv")
    dside = None
    if c.side:
        part = part.cpu()
        check_padding(part, c.BT * ns, 2 * D, "dside")
        dside = part[:c.BT * ns, :2 * D].reshape(c.BT, ns, 2 * D)
    got = (dq, dqkv[:c.BT * c.n, D:2 * D], dqkv[:c.BT * c.n, 2 * D:3 * D], dside)
    ratios = ar.backward_ratios(c, got, ref, prec, regime)
    print("backward error / bound:", {k_: round(v_, 3) for k_, v_ in ratios.items()})
    if RECORD:
        emu = ar.backward_ratios(c, ar.emulate_backward(c, x, prec), ref, prec, regime)
        for name in ratios:
            note(family(c, BWD_TABLES), name, f"{ar.PREC_NAME[prec]}/{ar.PREC_NAME[act]}", regime, ar.BWD_C, ratios[name], emu[name],
                 f"{ar.case_id(c)} {regime}")
    for name, r in ratios.items():
        assert r <= 1, f"{name}: error reaches {r:.2f} of 3 eps * the block's scale"


# ---------------------------------------------------------------------------------------------------------------------
def test_attention_entry_points_refuse():
    """GAVA_EINVAL comes back before anything is launched: causal past the resident forms, and the alignment and stride rules
    of the two entry points."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    D, dt = 128, torch.float16
    t = lambda rows, cols=D, d=dt: torch.zeros(rows, cols, dtype=d, device="cuda")
    bad = lambda: pytest.raises(hip.GavaError, match="GAVA_EINVAL")

    def fwd(q=None, k=None, v=None, out=None, L=32, **kw):
        args = dict(batch=2, heads=2, n_q=L, n_kmain=L, prec=hip.PREC_F16)
        args.update(kw)
        hip.attention(t(2 * L) if q is None else q, t(2 * L) if k is None else k, t(2 * L) if v is None else v,
                      t(2 * L) if out is None else out, **args)

    fwd()                                                            # the baseline is accepted
    fwd(L=320, causal=True)
    with bad():
        fwd(L=321, causal=True)
    side = t(2 + 4, 2 * D)
    with bad():                                                        # 320 main rows + prompt rows, causal
        fwd(L=320, causal=True, side_k=side[:, :D], side_v=side[:, D:], n_g=2, T=1, has_summary=True)
    with bad():
        fwd(k=t(64, D + 4)[:, :D])                                   # ld_qkv % 8
    with bad():
        fwd(out=t(64, D + 2)[:, :D])                                 # ld_out % 4
    with bad():
        fwd(q=t(65).view(-1)[4:4 + 64 * D].view(64, D))              # q 8 bytes off a 16-byte boundary
    with bad():
        fwd(out=t(65).view(-1)[1:1 + 64 * D].view(64, D))            # out 2 bytes off
    with bad():
        fwd(out=t(64, 2 * D), split_out=True)                        # split rows need 3 D columns
    with bad():
        fwd(q=t(2 * 8), n_q=16, q_batch_rows=8)                      # fewer rows per frame than queries
    with bad():
        fwd(side_k=side[:, :D], side_v=side[:, D:], n_g=2, T=3, has_summary=True)    # batch % T
    side4 = t(6, 2 * D + 4)
    with bad():
        fwd(side_k=side4[:, :D], side_v=side4[:, D:2 * D], n_g=2, T=1, has_summary=True)   # ld_side % 8
    with bad():
        fwd(prec=7)

    bf = torch.bfloat16

    def bwd(n=32, dout=None, dq=None, dk=None, dv=None, q=None, **kw):
        args = dict(batch=2, heads=2, n=n, prec=hip.PREC_BF16, q_scale=0.125)
        args.update(kw)
        z = lambda: t(2 * n, D, bf)
        hip.attention_backward(z() if q is None else q, z(), z(), z() if dout is None else dout, z() if dq is None else dq,
                               z() if dk is None else dk, z() if dv is None else dv, **args)

    bwd()
    bwd(n=288, causal=True)
    with bad():
        bwd(n=289, causal=True)
    with bad():
        bwd(causal=True, act_prec=hip.PREC_F16)                      # the causal form converts nothing on load
    with bad():
        bwd(causal=True, n_q=16)
    sideb, ds = t(6, 2 * D, bf), t(2 * 4, 2 * D, torch.float32)
    prompt = dict(side_k=sideb[:, :D], side_v=sideb[:, D:], dside_k=ds[:, :D], dside_v=ds[:, D:], n_g=2, T=1, has_summary=True)
    bwd(**prompt)
    with bad():
        bwd(causal=True, **prompt)
    with bad():
        bwd(**dict(prompt, T=3))                                     # batch % T
    with bad():
        bwd(**dict(prompt, dside_k=None))
    with bad():
        bwd(n_q=33)                                                  # more queries than rows
    with bad():
        bwd(dout=t(64, D + 4, bf)[:, :D])                            # ld_dout % 8
    with bad():
        bwd(dk=t(64, D + 2, bf)[:, :D], dv=t(64, D + 2, bf)[:, :D])  # ld_dqkv % 4
    with bad():
        bwd(dq=t(65, D, bf).view(-1)[1:1 + 64 * D].view(64, D))      # dq 2 bytes off
    with bad():
        bwd(q=t(65, D, bf).view(-1)[4:4 + 64 * D].view(64, D))       # q 8 bytes off
    with bad():
        bwd(q=t(2 * 8, D, bf), dout=t(2 * 8, D, bf), dq=t(2 * 8, D, bf), n_q=16, q_batch_rows=8)
    with bad():
        bwd(prec=hip.PREC_F16, act_prec=hip.PREC_BF16)               # fp16 gradients over bf16 activations: no such form
    torch.cuda.synchronize()
