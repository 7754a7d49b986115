"""The row-kernel edge tests' bounds, checked on the CPU before a GPU sees them (rowops_ref.py):

  * the emulation of every kernel's rounding points stays inside every bound test_gpu_rowops_edges.py uses, on every entry
    of its tables: within half of the bounds that carry a fitted constant, within the 16-bit rounding bounds themselves;
  * each constant is the smallest power of two that leaves the emulation that half;
  * mutated references - the bugs the tests are there for - fall outside the bound, and the test names the entry that
    catches each;
  * the tables reach every branch the kernels have.
"""
import pytest
import torch

import rowops_ref as rr
from rowops_ref import F16, BF16

SHARE = 0.5                    # the emulation's share of a bound with a fitted constant
# A mutated reference must miss the bound by more than the share a correct kernel's own rounding may use up, so that this
# rounding cannot pull a wrong result back inside: 1 + SHARE where a constant is fitted, 2 where the bound is a 16-bit rounding.
MUT_FITTED, MUT_ROUNDING = 1 + SHARE, 2.0
FITTED = {(fam, name) for fam, names in rr.GOVERNS.values() for name in names}


def families(emulate=True, mutate=None):
    """Yield (family, case id, regime, {check: ratio}) of the model (emulation or mutated reference) over every table."""
    if mutate is None or mutate in rr.LN_MUTATIONS:
        for c in rr.ln_forward_cases():
            inp = rr.ln_forward_inputs(c)
            yield "ln", rr.ln_case_id(c), c.regime, rr.ln_forward_ratios(c, inp, rr.ln_forward_model(c, inp, emulate, mutate))
    if mutate is None or mutate in rr.LNB_MUTATIONS:
        for c in rr.ln_backward_cases():
            inp = rr.ln_backward_inputs(c)
            yield "lnb", rr.lnb_case_id(c), c.regime, rr.ln_backward_ratios(c, inp, rr.ln_backward_model(c, inp, emulate, mutate))
    if mutate is None or mutate in rr.QG_MUTATIONS:
        for n, p in rr.qgelu_cases():
            pre, dh = rr.qgelu_inputs(n, p)
            res = {"out": rr.qgelu_backward_ratio(pre, dh, rr.qgelu_backward_model(pre, dh, p, emulate, mutate), p)}
            if mutate is None:
                res["fp32"] = rr.qgelu_backward_ratio(pre, dh, rr.qgelu_backward_model(pre, dh, p, emulate, rounded=False), p, rounded=False)
            yield "qg", f"n{n}-{rr.PREC_NAME[p]}", "tails", res
    if mutate is None or mutate in rr.CVT_MUTATIONS:
        for p in rr.PRECS:
            for n in rr.CVT_SIZES:
                x = rr.convert_input(n, p)
                yield "cvt", f"n{n}-{rr.PREC_NAME[p]}", "edges", {"bits": rr.convert_check(x, rr.convert_model(x, p, mutate), p)}
    if mutate is None or mutate in rr.RS_MUTATIONS:
        for c in rr.row_stats_cases():
            part = rr.row_stats_inputs(c)
            # (the hand-made negative variance is judged against the clamped value itself, no constant: a family of its own)
            yield ("rs negative" if c.kind == "negative" else "rs"), rr.rs_case_id(c), c.kind, \
                rr.row_stats_ratios(c, part, rr.row_stats_model(c, part, emulate, mutate))
    if mutate is None:
        for c in rr.similarity_cases():
            inp = rr.similarity_inputs(c)
            yield "sh", rr.sh_case_id(c), "norms", rr.similarity_ratios(c, inp, rr.similarity_model(c, inp, emulate))


@pytest.fixture(scope="module")
def emulated():
    """{(family, check): (worst ratio, entry)} of the emulation, computed once."""
    worst = {}
    for fam, cid, _, res in families():
        for name, r in res.items():
            if r > worst.get((fam, name), (-1.0, ""))[0]:
                worst[(fam, name)] = (r, cid)
    return worst


def test_every_emulation_is_within_every_bound(emulated):
    for (fam, name), (r, cid) in sorted(emulated.items()):
        limit = SHARE if (fam, name) in FITTED else 1.0
        print(f"{fam:12s} {name:16s} {r:8.3f} of {limit:3.1f}   {cid}")
    for (fam, name), (r, cid) in emulated.items():
        assert r <= (SHARE if (fam, name) in FITTED else 1.0), (fam, name, r, cid)
    assert FITTED <= set(emulated)


def test_constants_are_the_smallest_powers_of_two(emulated):
    for cname, (fam, names) in rr.GOVERNS.items():
        C = rr.CONSTANTS[cname]
        worst = max(emulated[(fam, n)][0] for n in names) * C         # against the form with C = 1
        print(f"{cname}: worst emulated ratio against C = 1: {worst:.2f}; C = {C:g}")
        assert C == 2.0 ** round(torch.log2(torch.tensor(C)).item())
        assert 2 * worst <= C < 4 * worst, (cname, worst, C)


# mutation -> (the check that must catch it, a predicate on (entry id, regime) where the catch is expected)
EXPECT = {
    "eps6": lambda cid, reg: reg == "tiny",
    "d_minus_1": lambda cid, reg: True,
    "single_pass": lambda cid, reg: reg == "offset",
    "gamma_shift": lambda cid, reg: True,
    "beta_drop_last": lambda cid, reg: True,
    "stale_lane": lambda cid, reg: "-D260-" in cid,
    "ln2_unaffined": lambda cid, reg: cid.startswith("g2_"),
    "pair_lo_optype": lambda cid, reg: cid.endswith("bf16") and "pair" in cid or cid.startswith("g2_"),
    "no_xhat_term": lambda cid, reg: True,
    "mean_over_1024": lambda cid, reg: "-D1024-" not in cid,
    "no_1702": lambda cid, reg: True,
    "truncate": lambda cid, reg: True,
    "ties_away": lambda cid, reg: True,
    "no_clamp": lambda cid, reg: reg == "negative",
    "next_slot": lambda cid, reg: True,
}
ALL_MUTATIONS = rr.LN_MUTATIONS + rr.LNB_MUTATIONS + rr.QG_MUTATIONS + rr.CVT_MUTATIONS + rr.RS_MUTATIONS


@pytest.mark.parametrize("mutation", ALL_MUTATIONS)
def test_mutated_reference_violates_the_bound(mutation):
    caught = []
    for fam, cid, regime, res in families(emulate=False, mutate=mutation):
        for name, r in res.items():
            if r > (MUT_FITTED if (fam, name) in FITTED else MUT_ROUNDING):
                caught.append((r, fam, name, cid, regime))
    assert caught, f"{mutation}: no entry of its table catches it"
    where = [c for c in caught if EXPECT[mutation](c[3], c[4])]
    assert where, f"{mutation}: caught, but not where it should show: {caught[:3]}"
    r, fam, name, cid, _ = max(where)
    print(f"{mutation}: caught by {len(caught)} checks; worst where it is expected: {fam} {cid} [{name}] at {r:.3g} of the bound")
    if mutation == "pair_lo_optype":                                  # fp16 operands round lo in fp16 either way
        assert all(c[3].endswith("bf16") for c in caught)
    if mutation == "mean_over_1024":
        assert all("-D1024-" not in c[3] for c in caught)


def test_unmutated_references_are_inside():
    """The fp64 models rounded once at the stores: far inside every fitted bound, inside every rounding bound."""
    for fam, cid, _, res in families(emulate=False):
        for name, r in res.items():
            assert r <= (0.25 if (fam, name) in FITTED else 1.0), (fam, cid, name, r)


def test_reference_matches_autograd():
    c = rr.LnbCase("dgamma_70rows", 260, 70, "randn")
    inp = rr.ln_backward_inputs(c)
    x, gm = inp.x.double().requires_grad_(), inp.gamma.double().requires_grad_()
    bt = torch.zeros(260, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (260,), gm, bt, 1e-5)
    y.backward(inp.dy.double())
    got = rr.ln_backward_model(c, inp, emulate=False)
    assert torch.allclose(got["dx"].double(), x.grad, rtol=1e-6, atol=1e-7)
    assert torch.allclose(got["dgamma"].double(), inp.g0.double() + gm.grad, rtol=1e-6, atol=1e-6)
    assert torch.allclose(got["dbeta"].double(), inp.b0.double() + bt.grad, rtol=1e-6, atol=1e-6)
    fc = rr.LnCase("out32", 260, 5, "randn", F16)
    fi = rr.ln_forward_inputs(fc)
    want = torch.nn.functional.layer_norm(fi.x.double(), (260,), fi.gamma.double(), fi.beta.double(), 1e-5)
    assert torch.allclose(rr.ln_forward_model(fc, fi, emulate=False)["out32"].double(), want, rtol=1e-6, atol=1e-7)
    pre, dh = rr.qgelu_inputs(1020, BF16)
    xq = pre.double().requires_grad_()
    (xq * torch.sigmoid(1.702 * xq)).backward(dh.double())
    assert rr.qgelu_backward_ratio(pre, dh, xq.grad.float().to(torch.bfloat16), BF16) <= 1


def test_tables_reach_every_branch():
    reached = []
    # gava_layernorm: act[] patterns (1 to 4 float4 groups per lane) x (last group partly active or not), both precisions
    for prec in rr.PRECS:
        pats = {rr.act_pattern(c.D) for c in rr.ln_forward_cases() if c.prec == prec}
        assert pats == {(n, partial) for n in (1, 2, 3, 4) for partial in (False, True)}, pats
    reached.append("layernorm: 4 act[] patterns x (partial, full) last group, f16 and bf16")
    cases = rr.ln_forward_cases()
    assert {c.form for c in cases} == set(rr.LN_FORMS) and {c.regime for c in cases} == set(rr.REGIMES)
    assert {c.rows for c in cases} == set(rr.LN_ROWS)
    for D in (260, 768, 1020):
        assert {c.form for c in cases if c.D == D and c.regime == "randn"} == set(rr.LN_FORMS)
    for D in (4, 260, 1024):
        for form in ("both", "pair", "g2_both"):
            assert {c.regime for c in cases if c.D == D and c.form == form} == set(rr.REGIMES)
    assert {c.D for c in cases if c.form == "both" and c.regime == "randn"} == set(rr.LN_WIDTHS)
    # the pair's two store paths: behind the first LayerNorm (gamma2) and at the end (no gamma2)
    pair_forms = {(f.g2, f.out32) for name, f in rr.LN_FORMS.items() if f.pair and not f.cast}
    assert pair_forms == {(False, False), (True, False), (True, True)}
    reached.append("layernorm pair: gamma2 and no-gamma2 store paths; split_out at strides 3 D and 3 D + 8; cast-only into all three")
    assert rr.LN_FORMS["split"].pad16 == 0 and rr.LN_FORMS["split_pad"].pad16 == 8
    # gava_layernorm_backward: the widths of the existing lane test and 1024; both dx16 instantiations
    b = rr.ln_backward_cases()
    assert {rr.act_pattern(c.D) for c in b} == {(1, True), (2, True), (4, True), (4, False)}
    assert {rr.lnb_prec(c) for c in b if c.form.startswith("dx16")} == {F16, BF16}
    for D in rr.LNB_WIDTHS:
        for r in rr.REGIMES:
            assert {c.form for c in b if c.D == D and c.regime == r} >= set(rr.LNB_FORMS)
    assert {c.rows for c in b if c.form.startswith("dgamma")} == {1, 70} and any(c.form == "dy_wide" for c in b)
    reached.append("layernorm_backward: D 4 / 260 / 1020 / 1024, f16 and bf16 dx16, atomics at 1 and 70 rows")
    # the grid-stride loops' second trip, both precisions
    assert {p for n, p in rr.qgelu_cases() if n // 4 > 8192 * 256} == set(rr.PRECS)
    assert max(rr.CVT_SIZES) > 4096 * 256 and max(rr.CVT_SIZES) % 256 and all(n % 4 == 0 for n in rr.QG_SIZES)
    reached.append("qgelu_backward and convert_h16: second trip of the grid-stride loop, f16 and bf16")
    for p in rr.PRECS:                                                # all 65536 patterns, and they survive the trim to n
        v = rr.convert_values(p)
        assert v.numel() <= max(rr.CVT_SIZES) and v.numel() >= 65536 + 3 * 2 * 8 * (1 << 7)
    # row_stats: a block with fewer than 64 rows (alone, and as the last of several), every slot count
    rs = rr.row_stats_cases()
    assert {c.slots for c in rs} >= set(rr.RS_SLOTS) and {c.rows % 64 for c in rs} >= {0, 1, 2, 63}
    assert any(c.rows < 64 for c in rs) and any(c.rows > 64 and c.rows % 64 for c in rs) and any(c.D != 64 * c.slots for c in rs)
    reached.append("row_stats: blocks of 1, 63, 64 rows and tails of 1 and 2 rows; 1 to 32 slots; D != 64 slots; negative variance")
    sh = rr.similarity_cases()
    assert {c.E % 64 for c in sh} == {4, 60} and {c.E for c in sh} == {4, 68, 132, 508} and {c.n_kv for c in sh} == {1, 5}
    reached.append("similarity_head: E % 64 != 0 below and above one lane stride, n_kv 1 and 5, with and without bias")
    print("\n".join(reached))
