"""The attention edge tests' bounds, checked on the CPU before a GPU sees them (attention_ref.py):

  * the fp64 reference agrees with torch autograd and with the older tests' ref_attention;
  * the emulation of the kernels' rounding points stays well inside every bound that test_gpu_attention_edges.py uses, on
    every shape, regime and precision of its tables;
  * mutated references - the bugs the tests are there for - violate the bound;
  * the tables reach every instantiation the two host dispatchers can launch.
"""
import pytest
import torch

import attention_ref as ar
from attention_ref import F16, BF16

# Forward: the emulation within HALF the bound (2 of the 4 eps * scale).  Backward: within 1.95 of the 3 eps * scale - the
# first-order count is 2 eps (P or dS rounded to the gradient type, the result rounded), measured 1.81 (bf16 dq, randn, 320
# keys); half of 3 is below that count, so no input could meet it.
FWD_SHARE, BWD_SHARE = 0.5, 1.95 / 3
# A mutated reference must miss the bound by more than the emulation's share of it, so that the kernel's own rounding
# error cannot pull a wrong result back inside: 1 + share.
MUT_FWD, MUT_BWD = 1 + FWD_SHARE, 1 + BWD_SHARE


def inputs(c, regime, prec, act=None):
    return ar.make_inputs(c, regime, ar.seed_of(c, regime), prec, act)


def test_reference_matches_autograd():
    for c in (ar.vision(4, 2, 3, 21, heads=2), ar.vision(4, 2, 3, 21, n_q=5, qbr=5, has_summary=False), ar.plain(2, 19, causal=True)):
        x = inputs(c, "randn", BF16)
        ref = ar.reference(c, x, backward=True)
        BT, nq, D, H = c.BT, ar.n_queries(c), c.heads * 64, c.heads
        q, k, v = [t.double().requires_grad_() for t in (x.q, x.k, x.v)]
        s = x.side.double().requires_grad_() if c.side else None
        K, V = k.view(BT, c.n, D), v.view(BT, c.n, D)
        if c.side:
            idx = ar.side_index(BT, c.T, c.G, "cpu")[:, :ar.n_side(c)]
            K, V = torch.cat([K, s[idx, :D]], 1), torch.cat([V, s[idx, D:]], 1)
        heads = lambda t: t.view(BT, -1, H, 64).transpose(1, 2)
        S = heads(q.view(BT, nq, D)) @ heads(K).transpose(-1, -2)
        if c.causal:
            S = S.masked_fill(torch.ones(nq, nq).triu(1).bool(), float("-inf"))
        o = (S.softmax(-1) @ heads(V)).transpose(1, 2).reshape(BT * nq, D)
        (o * x.dout.double()).sum().backward()
        assert torch.allclose(o, ref.out, rtol=1e-12, atol=1e-14)
        assert torch.allclose(q.grad * 0.125, ref.dq, rtol=1e-10, atol=1e-13)
        assert torch.allclose(k.grad, ref.dk, rtol=1e-10, atol=1e-13) and torch.allclose(v.grad, ref.dv, rtol=1e-10, atol=1e-13)
        if c.side:
            tot = ar.sum_side_partials(c, ref.dside)
            rows = [tot["global"]] + [tot[f"local{i}"] for i in range(BT // c.T)]
            assert torch.allclose(torch.cat(rows), s.grad[:c.G + BT], rtol=1e-10, atol=1e-13)
            if c.has_summary:
                assert torch.allclose(torch.cat([tot[f"summary{i}"] for i in range(BT // c.T)]), s.grad[c.G + BT:], rtol=1e-10, atol=1e-13)
            else:
                assert not s.grad[c.G + BT:].any()
    c = ar.vision(4, 2, 3, 21)
    x = inputs(c, "randn", F16)
    old = ar.ref_attention(x.q.view(4, 21, 128), x.k.view(4, 21, 128), x.v.view(4, 21, 128), x.side, 4, 2, 3, 21, 2, 21)
    assert torch.allclose(old.view(-1, 128), ar.reference(c, x).out, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("c", ar.FWD_ALL, ids=ar.case_id)
def test_forward_emulation_within_half_the_bound(c):
    for regime in ar.forward_regimes(c):
        for prec in (F16, BF16):
            x = inputs(c, regime, prec)
            emu = ar.emulate_forward(c, x, prec)
            assert torch.isfinite(emu.float()).all()
            r = ar.forward_ratio(c, emu, ar.reference(c, x), prec)
            assert r <= FWD_SHARE, (regime, ar.PREC_NAME[prec], r)


@pytest.mark.parametrize("c", ar.BWD_ALL, ids=ar.case_id)
def test_backward_emulation_within_its_share(c):
    for regime in ar.backward_regimes(c):
        for prec, act in ar.BWD_PRECS:
            if c.causal and prec != act or ar.backward_dropped(c, regime, prec):
                continue
            x = inputs(c, regime, prec, act)
            ratios = ar.backward_ratios(c, ar.emulate_backward(c, x, prec), ar.reference(c, x, backward=True), prec, regime)
            assert max(ratios.values()) <= BWD_SHARE, (regime, ar.PREC_NAME[prec], ratios)


def unique(cases):
    seen, out = set(), []
    for c in cases:
        key = c._replace(split=False)
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


# the regime a mutation is shown in: the gather ones also where the wrong row is an O(1) error by construction
MUT_REGIMES = {"drop_last": ("ramp",), "neighbour_local": ("randn", "hot_side"), "neighbour_summary": ("randn", "hot_side")}


@pytest.mark.parametrize("mutation", ar.MUTATIONS)
def test_mutated_forward_reference_violates_the_bound(mutation):
    """(drop_last is shown in the `ramp` regime only, where the last key carries the maximum: among 320 randn keys one key
    less is inside the bound, which is why it does not count as a requirement.)"""
    n = 0
    for c in unique(ar.FWD_ALL):
        if not ar.mutation_applies(c, mutation):
            continue
        for regime in MUT_REGIMES.get(mutation, ("randn",)):
            if regime not in ar.forward_regimes(c):                 # only where the GPU test runs it
                continue
            for prec in (F16, BF16):
                x = inputs(c, regime, prec)
                ref = ar.reference(c, x)
                r = ar.forward_ratio(c, ar.reference(c, x, mutate=mutation).out, ref, prec)
                assert r > MUT_FWD, (ar.case_id(c), regime, ar.PREC_NAME[prec], r)
                n += 1
    assert n >= 4


@pytest.mark.parametrize("mutation", ar.MUTATIONS)
def test_mutated_backward_reference_violates_the_bound(mutation):
    n = 0
    for c in unique(ar.BWD_ALL):
        if not ar.mutation_applies(c, mutation):
            continue
        for regime in MUT_REGIMES.get(mutation, ("randn",)):
            if regime not in ar.backward_regimes(c):
                continue
            for prec in (F16, BF16):
                x = inputs(c, regime, prec)
                ref = ar.reference(c, x, backward=True)
                m = ar.reference(c, x, backward=True, mutate=mutation)
                ratios = ar.backward_ratios(c, (m.dq, m.dk, m.dv, m.dside), ref, prec, regime)
                assert max(ratios.values()) > MUT_BWD, (ar.case_id(c), regime, ar.PREC_NAME[prec], ratios)
                n += 1
    assert n >= 4


def test_tables_reach_every_forward_instantiation():
    hit = {}
    for c, regime, prec in ar.forward_params():
        form = ar.forward_form(ar.n_keys(c), ar.n_queries(c), c.causal, c.split, prec)
        assert form is not None, ar.case_id(c)
        hit.setdefault(form, ar.case_id(c))
    missing = ar.forward_forms_all() - set(hit)
    assert not missing, sorted(missing)
    assert set(hit) <= ar.forward_forms_all()
    assert len(ar.forward_forms_all()) == 26 and len(ar.PERSISTENT_FORMS) == 2   # + the persistent kernel, covered elsewhere
    # the thresholds themselves
    f = lambda keys, nq, causal=False, split=False: ar.forward_form(keys, nq, causal, split, F16)
    assert f(32, 32) == "attn<f16,2,one>" and f(33, 33) == "attn<f16,6,one>" and f(96, 96) == "attn<f16,6,one>"
    assert f(97, 97) == "attn<f16,14,pair,full6>" and f(224, 224) == "attn<f16,14,pair,full13>"
    assert f(225, 225) == "attn<f16,20,pair,full14>" and f(305, 305) == f(320, 320) == "attn<f16,20,pair,full19>"
    assert f(304, 304) == "attn<f16,20,pair,full14>" and f(321, 321) == "stream<f16>" and f(321, 1, causal=True) is None
    assert f(298, 63) == "attn<f16,20,one>" and f(298, 64) == "attn<f16,20,pair,full14>" and f(305, 305, split=True) == "attn<f16,20,one>"


def test_tables_reach_every_backward_instantiation():
    hit = set()
    for c, regime, prec, act in ar.backward_params():
        forms = ar.backward_forms(ar.n_keys(c), ar.n_queries(c), c.causal, prec, act)
        assert forms is not None, ar.case_id(c)
        hit |= set(forms)
    missing = ar.backward_forms_all() - hit
    assert not missing, sorted(missing)
    assert len(ar.backward_forms_all()) == 2 * 8 + 3 * 10
    b = lambda keys, nq, causal=False: ar.backward_forms(keys, nq, causal, BF16, BF16)
    assert b(320, 320) == ("dq20<bf16,bf16,full>", "dkv_stream<bf16,bf16,full>")
    assert b(321, 288) == ("dq_stream<bf16,bf16,full>", "dkv18<bf16,bf16,full>")
    assert b(288, 288, True) == ("dq20<bf16,bf16,causal>", "dkv18<bf16,bf16,causal>") and b(289, 289, True) is None
    assert ar.backward_forms(77, 77, True, BF16, F16) is None


def test_the_dropped_backward_pair_has_no_relative_bound():
    """`peaked` with fp16 gradients on the CLS-only shapes is the one pair the tables leave out: the emulation's prompt-row
    gradients are all zero there.  The same shapes stay within their share in bf16."""
    c = next(c for c in ar.BWD_CLS if "peaked" in ar.backward_regimes(c))
    assert ar.backward_dropped(c, "peaked", F16) and not ar.backward_dropped(c, "peaked", BF16)
    x = inputs(c, "peaked", F16)
    ratios = ar.backward_ratios(c, ar.emulate_backward(c, x, F16), ar.reference(c, x, backward=True), F16, "peaked")
    assert ratios["dside"] > 100
    x = inputs(c, "peaked", BF16)
    ratios = ar.backward_ratios(c, ar.emulate_backward(c, x, BF16), ar.reference(c, x, backward=True), BF16, "peaked")
    assert max(ratios.values()) <= BWD_SHARE
