"""CPU checks of the GEMM edge tests' reference side (gemm_ref.py): the reference against plain fp64 torch formulas, the exact
regimes' exactness, every mutation outside the check, the once-rounded reference inside every bound, the walk restatement
visiting every tile once, and the case tables reaching every instantiation and walk branch of gemm.hip's dispatchers."""
import pytest
import torch
import torch.nn.functional as Fn

import gemm_ref as gr
from gemm_ref import BF16, F16, F32, F64, H16, K256, PAIR, PATCH, PP, QGELU, QGELU_BWD, Case

PRECS = [F16, BF16]
CPU_BUDGET = 3e8          # M N K of the cases whose reference the CPU tests evaluate


def small(c):
    return c.M * c.N * c.K * (2 if c.w_lo else 1) <= CPU_BUDGET


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_reference_agrees_with_plain_formulas(prec):
    """Each epilogue of the reference against the formula one would write down with torch.nn.functional, in fp64."""
    lin = lambda x, b=None: Fn.linear(x.A.to(F64), x.W.to(F64), None if b is None else b.to(F64))
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    c = Case(300, 256, 128, H16, prec, regime="randn")
    x = gr.make_inputs(c)
    want = lin(x, x.bias)
    want[:, :128] *= 0.125
    assert close(gr.reference(c, x)["out"], want)
    c = Case(300, 256, 128, QGELU, prec, regime="randn", aux_out=True)
    x = gr.make_inputs(c)
    pre = lin(x, x.bias)
    r = gr.reference(c, x)
    assert close(r["out"], pre * torch.sigmoid(1.702 * pre)) and close(r["aux_out"], pre)
    got = gr.ideal_outputs(c._replace(split=True, aux_out=False), x, r)                 # split rows: hi + lo carries the fp32 value
    assert torch.equal(got["hi"], r["out"].float().to(gr.DTYPE[prec]))
    assert torch.equal(got["lo"], (r["out"].float() - got["hi"].float()).to(gr.DTYPE[prec]))
    for resid in (0, 1, 2):
        c = Case(300, 512, 192, F32, prec, resid=resid, producer=2, regime="randn")
        x = gr.make_inputs(c)
        want = lin(x, x.bias) + (x.resid.to(F64) if resid else 0)
        r = gr.reference(c, x)
        assert close(r["out"], want)
        assert close(r["rowsum"][:, 1, 0], want[:, 256:].sum(1)) and close(r["rowsum"][:, 0, 1], want[:, :256].pow(2).sum(1))
    c = Case(300, 256, 128, F32, prec, w_lo=1, bias=False, regime="randn")               # [W_hi | W_lo]: the k-loop runs 2K deep over A twice
    x = gr.make_inputs(c)
    assert close(gr.reference(c, x)["out"], Fn.linear(torch.cat([x.A, x.A], 1).to(F64), x.W.to(F64)))
    c = Case(16 * 7, 256, 64, PATCH, prec, regime="randn")
    x = gr.make_inputs(c)
    want = lin(x, x.bias).view(7, 16, 256) + x.pos[1:].to(F64) + x.time.to(F64)[torch.tensor([0, 1, 2, 0, 1, 2, 0])][:, None]
    assert close(gr.reference(c, x)["out"], want.view(-1, 256))
    c = Case(300, 256, 64, QGELU_BWD, prec, bias=False, regime="randn")
    x = gr.make_inputs(c)
    a = x.aux.to(F64).requires_grad_()
    (a * torch.sigmoid(1.702 * a)).sum().backward()
    assert close(gr.reference(c, x)["out"], lin(x) * a.grad)
    # the folded consumers: LayerNorm (gamma = 1, beta = 0) of the stream, then the linear layer; the statistics the reference
    # takes from its fp32 inputs agree with the rows' own to fp32 rounding
    for fold in ("stats", "partials"):
        c = Case(300, 256, 512, H16, prec, bias=False, fold=fold, regime="randn")
        x = gr.make_inputs(c)
        want = Fn.linear(Fn.layer_norm(x.A.to(F64), (512,), eps=1e-5), x.W.to(F64), x.ft.to(F64))
        want[:, :128] *= 0.125
        r = gr.reference(c, x)
        assert torch.allclose(r["out"], want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_exact_regimes_are_exactly_representable():
    """ints / onehot: every fp32 output of the reference is an fp32 number, every partial sum stays below 2^24 in the units of
    the operands' last bit, and the producers' sums of squares stay below 2^24."""
    n = 0
    for c in gr.ALL_CASES:
        if c.regime not in gr.EXACT_REGIMES or not small(c) or c.fold or c.epi == QGELU_BWD:
            continue
        x = gr.make_inputs(c)
        r = gr.reference(c, x)
        unit = 1.0 if c.regime == "ints" else 2.0 ** -12           # onehot: W in 1/64ths, one product per row: sums of 1/64 and 1/8
        assert float(r["mag"].max()) / unit < 2 ** 24, gr.case_id(c)
        for name in (("pre",) if c.epi == QGELU else ("out", "pre")):     # QuickGELU: its pre-activation copy is the exact output
            assert torch.equal(r[name], r[name].float().to(F64)), (gr.case_id(c), name)
        if c.producer and c.regime == "ints":
            assert float(r["rowsum"][..., 1].max()) < 2 ** 24, gr.case_id(c)
        n += 1
    assert n >= 100


# ---------------------------------------------------------------------------------------------------------------------
# Which regimes must catch which mutation, and why the others need not:
#   drop_k, double_k   a 64-deep slice of one tile.  ints: the slice's integer sum is non-zero for all but a handful of elements.
#                      randn / offset / tiny: the slice is 1 / nk of |A|.|W|^T, the bound allows 2^-18 of it.  onehot: caught
#                      where the rows of the tile reach into the slice (k(m) = (7 m + 3) mod K sweeps all k within K rows); a
#                      tile with fewer rows than that need not.
#   swap16             every regime: neighbouring 16-column groups differ in W (and bias).
#   bias_neighbour     every regime with a bias that differs from column to column; `tiny` has a zero bias and need not.
#   resid_twice        every regime with a residual; `tiny` has a zero residual and need not.
#   row_shift          every regime: the check is on the poison outside the rows, not on values.
#   truncate           16-bit outputs.  ints: the bias of +-3000 pushes results past the exact integers of the type.  randn /
#                      offset: truncation errs by up to 2 eps, the bound allows eps plus 2^-18 mag.  onehot need not: with fp16
#                      every result is representable.  fp32 outputs are exact sums there, nothing is rounded.
#   last_tile_is_first every regime: a tile's outputs keep the poison.
ALL_R = ("ints", "onehot", "randn", "offset", "tiny")
EXPECT = {"drop_k": ALL_R, "double_k": ALL_R, "swap16": ALL_R, "bias_neighbour": ("ints", "onehot", "randn", "offset"),
          "resid_twice": ("ints", "onehot", "randn", "offset"), "truncate": ("ints", "randn", "offset"),
          "last_tile_is_first": ALL_R}


def mutation_cases(mutation, prec):
    f32 = Case(gr.m_of(9, 1), 256, 128, F32, prec, K256, 8, resid=1)          # nine tiles on eight workgroups, last tile 129 rows
    h16 = Case(gr.m_of(9, 1), 256, 128, H16, prec, K256, 8)
    pair = Case(gr.m_of(17, 1, 128), 256, 128, F32, prec, PAIR, 8, resid=2)
    tile = Case(2148, 128, 128, F32, prec, resid=1)                          # ring depth 2; 100 rows in the last tile (see onehot above)
    if mutation == "truncate":
        return [h16, h16._replace(split=True), Case(gr.m_of(9, 1), 256, 128, QGELU, prec, K256, 8, aux_out=True)]
    if mutation == "resid_twice":
        return [f32, pair, tile]
    if mutation == "last_tile_is_first":
        return [f32, h16, pair]
    return [f32, h16, pair, tile, h16._replace(w_lo=1, kernel=PP), Case(16 * 137, 256, 128, PATCH, prec, K256, 8)]


@pytest.mark.parametrize("prec", PRECS, ids=["f16", "bf16"])
@pytest.mark.parametrize("mutation", [m for m in gr.MUTATIONS if m != "row_shift"])
def test_every_mutation_falls_outside_the_check(mutation, prec):
    for base in mutation_cases(mutation, prec):
        for regime in EXPECT[mutation]:
            c = base._replace(regime=regime)
            x = gr.make_inputs(c)
            ref = gr.reference(c, x)
            good = gr.ideal_outputs(c, x, ref)
            assert gr.passes(gr.compare(c, x, ref, good)), (gr.case_id(c), "the unmutated reference fails")
            if mutation == "truncate":
                bad = gr.ideal_outputs(c, x, ref, "truncate")
            elif mutation == "last_tile_is_first":
                bad = gr.mutate_outputs(c, good, mutation)
            else:
                bad = gr.ideal_outputs(c, x, gr.reference(c, x, mutation))
            res = gr.compare(c, x, ref, bad)
            assert not gr.passes(res), (gr.case_id(c), mutation, res)


def test_row_shift_is_caught_by_the_poison():
    """Row M - 1 also written to row M: the value checks cannot see it, the check on what lies outside the rows does."""
    c = Case(300, 256, 64, F32, F16, regime="ints")
    x = gr.make_inputs(c)
    out = gr.ideal_outputs(c, x, gr.reference(c, x))["out"]
    buf = torch.full((c.M + 3, c.N + 8), float("nan"))
    buf[:c.M, :c.N] = out
    assert gr.untouched_violations(buf, c.M, c.N) == 0
    buf[c.M, :c.N] = buf[c.M - 1, :c.N]
    assert gr.untouched_violations(buf, c.M, c.N) == c.N
    buf[c.M] = float("nan")
    buf[5, c.N] = 0.0                                              # and a store into the pad columns
    assert gr.untouched_violations(buf, c.M, c.N) == 1


def test_rounded_reference_is_inside_every_bound():
    """The fp64 reference rounded once to the output type - the best a kernel can do - passes every case's check, exact or
    bounded; the worst ratio per output type is printed.  A 16-bit output sits at 1 - (the accumulation term's share) at its
    worst element by construction: e_out is the largest relative error of one rounding."""
    worst = {}
    n = 0
    for c in gr.ALL_CASES:
        if not small(c) or (c.regime in gr.EXACT_REGIMES and n % 3):  # every bounded case, a third of the exact ones
            n += 1
            continue
        n += 1
        x = gr.make_inputs(c)
        ref = gr.reference(c, x)
        res = gr.compare(c, x, ref, gr.ideal_outputs(c, x, ref))
        assert gr.passes(res), (gr.case_id(c), res)
        key = (gr.family(c), "f32" if gr.out_is_f32(c) else gr.PREC_NAME[c.prec])
        worst[key] = max(worst.get(key, 0.0), gr.worst(res))
    for key, v in sorted(worst.items()):
        print(f"rounded reference, worst error / bound, {key[0]:10s} {key[1]:5s}: {v:.3f}")
        assert v <= 1


# ---------------------------------------------------------------------------------------------------------------------
def every_tile_once(g):
    seen = sorted(t for tiles in gr.walk(g) for t in tiles)
    return seen == [(m, n) for m in range(g.tiles_m) for n in range(g.tiles_n)]


def test_walk_visits_every_tile_exactly_once():
    """The restated walk over every persistent case of the tables, and over a sweep of tile grids on 8 ... 256 workgroups in
    both walks."""
    n = 0
    for c in gr.ALL_CASES:
        name = gr.route(c)
        if "g256" in name or "pair" in name:
            assert every_tile_once(gr.persistent_grid(c, pair="pair" in name)), gr.case_id(c)
            n += 1
    assert n > 250
    aligned = 0
    for tm in range(1, 31):
        for tn in range(1, 10):
            for wg in (8, 16, 32, 64, 256):
                for epi in (F32, H16):
                    g = gr.persistent_grid(Case(256 * tm, 256 * tn, 64, epi, F16, K256, wg))
                    assert every_tile_once(g), g
                    aligned += g.align
    assert aligned > 100


# (tiles_m, tiles_n, workgroups) -> the walk branches the issue's table claims for the fp32-output kernels
CLAIMS = {(9, 1, 8): {"aligned sm=1", "tiles/wg=2"}, (9, 4, 32): {"aligned sm=1", "tiles/wg=2"},
          (17, 1, 16): {"aligned sm=2", "aligned short last m-range", "tiles/wg=2"},
          (17, 2, 32): {"aligned sm=2", "aligned short last m-range", "tiles/wg=2"},
          (25, 3, 64): {"aligned sm=2", "aligned short last m-range", "tiles/wg=2"},
          (5, 8, 32): {"aligned sm=1", "aligned two column chunks"},
          (3, 5, 8): {"plain", "plain tiles_n % sn"}, (2, 9, 8): {"plain", "plain tiles_n % sn", "tiles/wg=3"},
          (3, 6, 16): {"plain", "plain tiles_n % sn"},
          (9, 4, 8): {"plain", "plain short last m-group", "tiles/wg=5"}, (11, 3, 8): {"plain", "plain short last m-group"},
          (3, 3, 8): {"plain", "tiles/wg=2"}, (3, 3, 16): {"plain", "idle workgroups"}}


def test_tables_reach_every_instantiation_and_walk_branch():
    """The tables through the route restatement with n_cu = 256: every instantiation launch_prec, launch_256 and launch_pair can
    launch in the default environment (w_lo <= 1, no 16-bit residual pair) is reached, by name, and so is every walk branch."""
    names = gr.all_instantiations()
    assert len(names) == len(set(names)) == gr.N_INSTANTIATIONS == 74
    reached = {}
    for c in gr.ALL_CASES:
        r = gr.route(c)
        assert r != gr.EINVAL, gr.case_id(c)
        reached.setdefault(r, []).append(c)
    assert sorted(reached) == sorted(names), (set(names) - set(reached), set(reached) - set(names))
    for (tm, tn, wg), tags in CLAIMS.items():
        for r in range(3):
            g = gr.persistent_grid(Case(gr.m_of(tm, r), 256 * tn, 64, F32, F16, K256, wg))
            assert tags <= gr.walk_classes(g), ((tm, tn, wg), gr.walk_classes(g))
    # each walk class with the minimum and minimum + 1 k-tile count of both loops, ping-pong with w_lo = 1 at K = 128, both types
    seen = set()
    for c in gr.WALKS:
        g = gr.persistent_grid(c)
        assert (g.tiles_m, g.tiles_n, c.avail) in CLAIMS
        assert ("PP=1" in gr.route(c)) == (c.kernel == PP)
        if c.epi == F32:
            assert CLAIMS[(g.tiles_m, g.tiles_n, c.avail)] <= gr.walk_classes(g), gr.case_id(c)
        seen.add(((g.tiles_m, g.tiles_n, c.avail), c.kernel, c.K, c.w_lo, c.prec))
    assert len(seen) == len(CLAIMS) * len(gr.LOOPS) * 2
    # the fold block's parity: one, two and three tiles on a workgroup, both statistics forms, both loops
    fold = {(max(len(t) for t in gr.walk(gr.persistent_grid(c))), c.fold, c.kernel) for c in gr.FOLDS if c.fold}
    assert fold == {(n, f, k) for n in (1, 2, 3) for f in ("stats", "partials") for k in (K256, PP)}
    assert {c.K for c in gr.FOLDS if c.fold == "partials"} == {256, 1024}
    pair = {max(len(t) for t in gr.walk(gr.persistent_grid(c, pair=True))) for c in gr.PAIRS}
    assert pair >= {2, 3}
    assert max(c.M * c.N for c in gr.ALL_CASES) <= 6.6e6 and all(c.K <= 3072 and (c.K < 3072 or c.M <= 600) for c in gr.ALL_CASES)


def test_route_rejects_what_the_library_rejects():
    """The reject paths the tables brush (the GPU test makes the same calls)."""
    assert gr.route(Case(600, 256, 192, H16, F16, PP, 8)) == gr.EINVAL                       # K % 128
    assert gr.route(Case(600, 256, 256, H16, F16, K256, 8, bias=False, split=True, fold="partials")) == gr.EINVAL
    assert gr.route(Case(600, 256, 128, H16, F16, PP, 8)) == gr.EINVAL                       # ping-pong below four k-tiles
    assert gr.route(Case(600, 256, 128, H16, F16, PP, 8, w_lo=1)) != gr.EINVAL               # ... which w_lo = 1 doubles
    assert gr.route(Case(600, 256, 256, QGELU, F16, PP, 8)) == gr.EINVAL                     # no plain QuickGELU on the ping-pong loop
    assert gr.route(Case(600, 384, 128, F32, F16, K256, 8)) == gr.EINVAL                     # N % 256
