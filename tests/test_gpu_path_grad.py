"""GPU: integrated gradients and SmoothGrad - the four path-gradient kernels op by op against tests/path_grad_ref.py, then
VitaCLIP.integrated_gradients / smooth_grad end to end.

Op level, on synthetic data with no model, at three (size, patch, ld) so that all three vector widths run.  The bounds:
  path_clips line   exact at alpha = 0 and 1; elsewhere two fp32 roundings, 2^-23 (|x| + |x0|), against fp64 on the same fp32 alpha, beta
  path_clips noise  |z - z_ref| <= 2e-5: radius <= sqrt(48 ln 2) = 5.77 times a few ulp of logf / sqrtf / sincosf on exact 24-bit uniforms
  clip_range        exact
  unpatchify_path   (m + 8) 2^-24 S_abs element-wise, S_abs the same expression on absolute values (path_grad_ref.reduce_path)
  path_delta        2^-24 |sum| + 2^-27 sum |a|: one rounding of a double-precision sum
Model level at TINY, B = 2: the fused call against the composition of what is already pinned (path_clips + saliency(reduce=None) on
the B*m copies + the fp64 reduction: the same batch through the same kernels, so the patch gradients are the same bits and the
fold's bound applies), and against the fixture the REFERENCE produced (tests/golden/tiny_path_grads.npz) within the project's
frozen gradient criterion, 4e-2 norm-wise.  Every case prints a [path-grad] line."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402
import path_grad_ref as ref  # noqa: E402

F64 = torch.float64
U = 2.0 ** -24
GRAD_TOL = 4e-2         # the frozen norm-wise criterion of the backward's gradients (tests/test_gpu_backward.py)
#         size, P, ld, T, CLS row
SHAPES = [(64, 16, 768, 2, True),       # 16-byte accesses, the model's form
          (56, 14, 640, 3, True),       # P = 14: 588 columns in rows of 640, 8-byte accesses
          (21, 7, 149, 2, False)]       # single floats, an odd ld, the dense form
MODES = (hip.PATH_GRAD, hip.PATH_ABSMAX, hip.PATH_L2, hip.PATH_ATTR, hip.PATH_ATTR_SUM, hip.PATH_ATTR_ABS)


def note(tag, **values):
    print(f"\n[path-grad] {tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in values.items()))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1009 * int(k) for i, k in enumerate(key)))


def _baselines(x, g):
    return {"zero": None, "channel": torch.randn(3, generator=g), "tensor": torch.randn(x.shape, generator=g)}


def _alphas(m):
    if m == 1:
        return [0.37]
    if m == 2:
        return [0.0, 1.0]
    a = [k / (m - 1) for k in range(m)]
    a[1], a[5], a[m - 2] = 1.0, 0.0, 1 / 3                # the endpoints also away from the ends, and a value that is no fp32
    return a


# ---- gava_path_clips ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("m", [1, 2, 64])
def test_path_clips_line(shape, m):
    size, P, _, T, _ = shape
    g = _gen(size, m)
    x = torch.randn(2, 3, T, size, size, generator=g)
    alpha = _alphas(m)
    xd = x.cuda()
    for kind, base in _baselines(x, g).items():
        bd = base.cuda() if base is not None else None
        out = hip.path_clips(xd, patch=P, alpha=alpha, baseline=bd)
        assert out.shape == (2, m, 3, T, size, size) and torch.equal(out, hip.path_clips(xd, patch=P, alpha=alpha, baseline=bd))
        x0 = ref.baseline_like(x, base)
        want = ref.line(x, base, alpha)
        got = out.cpu()
        for k, a in enumerate(alpha):
            if a == 0.0:
                assert torch.equal(got[:, k], x0), (kind, k)
            elif a == 1.0:
                assert torch.equal(got[:, k], x), (kind, k)
        worst = float(((got.to(F64) - want).abs() / (2 ** -23 * (x.abs() + x0.abs()).to(F64).unsqueeze(1))).max())
        note(f"line {shape} m={m} {kind}", of_bound=worst)
        assert worst <= 1
    into = torch.full((2, m, 3, T, size, size), float("nan"), device="cuda")
    assert hip.path_clips(xd, patch=P, alpha=alpha, out=into) is into and torch.equal(into, hip.path_clips(xd, patch=P, alpha=alpha))


@pytest.mark.parametrize("size,P,T", [(64, 16, 2), (56, 14, 3), (42, 7, 2)])
def test_path_clips_noise(size, P, T):
    nb, m, seed = 4, 3, 7 + (5 << 32)
    g = _gen(size, P)
    x = torch.randn(nb, 3, T, size, size, generator=g)
    sigma = torch.rand(nb, generator=g) * 1.5 + 0.5
    xd, sd = x.cuda(), sigma.cuda()
    out = hip.path_clips(xd, patch=P, sigma=sd, samples=m, seed=seed)
    n = 3 * T * size * size
    z = (out.cpu().to(F64) - x.to(F64).unsqueeze(1)).view(nb, m, n) / sigma.to(F64).view(nb, 1, 1)
    want = ref.noise(seed, 0, nb, m, n)
    err = float((z - want).abs().max())
    note(f"noise size={size} P={P}", z_err=err, mean=float(z.mean()), var=float(z.var()))
    assert err <= 2e-5
    # counter-based: the two halves generated on their own are the whole's bits; a second call repeats; another seed differs
    halves = [hip.path_clips(xd[i:i + 2], patch=P, sigma=sd[i:i + 2], samples=m, seed=seed, clip0=i) for i in (0, 2)]
    assert torch.equal(torch.cat(halves), out)
    assert torch.equal(hip.path_clips(xd, patch=P, sigma=sd, samples=m, seed=seed), out)
    assert not torch.equal(hip.path_clips(xd, patch=P, sigma=sd, samples=m, seed=seed + 1), out)
    assert not torch.equal(hip.path_clips(xd[:2], patch=P, sigma=sd[:2], samples=m, seed=seed, clip0=1), out[:2])
    assert torch.equal(hip.path_clips(xd, patch=P, sigma=torch.zeros(nb, device="cuda"), samples=2), xd.unsqueeze(1).expand(nb, 2, *x.shape[1:]))
    with pytest.raises(hip.GavaError, match="odd size"):
        hip.path_clips(torch.zeros(1, 3, 2, 21, 21, device="cuda"), patch=7, sigma=sd[:1], samples=2)


# ---- gava_clip_range ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb,T,size", [(3, 2, 64), (2, 3, 21), (1, 8, 224), (5, 1, 2)])
def test_clip_range_is_exact(nb, T, size):
    x = torch.randn(nb, 3, T, size, size, generator=_gen(nb, size)) * 3
    x[0, 2, T - 1, size - 1, size - 1] = 50.0             # the extremes in the last and the first element
    x[nb - 1, 0, 0, 0, 0] = -60.0
    xd = x.cuda()
    for r in (0.15, 1.0):
        mn, mx, sg = hip.clip_range(xd, r)
        flat = xd.view(nb, -1)
        assert torch.equal(mn, flat.amin(1)) and torch.equal(mx, flat.amax(1))
        assert torch.equal(sg, (mx - mn) * torch.tensor(r, dtype=torch.float32, device="cuda"))
    if nb > 1:                                            # a NaN takes its own clip's three values, and no other's
        xd[1, 1, 0, size // 2, 1] = float("nan")
        mn2, mx2, sg2 = hip.clip_range(xd, 1.0)
        assert bool(torch.isnan(mn2[1]) and torch.isnan(mx2[1]) and torch.isnan(sg2[1]))
        keep = [b for b in range(nb) if b != 1]
        assert torch.equal(mn2[keep], mn[keep]) and torch.equal(mx2[keep], mx[keep]) and torch.equal(sg2[keep], sg[keep])


# ---- gava_unpatchify_path -------------------------------------------------------------------------------------------------------

def _weights(m, g):
    if m == 1:
        return [-0.75]
    if m == 3:
        return [0.5, 0.0, -1.25]
    w = torch.randn(m, generator=g)
    w[[0, 7, m - 1]] = 0.0
    return w.tolist()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("m", [1, 3, 64])
def test_unpatchify_path_matches_the_restatement(shape, m):
    size, P, ld, T, cls = shape
    B, n = 2, (size // P) ** 2
    frame_rows, row_offset = (n + 1, 1) if cls else (n, 0)
    g = _gen(size, m, 3)
    w = _weights(m, g)
    # NaN in every row and column the kernel must not read - the steps of zero weight included
    dp = torch.full((B * m * T, frame_rows, ld), float("nan"))
    dp[:, row_offset:row_offset + n, :3 * P * P] = torch.randn(B * m * T, n, 3 * P * P, generator=g)
    for k, wk in enumerate(w):
        if wk == 0.0:
            dp.view(B, m, T, frame_rows, ld)[:, k] = float("nan")
    x = torch.randn(B, 3, T, size, size, generator=g)
    geo = dict(B=B, T=T, size=size, patch=P, frame_rows=frame_rows, row_offset=row_offset, w=w)
    dpd, xd = dp.cuda(), x.cuda()
    worst = {}
    for mode in MODES:
        shape_out = (B, 3, T, size, size) if mode in (hip.PATH_GRAD, hip.PATH_ATTR) else (B, T, size, size)
        for kind, base in (_baselines(x, g) if mode >= hip.PATH_ATTR else {"zero": None}).items():
            kw = dict(x=xd, baseline=base.cuda() if base is not None else None) if mode >= hip.PATH_ATTR else {}
            out = hip.unpatchify_path(dpd, torch.full(shape_out, float("nan"), device="cuda"), mode=mode, **geo, **kw)
            again = hip.unpatchify_path(dpd.view(-1, ld), torch.empty(shape_out, device="cuda"), mode=mode, **geo, **kw)
            assert bool(torch.isfinite(out).all()) and torch.equal(out, again), (mode, kind)
            want, s_abs = ref.fold_path(dp.to(F64), B, m, T, size, P, frame_rows, row_offset, w, mode, x=x, baseline=base)
            err = (out.cpu().to(F64) - want).abs()
            bound = ref.fold_bound(m, s_abs)
            assert bool((err <= bound).all()), (mode, kind, float((err / bound)[bound > 0].max()))
            worst[(mode, kind)] = float((err / bound)[bound > 0].max())
    note(f"fold {shape} m={m}", **{f"mode{k[0]}_{k[1]}": v for k, v in worst.items()})


@pytest.mark.parametrize("shape", SHAPES)
def test_unpatchify_path_of_one_copy_is_unpatchify(shape):
    size, P, ld, T, cls = shape
    B, n = 2, (size // P) ** 2
    frame_rows, row_offset = (n + 1, 1) if cls else (n, 0)
    dp = torch.randn(B * T, frame_rows, ld, generator=_gen(size, 5)).cuda()
    for mode, plain in ((hip.PATH_GRAD, hip.UNPATCH_GRAD), (hip.PATH_ABSMAX, hip.UNPATCH_ABSMAX), (hip.PATH_L2, hip.UNPATCH_L2)):
        shape_out = (B, 3, T, size, size) if mode == hip.PATH_GRAD else (B, T, size, size)
        geo = dict(B=B, T=T, size=size, patch=P, frame_rows=frame_rows, row_offset=row_offset)
        got = hip.unpatchify_path(dp, torch.empty(shape_out, device="cuda"), mode=mode, w=[1.0], **geo)
        assert torch.equal(got, hip.unpatchify(dp, torch.empty(shape_out, device="cuda"), mode=plain, **geo)), mode


# ---- gava_path_delta ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,size", [(2, 21), (3, 64), (1, 8)])
def test_path_delta(T, size):
    B, m, C = 4, 5, 5
    g = _gen(T, size, 9)
    a = torch.randn(B, T, size, size, generator=g) * torch.tensor([1.0, 1e3, 1e-3, 30.0]).view(B, 1, 1, 1)
    a[0] += 0.5                                                           # a sum well away from zero next to cancelling ones
    logits = torch.randn(B * m, 8, generator=g) * 10
    target = torch.tensor([1, 5, 4, -1])                                  # clips 1 and 3: outside [0, C)
    lg = logits.cuda()[:, :C]                                             # rows of 5 in rows of 8
    res = hip.path_delta(a.cuda(), lg, target.cuda(), m=m, k_lo=1, k_hi=3)
    again = hip.path_delta(a.cuda(), lg, target.cuda(), m=m, k_lo=1, k_hi=3)
    s64, f64, abs64 = ref.delta(a, logits[:, :C], target, m, 1, 3)
    s, fd, d = (res[k].cpu() for k in ("sum_attr", "f_diff", "delta"))
    for k in res:
        assert torch.equal(res[k].cpu().nan_to_num(nan=7.0), again[k].cpu().nan_to_num(nan=7.0)), k
    bad = torch.tensor([False, True, False, True])
    assert bool(torch.isnan(s[bad]).all() and torch.isnan(fd[bad]).all() and torch.isnan(d[bad]).all())
    ok = ~bad
    assert bool(torch.isfinite(s[ok]).all() and torch.isfinite(fd[ok]).all() and torch.isfinite(d[ok]).all())
    err = (s[ok].to(F64) - s64[ok]).abs()
    bound = 2.0 ** -24 * s64[ok].abs() + 2.0 ** -27 * abs64[ok]
    note(f"delta T={T} size={size}", of_bound=float((err / bound).max()))
    assert bool((err <= bound).all())
    rows = logits[:, :C].reshape(B, m, C)[torch.arange(B), :, target.clamp(0, C - 1)]       # [B, m]: the target's logit per step
    assert torch.equal(fd[ok], (rows[:, 3] - rows[:, 1])[ok])
    assert torch.equal(d[ok], s[ok] - fd[ok])


# ---- model level ----------------------------------------------------------------------------------------------------------------

def _model(keep=True, train=True):
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
    m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
    m = m.cuda()
    m = m.train() if train else m.eval()
    if not keep:
        m.keep_activation_bytes = 0
    return m


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_path_grads.npz"))
    return {k: torch.from_numpy(g[k]) for k in g.files}


@pytest.fixture(scope="module")
def tiny_x():
    return torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda()


def _check_fold(tag, got, g, w, mode, x=None, base=None):
    """got against the fp64 reduction of the per-copy gradients g [B, m, 3, T, S, S] (device bits), within the fold's bound."""
    want, s_abs = ref.reduce_path(g.cpu().to(F64), w, mode, x=x.cpu() if x is not None else None, baseline=base.cpu() if base is not None else None)
    err, bound = (got.cpu().to(F64) - want).abs(), ref.fold_bound(g.shape[1], s_abs)
    worst = float((err / bound)[bound > 0].max())
    note(tag, of_bound=worst)
    assert got.shape == want.shape and bool((err <= bound).all()), (tag, worst)


@pytest.mark.parametrize("keep,train", [(True, True), (False, True), (True, False)])
def test_fused_calls_are_the_composition_of_the_pinned_parts(tiny_x, keep, train):
    m = _model(keep=keep, train=train)
    P, B = TINY.patch_size, 2
    target = torch.tensor([2, 0], device="cuda")
    cases = [("trapezoid", 8, "zero", None), ("gausslegendre", 5, torch.tensor([0.3, -0.2, 0.1], device="cuda"), None),
             ("gausslegendre", 5, "blur", hip.blur_clips(tiny_x, hip.gaussian_taps(5.0).cuda()))]
    for rule, steps, baseline, blurred in cases:
        alpha, w = hip.path_rule(rule, steps)
        n = len(alpha)
        assert n == (8 if rule == "trapezoid" else 7)
        base = blurred if blurred is not None else baseline if torch.is_tensor(baseline) else None
        copies = hip.path_clips(tiny_x, patch=P, alpha=alpha, baseline=base)
        g, lg, _ = m.saliency(copies.view(B * n, *tiny_x.shape[1:]), target=target.repeat_interleave(n), reduce=None)
        g = g.view(B, n, *tiny_x.shape[1:])
        tag = f"{rule} {steps} keep={keep} train={train} base={baseline if isinstance(baseline, str) else 'channel'}"
        for multiply, reduce, mode in ((False, None, hip.PATH_GRAD), (False, "absmax", hip.PATH_ABSMAX), (False, "l2", hip.PATH_L2),
                                       (True, None, hip.PATH_ATTR), (True, "sum", hip.PATH_ATTR_SUM), (True, "abs", hip.PATH_ATTR_ABS)):
            r = m.integrated_gradients(tiny_x, target=target, baseline=baseline, steps=steps, rule=rule, reduce=reduce, multiply=multiply)
            _check_fold(f"{tag} mode={mode}", r.maps, g, w, mode, x=tiny_x, base=base)
            assert torch.equal(r.logits, lg.view(B, n, -1)[:, -1]) and torch.equal(r.target, target)
            assert r.alpha.tolist() == torch.tensor(alpha).float().tolist() and r.w.tolist() == torch.tensor(w).float().tolist()
            if not multiply:
                assert r.sum_attr is None and r.delta is None
                continue
            signed, _ = ref.reduce_path(g.cpu().to(F64), w, ref.ATTR_SUM, x=tiny_x.cpu(), baseline=base.cpu() if base is not None else None)
            s64 = signed.reshape(B, -1).sum(1)
            # the device's signed map is within the fold's bound of `signed`; its sum then rounds once
            _, s_abs = ref.reduce_path(g.cpu().to(F64), w, ref.ATTR_SUM, x=tiny_x.cpu(), baseline=base.cpu() if base is not None else None)
            slack = ref.fold_bound(n, s_abs).reshape(B, -1).sum(1) + 2.0 ** -24 * s64.abs() + 2.0 ** -27 * signed.abs().reshape(B, -1).sum(1)
            assert bool(((r.sum_attr.cpu().to(F64) - s64).abs() <= slack).all())
            f = lg.view(B, n, -1)[torch.arange(B, device="cuda"), :, target]
            assert torch.equal(r.delta, r.sum_attr - (f[:, -1] - f[:, 0]))
            note(f"{tag} reduce={reduce}", **{f"delta{b}": float(r.delta[b]) for b in range(B)}, **{f"f_diff{b}": float(f[b, -1] - f[b, 0]) for b in range(B)})
    # SmoothGrad the same way
    sg = hip.clip_range(tiny_x, 0.15)[2]
    copies = hip.path_clips(tiny_x, patch=P, sigma=sg, samples=4, seed=3)
    g, _, _ = m.saliency(copies.view(B * 4, *tiny_x.shape[1:]), target=target.repeat_interleave(4), reduce=None)
    g = g.view(B, 4, *tiny_x.shape[1:])
    with torch.no_grad():
        plain = m(tiny_x)[0] if not train else None
    for reduce, mode in ((None, hip.PATH_GRAD), ("absmax", hip.PATH_ABSMAX), ("l2", hip.PATH_L2)):
        maps, lg, tg = m.smooth_grad(tiny_x, target=target, samples=4, sigma=0.15, seed=3, reduce=reduce)
        _check_fold(f"smooth_grad keep={keep} train={train} mode={mode}", maps, g, [0.25] * 4, mode)
        assert torch.equal(tg, target) and lg.shape == (B, 3) and not lg.requires_grad and (plain is None or torch.equal(lg, plain))
    absolute = m.smooth_grad(tiny_x, target=target, samples=4, sigma=float(sg[0]), relative=False, seed=3, reduce=None)[0]
    assert torch.equal(absolute[0], m.smooth_grad(tiny_x, target=target, samples=4, sigma=0.15, seed=3, reduce=None)[0][0])


def _check_grad(tag, got, want):
    assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all()), tag
    whole, clips = rel(got.cpu(), want), [rel(got[b].cpu(), want[b]) for b in range(want.shape[0])]
    note(tag, whole=whole, **{f"clip{b}": e for b, e in enumerate(clips)})
    assert whole <= GRAD_TOL and max(clips) <= GRAD_TOL, (tag, whole, clips)


@pytest.mark.parametrize("keep", [True, False])
def test_against_the_reference(gold, tiny_x, keep):
    """delta is reported and not bounded: it is the trapezoid's discretisation error at 8 steps plus the bf16 gradient operands',
    and the reference's own residual (the fixture's sum_attr - (f_x - f_x0)) is printed next to it."""
    m = _model(keep=keep)
    target = gold["target"].cuda()
    r = m.integrated_gradients(tiny_x, target=target, steps=8, reduce=None, multiply=False)
    _check_grad(f"path-mean gradient {'kept' if keep else 'recompute'} vs reference", r.maps, gold["ig_mean_grad"])
    a = m.integrated_gradients(tiny_x, target=target, steps=8)
    assert r.sum_attr is None and torch.equal(a.logits, r.logits) and a.maps.shape == (2, TINY.num_frames, TINY.input_size, TINY.input_size)
    xn = tiny_x.cpu().double().reshape(2, -1).norm(dim=1)                  # x0 = 0
    gn = gold["ig_mean_grad"].double().reshape(2, -1).norm(dim=1)
    err = (a.sum_attr.cpu().double() - gold["ig_sum_attr"]).abs()
    note("sum_attr vs reference", **{f"clip{b}": float(err[b] / (xn[b] * gn[b])) for b in range(2)})
    assert bool((err <= GRAD_TOL * xn * gn).all())
    assert torch.equal(a.alpha, gold["ig_alpha"].float()) and torch.equal(a.w, gold["ig_w"].float())      # the same path
    # both endpoints' logits within 1e-3 of their own largest: x is the call's `logits`; x0 = 0 is the alpha = 0 row, read here
    # from the same grad-enabled forward on the zero clips, and once more as the f(x0) the residual was formed with
    scale, scale0 = float(gold["ig_logits_x"].abs().max()), float(gold["ig_logits_x0"].abs().max())
    lg0 = m.saliency(torch.zeros_like(tiny_x), target=target)[1].cpu()
    f_x = a.logits.cpu().gather(1, gold["target"].view(-1, 1)).squeeze(1)
    f_diff = a.sum_attr.cpu() - a.delta.cpu()
    e_x, e_x0 = float((a.logits.cpu() - gold["ig_logits_x"]).abs().max()), float((lg0 - gold["ig_logits_x0"]).abs().max())
    e_f0 = float(((f_x - f_diff) - gold["ig_f_x0"]).abs().max())
    note("endpoint logits vs reference", x=e_x / scale, x0=e_x0 / scale0, f_x0=e_f0 / scale0)
    assert e_x <= 1e-3 * scale and e_x0 <= 1e-3 * scale0 and e_f0 <= 1e-3 * scale0
    ref_delta = gold["ig_sum_attr"] - (gold["ig_f_x"].double() - gold["ig_f_x0"].double())
    note("completeness residual", **{f"delta{b}": float(a.delta[b]) for b in range(2)}, **{f"reference{b}": float(ref_delta[b]) for b in range(2)},
         **{f"f_diff{b}": float(f_diff[b]) for b in range(2)})
    maps, _, _ = m.smooth_grad(tiny_x, target=target, samples=4, sigma=0.15, seed=7, reduce=None)
    _check_grad(f"SmoothGrad mean gradient {'kept' if keep else 'recompute'} vs reference", maps, gold["sg_mean_grad"])
    assert torch.equal(hip.clip_range(tiny_x, 0.15)[2].cpu(), gold["sg_sigma"])


def _count_syncs(fn):
    fn()                                        # warm-up: packs, workspaces, the side stream
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return len([w for w in caught if "synchroniz" in str(w.message).lower()])


@pytest.mark.parametrize("train", [True, False])
def test_interface(tiny_x, train):
    m = _model(train=train)
    B = 2
    with torch.no_grad():                       # the calls enable grad for themselves
        auto = m.integrated_gradients(tiny_x, steps=4)
        sg_auto = m.smooth_grad(tiny_x, samples=4)
    top1 = auto.logits.argmax(1)
    assert auto.target.dtype == torch.int64 and torch.equal(auto.target, top1) and torch.equal(sg_auto[2], sg_auto[1].argmax(1))
    explicit = m.integrated_gradients(tiny_x, target=top1, steps=4)
    for k in ("maps", "logits", "target", "sum_attr", "delta"):
        assert torch.equal(getattr(auto, k), getattr(explicit, k)), k
    assert torch.equal(sg_auto[0], m.smooth_grad(tiny_x, target=sg_auto[2], samples=4)[0])
    one = m.integrated_gradients(tiny_x, target=1, steps=4)
    assert one.target.tolist() == [1, 1] and torch.equal(one.maps, m.integrated_gradients(tiny_x, target=torch.tensor([1, 1], device="cuda"), steps=4).maps)
    assert not auto.maps.requires_grad and not auto.logits.requires_grad and tiny_x.grad is None and not tiny_x.requires_grad
    # two chunks (max_clips = m: one clip at a time) against one: the same maps within the fold's bound, the same noise
    alpha, w = hip.path_rule("trapezoid", 4)
    copies = hip.path_clips(tiny_x, patch=TINY.patch_size, alpha=alpha)
    g = m.saliency(copies.view(B * 4, *tiny_x.shape[1:]), target=top1.repeat_interleave(4), reduce=None)[0].view(B, 4, *tiny_x.shape[1:])
    whole = m.integrated_gradients(tiny_x, target=top1, steps=4, reduce=None, multiply=False, max_clips=64)
    cut = m.integrated_gradients(tiny_x, target=top1, steps=4, reduce=None, multiply=False, max_clips=4)
    _check_fold("one chunk", whole.maps, g, w, hip.PATH_GRAD)
    _check_fold("two chunks", cut.maps, g, w, hip.PATH_GRAD)
    bound = ref.fold_bound(4, ref.reduce_path(g.cpu().to(F64), w, ref.GRAD)[1])
    assert bool(((cut.maps.cpu().to(F64) - whole.maps.cpu().to(F64)).abs() <= bound).all()) and torch.equal(cut.target, whole.target)
    cut_auto = m.integrated_gradients(tiny_x, steps=4, max_clips=1)
    assert torch.equal(cut_auto.target, top1) and cut_auto.sum_attr.shape == (B,) and bool(torch.isfinite(cut_auto.delta).all())
    noisy = hip.path_clips(tiny_x, patch=TINY.patch_size, sigma=hip.clip_range(tiny_x, 0.15)[2], samples=4, seed=5)
    gs = m.saliency(noisy.view(B * 4, *tiny_x.shape[1:]), target=top1.repeat_interleave(4), reduce=None)[0].view(B, 4, *tiny_x.shape[1:])
    sg_whole = m.smooth_grad(tiny_x, target=top1, samples=4, seed=5, reduce=None)[0]
    sg_cut = m.smooth_grad(tiny_x, target=top1, samples=4, seed=5, reduce=None, max_clips=4)[0]
    _check_fold("smooth_grad one chunk", sg_whole, gs, [0.25] * 4, hip.PATH_GRAD)
    _check_fold("smooth_grad two chunks", sg_cut, gs, [0.25] * 4, hip.PATH_GRAD)
    bound = ref.fold_bound(4, ref.reduce_path(gs.cpu().to(F64), [0.25] * 4, ref.GRAD)[1])
    assert bool(((sg_cut.cpu().to(F64) - sg_whole.cpu().to(F64)).abs() <= bound).all())
    assert not torch.equal(sg_whole, m.smooth_grad(tiny_x, target=top1, samples=4, seed=6, reduce=None)[0])
    # max_clips = 1: the plain forward behind `logits` and the top-1 target runs one clip at a time too, and changes no bit
    _, lg_one, tg_one = m.smooth_grad(tiny_x, samples=1, max_clips=1)
    _, lg_all, tg_all = m.smooth_grad(tiny_x, samples=1)
    assert torch.equal(lg_one, lg_all) and torch.equal(tg_one, tg_all) and lg_one.shape == (B, 3)
    # no parameter gradient, nothing kept
    assert all(p.grad is None for p in m.parameters())
    del auto, sg_auto, explicit, one, whole, cut, cut_auto, sg_whole, sg_cut, copies, g, gs, noisy
    for call in (lambda: m.integrated_gradients(tiny_x, steps=4, reduce="abs"), lambda: m.smooth_grad(tiny_x, samples=4)):
        call()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = call()
        del out
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    assert all(p.grad is None for p in m.parameters())


def test_path_calls_add_no_host_synchronisation(tiny_x):
    m = _model()
    target = torch.tensor([0, 2], device="cuda")

    def plain():
        for p in m.parameters():
            p.grad = None
        m(tiny_x)[0].gather(1, target.view(-1, 1)).sum().backward()

    n_plain = _count_syncs(plain)
    counts = dict(ig=_count_syncs(lambda: m.integrated_gradients(tiny_x, target=target, steps=4)),
                  ig_top1_blur_chunks=_count_syncs(lambda: m.integrated_gradients(tiny_x, steps=4, baseline="blur", reduce="abs", max_clips=4)),
                  sg=_count_syncs(lambda: m.smooth_grad(tiny_x, target=target, samples=4)),
                  sg_top1=_count_syncs(lambda: m.smooth_grad(tiny_x, samples=4, max_clips=4)))
    print(f"\n[path-grad] host synchronisations: forward + backward {n_plain}, " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    assert all(v <= n_plain for v in counts.values()), (n_plain, counts)


def test_faithfulness_takes_the_two_new_methods(tiny_x):
    m = _model(train=False)
    with torch.no_grad():
        f = m.faithfulness(tiny_x, methods=("saliency", "integrated", "smoothgrad"), steps=3, seed=4)
        assert list(f) == ["saliency", "integrated", "smoothgrad", "random"]
        target = f["saliency"]["deletion"].target
        maps = dict(saliency=m.saliency(tiny_x, target)[0], integrated=m.integrated_gradients(tiny_x, target).maps,
                    smoothgrad=m.smooth_grad(tiny_x, target)[0])
        for name, s in maps.items():
            for mode in ("deletion", "insertion"):
                want = m.perturbation_curves(tiny_x, s, mode=mode, target=target, steps=3)
                for k in ("logit", "prob", "top1", "auc_logit", "auc_prob", "target", "ranks"):
                    assert torch.equal(getattr(f[name][mode], k), getattr(want, k)), (name, mode, k)
        assert list(m.faithfulness(tiny_x, steps=2)) == ["rollout", "relevance", "saliency", "random"]
