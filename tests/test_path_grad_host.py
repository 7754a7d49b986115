"""CPU: the host side of integrated gradients and SmoothGrad (the "path gradients" section of include/gava_hip.h).

The restatement (tests/path_grad_ref.py) is pinned first: its Philox4x32-10 to the Random123 known answers, its Box-Muller to the
moments of a normal, its weighted fold to fp64 autograd of a path integral through a Conv2d(3, D, P, stride=P).  Then the
quadrature rules of hip.path_rule, the C ABI's surface (names, struct mirrors, the argument checks that return before any
launch) and every refusal of the wrappers and of the two model methods that needs no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gava_clip_amd.config import TINY
from helpers import REPO
import path_grad_ref as ref

NAMES = ("gava_path_clips", "gava_clip_range", "gava_unpatchify_path", "gava_path_delta", "gava_path_grad_struct_sizes")
STRUCTS = ("gava_path_clips_args", "gava_clip_range_args", "gava_unpatchify_path_args", "gava_path_delta_args")


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_reproduces_the_random123_known_answers(ctr, key, want):
    assert tuple(int(v) for v in ref.philox4x32_10(ctr, key)) == want
    # and as arrays: every element is the scalar answer
    got = ref.philox4x32_10([np.full(5, c, dtype=np.uint64) for c in ctr], key)
    assert all((g == w).all() for g, w in zip(got, want))


def test_normals_are_counter_based_and_normal():
    n = 1 << 16
    z = ref.normals(7, 3, 2, n)
    assert z.shape == (n,) and np.isfinite(z).all()
    assert abs(z.mean()) < 4 / n ** 0.5 and abs(z.var() - 1) < 4 * (2 / n) ** 0.5 and abs((z ** 4).mean() - 3) < 0.15
    assert np.abs(z).max() <= (48 * np.log(2)) ** 0.5                    # u1 >= 2^-24
    assert (ref.normals(7, 3, 2, 64) == z[:64]).all()                    # an element's value does not depend on how many are drawn
    for other in (ref.normals(8, 3, 2, 64), ref.normals(7, 4, 2, 64), ref.normals(7, 3, 1, 64), ref.normals(7 + (1 << 32), 3, 2, 64)):
        assert (other != z[:64]).any()
    full = ref.noise(7, 0, 4, 2, 64)
    assert torch.equal(torch.cat([ref.noise(7, 0, 2, 2, 64), ref.noise(7, 2, 2, 2, 64)]), full)
    # the extreme words: u1 = 1 gives radius 0, u1 = 2^-24 the largest one
    z0, z1 = ref.box_muller(np.array([0xffffffff, 0], dtype=np.uint64), np.array([0, 0], dtype=np.uint64))
    assert z0[0] == 0 and z1[0] == 0 and abs(z0[1] - (48 * np.log(2)) ** 0.5) < 1e-12


def test_line_endpoints_and_rounding_of_alpha():
    x = torch.randn(2, 3, 2, 4, 4)
    x0 = torch.randn(2, 3, 2, 4, 4)
    out = ref.line(x, x0, [0.0, 1 / 3, 1.0])
    assert torch.equal(out[:, 0], x0.double()) and torch.equal(out[:, 2], x.double())
    a, b = ref.f32_pair([1 / 3])
    assert float(a) == float(np.float32(1 / 3)) and float(b) == float(np.float32(1 - 1 / 3))
    assert torch.equal(ref.line(x, torch.tensor([1.0, 2.0, 3.0]), [0.0])[:, 0, 1], torch.full((2, 2, 4, 4), 2.0, dtype=torch.float64))
    assert not ref.line(x, None, [0.0]).any()


@pytest.mark.parametrize("rule,steps", [("trapezoid", 2), ("trapezoid", 8), ("trapezoid", 64), ("gausslegendre", 1),
                                        ("gausslegendre", 5), ("gausslegendre", 62)])
def test_rule_weights_sum_to_one(rule, steps):
    from gava_clip_amd import hip
    alpha, w = hip.path_rule(rule, steps)
    m = steps if rule == "trapezoid" else steps + 2
    assert len(alpha) == len(w) == m <= hip.PATH_MAX_STEPS
    assert abs(sum(w) - 1.0) <= 1e-14 and alpha[0] == 0.0 and alpha[-1] == 1.0
    assert all(0.0 <= a <= 1.0 for a in alpha) and all(b > a for a, b in zip(alpha, alpha[1:]))
    want = ref.trapezoid(steps) if rule == "trapezoid" else ref.gauss_legendre(steps)
    assert (alpha, w) == want
    if rule == "trapezoid":
        assert w[0] == w[-1] == 0.5 / (m - 1) and all(v == 1.0 / (m - 1) for v in w[1:-1])
        assert abs(sum(wk * a for wk, a in zip(w, alpha)) - 0.5) <= 1e-14                     # exact for a line
    else:
        assert w[0] == w[-1] == 0.0 and all(v > 0 for v in w[1:-1])
        for deg in range(min(2 * steps, 12)):                                                # exact up to degree 2 steps - 1
            assert abs(sum(wk * a ** deg for wk, a in zip(w, alpha)) - 1.0 / (deg + 1)) <= 1e-13, deg


def test_rule_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    for rule, steps in (("simpson", 8), ("trapezoid", 1), ("trapezoid", 65), ("gausslegendre", 0), ("gausslegendre", 63),
                        ("trapezoid", 8.0), ("trapezoid", True), ("trapezoid", None)):
        with pytest.raises(E, match="path_rule"):
            hip.path_rule(rule, steps)


@pytest.mark.parametrize("B,T,size,P,baseline", [(2, 3, 64, 16, "tensor"), (1, 2, 28, 14, "channel"), (2, 2, 21, 7, None)])
def test_restated_fold_is_the_path_integral_of_the_conv_gradient(B, T, size, P, baseline):
    """f(x) = sum(v * tanh(conv(x))): the restated fold of the m interpolants' patch gradients, weighted, is sum_k w_k grad f(x_k)
    as fp64 autograd gives it, and (x - x0) times it sums to f(x) - f(x0) (completeness, to the quadrature's error)."""
    D, n = 12, (size // P) ** 2
    gen = torch.Generator().manual_seed(size + P)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    conv = torch.nn.Conv2d(3, D, P, stride=P).double()
    with torch.no_grad():
        conv.weight.copy_(rnd(*conv.weight.shape) / (3 * P * P) ** 0.5)
    x, v = rnd(B, 3, T, size, size), rnd(B * T, n, D)
    base = rnd(B, 3, T, size, size) if baseline == "tensor" else rnd(3) if baseline == "channel" else None
    x0 = ref.baseline_like(x, base)

    def f(xx, vw):                                           # -> per-clip value, embedding output [clips*T, n, D]
        E = conv(xx.permute(0, 2, 1, 3, 4).reshape(-1, 3, size, size)).flatten(2).transpose(1, 2)
        return (vw * torch.tanh(E)).sum((1, 2)).view(-1, T).sum(1), E

    alpha, w = ref.gauss_legendre(30)
    m = len(alpha)
    w32 = [float(np.float32(k)) for k in w]                  # the kernel's weights are fp32
    a64 = torch.tensor(alpha, dtype=torch.float64).view(1, m, 1, 1, 1, 1)
    pts = (x0.unsqueeze(1) + a64 * (x - x0).unsqueeze(1)).reshape(B * m, 3, T, size, size).requires_grad_()       # clip b's copy k: b*m + k
    vv = v.view(B, 1, T, n, D).expand(B, m, T, n, D).reshape(B * m * T, n, D)           # every copy of a clip shares its clip's v
    vals, E = f(pts, vv)
    (grads,) = torch.autograd.grad(vals.sum(), [pts])
    want = (torch.tensor(w32, dtype=torch.float64).view(1, m, 1, 1, 1, 1) * grads.view(B, m, 3, T, size, size)).sum(1)
    # d E of every copy by hand, then the patch dgrad: what the backward hands the fold (here with a CLS row and padding columns)
    dE = vv * (1 - torch.tanh(E.detach()) ** 2)
    dpatch = torch.full((B * m * T, n + 1, 3 * P * P + 5), float("nan"), dtype=torch.float64)
    dpatch[:, 1:, :3 * P * P] = dE @ conv.weight.detach().view(D, -1)
    geo = (B, m, T, size, P, n + 1, 1, w32)
    got, s_abs = ref.fold_path(dpatch, *geo, ref.GRAD)
    assert got.shape == x.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((s_abs >= got.abs() * (1 - 1e-12)).all())
    attr, _ = ref.fold_path(dpatch, *geo, ref.ATTR, x=x, baseline=base)
    assert float((attr - (x - x0) * want).abs().max()) <= 1e-12 * float(attr.abs().max())
    signed, _ = ref.fold_path(dpatch, *geo, ref.ATTR_SUM, x=x, baseline=base)
    assert float((signed - attr.sum(1)).abs().max()) <= 1e-12 * float(attr.abs().max())
    mag, _ = ref.fold_path(dpatch, *geo, ref.ATTR_ABS, x=x, baseline=base)
    assert float((mag - attr.abs().sum(1)).abs().max()) <= 1e-12 * float(attr.abs().max())
    amax, _ = ref.fold_path(dpatch, *geo, ref.ABSMAX)
    l2, _ = ref.fold_path(dpatch, *geo, ref.L2)
    assert torch.equal(amax, got.abs().amax(1)) and float((l2 - got.pow(2).sum(1).sqrt()).abs().max()) <= 1e-12 * float(l2.max())
    # completeness: the endpoints are copies 0 and m - 1
    fx = vals.detach().view(B, m)
    total = signed.reshape(B, -1).sum(1)
    resid = float(((total - (fx[:, -1] - fx[:, 0])).abs() / signed.reshape(B, -1).abs().sum(1)).max())
    print(f"\n[path-grad] completeness residual {resid:.3e} of sum |a|")
    assert resid <= 1e-6                                     # the weights are rounded to fp32: 6e-8, and the quadrature's own error
    # the delta's restatement on the same numbers: one "class", rows b*m + k
    s, fd, sa = ref.delta(signed, fx.reshape(B * m, 1), torch.zeros(B, dtype=torch.int64), m, 0, m - 1)
    assert torch.allclose(s, total) and torch.allclose(fd, fx[:, -1] - fx[:, 0]) and bool((sa >= s.abs()).all())
    s, fd, _ = ref.delta(signed, fx.reshape(B * m, 1), torch.tensor([1] + [0] * (B - 1)), m, 0, m - 1)
    assert bool(torch.isnan(s[0])) and bool(torch.isnan(fd[0])) and not bool(torch.isnan(s[1:]).any())


# ---- the ABI's surface ---------------------------------------------------------------------------------------------------------

def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    from gava_clip_amd.build import SOURCES
    assert "path_grad.hip" in SOURCES
    for name, value in (("MAX_STEPS", 64), ("LINE", 0), ("NOISE", 1), ("GRAD", 0), ("ABSMAX", 1), ("L2", 2), ("ATTR", 3), ("ATTR_SUM", 4),
                        ("ATTR_ABS", 5)):
        assert re.search(rf"#define GAVA_PATH_{name} {value}\b", header) and getattr(hip, "PATH_" + name) == value == getattr(ref, name), name
    assert re.search(rf"#define GAVA_CLIP_RANGE_PARTS {hip.CLIP_RANGE_PARTS}\b", header)
    assert (hip.PATH_GRAD, hip.PATH_ABSMAX, hip.PATH_L2) == (hip.UNPATCH_GRAD, hip.UNPATCH_ABSMAX, hip.UNPATCH_L2)


def test_structs_match_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirrors == what the library reports (gava_path_grad_struct_sizes)."""
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){printf("' + " ".join(["%zu"] * len(STRUCTS)) + '\\n", ' + \
          ", ".join(f"sizeof({s})" for s in STRUCTS) + ");return 0;}"
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    lib = hip.load()
    got = (ctypes.c_size_t * 4)()
    assert lib.gava_path_grad_struct_sizes(got, 4) == 4
    mirrors = (hip.PathClipsArgs, hip.ClipRangeArgs, hip.UnpatchifyPathArgs, hip.PathDeltaArgs)
    assert [ctypes.sizeof(c) for c in mirrors] == sizes == list(got)
    assert lib.gava_path_grad_struct_sizes(None, 0) == 4              # a zero capacity writes nothing


ONE = 64      # a non-null, 16-byte aligned stand-in for a device pointer: every call below returns before it is used


def _refused(fn, make, bad):
    """Every change of `bad` to the valid arguments make() is refused with GAVA_EINVAL before any launch."""
    for kw in bad:
        a = make()
        for k, v in kw.items():
            if isinstance(v, tuple):                                   # (index, value) of an array field
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        assert fn(ctypes.byref(a), None) == -1, kw
    assert fn(None, None) == -1


def test_path_clips_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip
    lib = hip.load()

    def line():
        a = hip.PathClipsArgs()
        a.x, a.out, a.baseline = ONE, ONE, ONE
        a.nb, a.T, a.size, a.patch, a.mode, a.baseline_kind, a.m = 2, 3, 28, 14, hip.PATH_LINE, hip.BASELINE_TENSOR, 3
        for k, v in enumerate((0.0, 0.5, 1.0)):
            a.alpha[k], a.beta[k] = v, 1.0 - v
        return a

    def noise():
        a = hip.PathClipsArgs()
        a.x, a.out, a.sigma = ONE, ONE, ONE
        a.nb, a.T, a.size, a.patch, a.mode, a.baseline_kind, a.m, a.clip0, a.seed = 2, 3, 28, 14, hip.PATH_NOISE, hip.BASELINE_ZERO, 4, 5, 2 ** 63
        return a

    common = [dict(x=None), dict(out=None), dict(x=ONE + 4), dict(out=ONE + 8), dict(size=30), dict(m=0), dict(m=65), dict(mode=2), dict(mode=-1)] + \
             [{f: v} for f in ("nb", "T", "size", "patch") for v in (0, -1)]
    _refused(lib.gava_path_clips, line, common + [
        dict(baseline=None), dict(baseline=ONE + 4), dict(baseline_kind=hip.BASELINE_ZERO), dict(baseline_kind=3), dict(baseline_kind=-1),
        dict(baseline_kind=hip.BASELINE_CHANNEL, baseline=ONE + 2), dict(sigma=ONE),
        dict(alpha=(1, -0.25)), dict(alpha=(1, 1.5)), dict(alpha=(2, float("nan"))), dict(alpha=(0, float("inf"))), dict(beta=(1, float("nan")))])
    _refused(lib.gava_path_clips, noise, common + [
        dict(sigma=None), dict(sigma=ONE + 2), dict(baseline=ONE), dict(baseline_kind=hip.BASELINE_CHANNEL), dict(size=21, patch=7),
        dict(clip0=-1), dict(clip0=2 ** 31 - 2)])


def test_clip_range_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip

    def make():
        a = hip.ClipRangeArgs()
        a.x, a.min, a.max, a.sigma, a.workspace = ONE, ONE, ONE, ONE, ONE
        a.nb, a.T, a.size, a.rel = 2, 3, 21, 0.15
        return a

    _refused(hip.load().gava_clip_range, make, [{f: None} for f in ("x", "min", "max", "sigma", "workspace")] +
             [{f: ONE + 2} for f in ("x", "min", "max", "sigma", "workspace")] +
             [{f: v} for f in ("nb", "T", "size") for v in (0, -1)] + [dict(nb=65536)])


def test_unpatchify_path_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip

    def make(mode=hip.PATH_ABSMAX):
        def f():
            a = hip.UnpatchifyPathArgs()
            a.dpatch, a.ld, a.out = ONE, 640, ONE
            a.B, a.T, a.size, a.patch, a.mode, a.frame_rows, a.row_offset, a.m = 2, 3, 28, 14, mode, 5, 1, 3
            a.w[0], a.w[1], a.w[2] = 0.25, 0.0, -0.75
            if mode >= hip.PATH_ATTR:
                a.x = ONE
            return a
        return f

    fn = hip.load().gava_unpatchify_path
    geometry = [dict(dpatch=None), dict(out=None), dict(dpatch=ONE + 4), dict(out=ONE + 8), dict(size=30), dict(ld=587), dict(frame_rows=4),
                dict(row_offset=2), dict(row_offset=-1), dict(mode=6), dict(mode=-1), dict(m=0), dict(m=65), dict(B=65536, T=32768, m=1),
                dict(B=32768, T=32768, m=2), dict(w=(1, float("nan"))), dict(w=(2, float("inf"))), dict(baseline_kind=3)] + \
               [{f: v} for f in ("B", "T", "size", "patch") for v in (0, -1)]
    for mode in (hip.PATH_GRAD, hip.PATH_ABSMAX, hip.PATH_L2):
        _refused(fn, make(mode), geometry + [dict(x=ONE), dict(baseline=ONE), dict(baseline_kind=hip.BASELINE_CHANNEL),
                                             dict(baseline=ONE, baseline_kind=hip.BASELINE_TENSOR)])
    for mode in (hip.PATH_ATTR, hip.PATH_ATTR_SUM, hip.PATH_ATTR_ABS):
        _refused(fn, make(mode), geometry + [dict(x=None), dict(x=ONE + 4), dict(baseline=ONE), dict(baseline_kind=hip.BASELINE_TENSOR),
                                             dict(baseline=ONE + 4, baseline_kind=hip.BASELINE_TENSOR),
                                             dict(baseline=ONE + 2, baseline_kind=hip.BASELINE_CHANNEL)])


def test_path_delta_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip

    def make():
        a = hip.PathDeltaArgs()
        a.map, a.logits, a.ld, a.target, a.sum_attr, a.f_diff, a.delta = ONE, ONE, 3, ONE, ONE, ONE, ONE
        a.B, a.T, a.size, a.m, a.C, a.k_lo, a.k_hi = 2, 3, 28, 8, 3, 0, 7
        return a

    ptrs = ("map", "logits", "target", "sum_attr", "f_diff", "delta")
    _refused(hip.load().gava_path_delta, make, [{f: None} for f in ptrs] + [{f: ONE + 2} for f in ptrs] + [dict(target=ONE + 4)] +
             [{f: v} for f in ("B", "T", "size", "C") for v in (0, -1)] +
             [dict(ld=2), dict(m=0), dict(m=65), dict(k_lo=-1), dict(k_lo=8), dict(k_hi=-1), dict(k_hi=8)])


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------

def f(*s, dtype=torch.float32):
    return torch.zeros(*s, dtype=dtype)


def test_path_clips_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    x, sg = f(2, 3, 3, 28, 28), f(2)
    ok = dict(patch=14, alpha=[0.0, 0.5, 1.0])
    with pytest.raises(E, match="HIP device"):
        hip.path_clips(x, **ok)                                                        # CPU tensors: everything else about them is right
    with pytest.raises(E, match="HIP device"):
        hip.path_clips(x, patch=14, sigma=sg, samples=4)
    with pytest.raises(E, match="not both and not neither"):
        hip.path_clips(x, patch=14)
    with pytest.raises(E, match="not both and not neither"):
        hip.path_clips(x, sigma=sg, samples=2, **ok)
    for bad in (x.double(), x[..., ::2], f(2, 3, 3, 28, 14), f(2, 4, 3, 28, 28), f(0, 3, 3, 28, 28), "x"):
        with pytest.raises(E, match="contiguous fp32"):
            hip.path_clips(bad, **ok)
    for patch in (13, 0, 14.0):
        with pytest.raises(E, match="whole patches"):
            hip.path_clips(x, patch=patch, alpha=[0.5])
    for alpha in ([], [0.5] * 65):
        with pytest.raises(E, match="between 1 and 64"):
            hip.path_clips(x, patch=14, alpha=alpha)
    for alpha in ([0.5, -0.1], [1.5]):
        with pytest.raises(E, match=r"\[0, 1\]"):
            hip.path_clips(x, patch=14, alpha=alpha)
    with pytest.raises(E, match="finite"):
        hip.path_clips(x, patch=14, alpha=[float("nan")])
    with pytest.raises(E, match="list of numbers"):
        hip.path_clips(x, patch=14, alpha=["a"])
    with pytest.raises(E, match="samples goes with sigma"):
        hip.path_clips(x, samples=3, **ok)
    for base in (f(4), f(2, 3, 3, 28, 14), f(3).double(), "zero"):
        with pytest.raises(E, match="baseline must be"):
            hip.path_clips(x, baseline=base, **ok)
    with pytest.raises(E, match="out must be"):
        hip.path_clips(x, out=f(2, 2, 3, 3, 28, 28), **ok)
    with pytest.raises(E, match="baseline goes with alpha"):
        hip.path_clips(x, patch=14, sigma=sg, samples=2, baseline=f(3))
    for samples in (0, 65, None, 2.0, True):
        with pytest.raises(E, match="samples must be"):
            hip.path_clips(x, patch=14, sigma=sg, samples=samples)
    for sigma in (f(3), f(2).double(), f(2, 1), 0.1):
        with pytest.raises(E, match="sigma must be"):
            hip.path_clips(x, patch=14, sigma=sigma, samples=2)
    with pytest.raises(E, match="odd size"):
        hip.path_clips(f(2, 3, 3, 21, 21), patch=7, sigma=sg, samples=2)
    for seed in (-1, 2 ** 64, 1.0):
        with pytest.raises(E, match="seed must be"):
            hip.path_clips(x, patch=14, sigma=sg, samples=2, seed=seed)
    for clip0 in (-1, 2 ** 31 - 2, 1.0):
        with pytest.raises(E, match="clip0"):
            hip.path_clips(x, patch=14, sigma=sg, samples=2, clip0=clip0)


def test_clip_range_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    with pytest.raises(E, match="HIP device"):
        hip.clip_range(f(2, 3, 3, 28, 28), 0.15)
    for bad in (f(2, 3, 3, 28, 28).half(), f(2, 3, 28, 28), f(2, 3, 3, 28, 14), f(0, 3, 3, 28, 28)):
        with pytest.raises(E, match="contiguous fp32"):
            hip.clip_range(bad)
    for rel in (float("nan"), float("inf"), None, "a", True):
        with pytest.raises(E, match="rel must be"):
            hip.clip_range(f(1, 3, 1, 4, 4), rel)
    with pytest.raises(E, match="at most 65535"):
        hip.clip_range(f(65536, 3, 1, 2, 2))


def test_unpatchify_path_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    kw = dict(B=2, T=3, size=28, patch=14, mode=hip.PATH_ABSMAX, frame_rows=5, row_offset=1, w=[0.5, 0.0, -0.5])
    dp, out, clip = f(90, 640), f(2, 3, 28, 28), f(2, 3, 3, 28, 28)
    attr = {**kw, "mode": hip.PATH_ATTR_SUM}
    with pytest.raises(E, match="HIP device"):
        hip.unpatchify_path(dp, out, **kw)
    with pytest.raises(E, match="HIP device"):
        hip.unpatchify_path(dp, clip, x=clip, baseline=f(3), **{**kw, "mode": hip.PATH_ATTR})
    with pytest.raises(E, match="unknown mode"):
        hip.unpatchify_path(dp, out, **{**kw, "mode": 6})
    with pytest.raises(E, match="x goes with"):
        hip.unpatchify_path(dp, out, x=clip, **kw)
    with pytest.raises(E, match="x goes with"):
        hip.unpatchify_path(dp, out, **attr)
    with pytest.raises(E, match="baseline goes with"):
        hip.unpatchify_path(dp, out, baseline=f(3), **kw)
    with pytest.raises(E, match="fp32"):
        hip.unpatchify_path(dp.double(), out, **kw)
    with pytest.raises(E, match="contiguous"):
        hip.unpatchify_path(dp, f(2, 3, 28, 56)[..., ::2], **kw)
    for w in ([], [1.0] * 65):
        with pytest.raises(E, match="between 1 and 64"):
            hip.unpatchify_path(dp, out, **{**kw, "w": w})
    with pytest.raises(E, match="finite"):
        hip.unpatchify_path(dp, out, **{**kw, "w": [1.0, float("inf"), 0.0]})
    with pytest.raises(E, match="frames of"):
        hip.unpatchify_path(dp, out, **{**kw, "w": [1.0, 1.0]})                    # 90 rows are 2 x 3 x 3 frames, not 2 x 2 x 3
    with pytest.raises(E, match="frames of"):
        hip.unpatchify_path(f(15, 6, 640), out, **kw)
    with pytest.raises(E, match="patch columns"):
        hip.unpatchify_path(f(90, 584), out, **kw)
    with pytest.raises(E, match="of a frame of"):
        hip.unpatchify_path(f(72, 640), out, **{**kw, "frame_rows": 4})
    with pytest.raises(E, match="this mode writes"):
        hip.unpatchify_path(dp, clip, **kw)
    with pytest.raises(E, match="this mode writes"):
        hip.unpatchify_path(dp, out, **{**kw, "mode": hip.PATH_GRAD})
    with pytest.raises(E, match="this mode writes"):
        hip.unpatchify_path(dp, out, x=clip, **{**kw, "mode": hip.PATH_ATTR})
    with pytest.raises(E, match="x is"):
        hip.unpatchify_path(dp, out, x=f(2, 3, 3, 28, 14), **attr)
    with pytest.raises(E, match="baseline must be"):
        hip.unpatchify_path(dp, out, x=clip, baseline=f(4), **attr)
    with pytest.raises(E, match="size=30"):
        hip.unpatchify_path(dp, out, **{**kw, "size": 30})


def test_path_delta_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    a, lg, tg = f(2, 3, 28, 28), f(16, 3), f(2, dtype=torch.int64)
    kw = dict(m=8, k_lo=0, k_hi=7)
    with pytest.raises(E, match="HIP device"):
        hip.path_delta(a, lg, tg, **kw)
    for bad in (a.double(), f(2, 3, 3, 28, 28), f(2, 3, 28, 14), f(0, 3, 28, 28)):
        with pytest.raises(E, match="attr must be"):
            hip.path_delta(bad, lg, tg, **kw)
    for m in (0, 65, 8.0, True):
        with pytest.raises(E, match="m must be"):
            hip.path_delta(a, lg, tg, **{**kw, "m": m})
    for bad in (lg.double(), f(16), f(3, 16).t()):
        with pytest.raises(E, match="logits must be"):
            hip.path_delta(a, bad, tg, **kw)
    with pytest.raises(E, match="clips of 8 steps"):
        hip.path_delta(a, f(15, 3), tg, **kw)
    for name in ("k_lo", "k_hi"):
        for k in (-1, 8, 1.0):
            with pytest.raises(E, match=name):
                hip.path_delta(a, lg, tg, **{**kw, name: k})
    for bad in (tg.int(), f(3, dtype=torch.int64), f(4, dtype=torch.int64)[::2], None):
        with pytest.raises(E, match="target must be"):
            hip.path_delta(a, lg, bad, **kw)


# ---- the model methods -----------------------------------------------------------------------------------------------------------

def test_model_method_refusals_without_a_device():
    from gava_clip_amd import VitaCLIP, hip
    from helpers import CLASSES_3, model_kwargs
    E = hip.GavaError
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3)).eval()
    S, T = TINY.input_size, TINY.num_frames
    x = torch.zeros(1, 3, T, S, S)
    for call in (m.integrated_gradients, m.smooth_grad):
        with pytest.raises(E, match="HIP device"):
            call(x)                                                                    # everything else about the call is right
        with pytest.raises(E, match="HIP device"):
            call(x, target=torch.zeros(1, dtype=torch.int64))
        for bad in (x[0], x.long(), torch.zeros(1, 3, T, S, S // 2), torch.zeros(1, 3, T, S // 2, S // 2), torch.zeros(0, 3, T, S, S), None):
            with pytest.raises(E, match="floating-point clip batch"):
                call(bad)
        for target in (3, -1):
            with pytest.raises(E, match="outside the 3 classes"):
                call(x, target=target)
        for target in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
            with pytest.raises(E, match="int64"):
                call(x, target=target)
        for max_clips in (0, -1, 2.0, None, True):
            with pytest.raises(E, match="max_clips"):
                call(x, max_clips=max_clips)
        with pytest.raises(E, match="reduce"):
            call(x, reduce="max")
    # integrated_gradients' own
    for kw in (dict(reduce="absmax"), dict(reduce="l2"), dict(reduce="sum", multiply=False), dict(reduce="abs", multiply=False)):
        with pytest.raises(E, match="reduce"):
            m.integrated_gradients(x, **kw)
    for kw in (dict(rule="simpson"), dict(steps=1), dict(steps=65), dict(steps=63, rule="gausslegendre"), dict(steps=0, rule="gausslegendre"),
               dict(steps=8.0)):
        with pytest.raises(E, match="path_rule"):
            m.integrated_gradients(x, **kw)
    for baseline in ("mean", torch.zeros(4), torch.zeros(1, 3, T, S, S // 2), torch.zeros(3, dtype=torch.int64), None):
        with pytest.raises(E, match="baseline must be"):
            m.integrated_gradients(x, baseline=baseline)
    with pytest.raises(E, match="gaussian_taps"):
        m.integrated_gradients(x, baseline="blur", blur_sigma=0.0)
    with pytest.raises(E, match="frames one launch covers"):
        m.integrated_gradients(_long_clip(S, 1100), steps=64)
    # smooth_grad's own
    for samples in (0, 65, 4.0, None, True):
        with pytest.raises(E, match="samples must be"):
            m.smooth_grad(x, samples=samples)
    for sigma in (-0.1, float("nan"), float("inf"), "a", None):
        with pytest.raises(E, match="sigma must be"):
            m.smooth_grad(x, sigma=sigma)
    for seed in (-1, 2 ** 64, 0.5):
        with pytest.raises(E, match="seed must be"):
            m.smooth_grad(x, seed=seed)
    with pytest.raises(E, match="frames one launch covers"):
        m.smooth_grad(_long_clip(S, 1100), samples=64)
    # faithfulness knows the two new names and still refuses the unknown ones; its default is what it was
    assert m._FAITHFULNESS_METHODS == ("rollout", "relevance", "saliency", "integrated", "smoothgrad")
    import inspect
    assert inspect.signature(m.faithfulness).parameters["methods"].default == ("rollout", "relevance", "saliency")
    with torch.no_grad():
        with pytest.raises(E, match="distinct names"):
            m.faithfulness(x, methods=("integrated", "lime"))
        with pytest.raises(E, match="distinct names"):
            m.faithfulness(x, methods=("smoothgrad", "smoothgrad"))
        with pytest.raises(E, match="no CPU fallback"):
            m.faithfulness(x, methods=("integrated", "smoothgrad"))


def _long_clip(S, T):
    """A [1, 3, T, S, S] clip that takes no memory: every refusal returns before it is read."""
    return torch.zeros(1, 1, 1, 1, 1).expand(1, 3, T, S, S)
