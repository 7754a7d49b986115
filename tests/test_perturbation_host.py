"""CPU: the reference of the faithfulness curves (perturbation_ref.py) against the definitions, the host arithmetic of the
wrappers (thresholds, taps), their argument checks - every one refused with GavaError before a device is touched - and the ABI
of the four new calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import perturbation_ref as pr
from helpers import REPO

NAN, INF = float("nan"), float("inf")


# ---- the reference ranking ----------------------------------------------------------------------------------------------
def test_stable_sort_ranks_agree_with_the_counting_definition():
    s = [1.5, 0.0, -0.0, NAN, 1.5, INF, -INF, -2.0, NAN, 0.0, 1.5, -INF]
    want = pr.ranks_by_counting(s)
    got = pr.ranks_1d(np.array(s, dtype=np.float32))
    assert np.array_equal(got, want)
    # spelled out: +inf, the three 1.5 by index, the three zeros (either sign) by index, -2, the two -inf, the two NaNs
    assert got.tolist() == [1, 4, 5, 10, 2, 0, 8, 7, 11, 6, 3, 9]
    assert sorted(got.tolist()) == list(range(len(s)))


@pytest.mark.parametrize("regime", pr.REGIMES)
def test_reference_ranks_are_a_permutation_per_ranking(regime):
    s = pr.regime_scores((2, 3, 4, 4), regime, 7)
    for scope, n in (("clip", 48), ("frame", 16)):
        r = pr.ranks(s, scope).view(-1, n)
        assert r.dtype == torch.int32 and torch.equal(r.sort(1).values, torch.arange(n, dtype=torch.int32).expand_as(r))
    flat = s.view(2, -1)
    assert np.array_equal(pr.ranks(s, "clip")[1].numpy(), pr.ranks_by_counting(flat[1].tolist()))
    if regime == "equal":
        assert torch.equal(pr.ranks(s, "clip")[0], torch.arange(48, dtype=torch.int32))
    if regime == "descending":
        assert torch.equal(pr.ranks(s, "clip")[0], torch.arange(48, dtype=torch.int32))
    if regime == "ascending":
        assert torch.equal(pr.ranks(s, "clip")[0], torch.arange(47, -1, -1, dtype=torch.int32))


def test_pixel_scores_pool_to_patches():
    s = pr.integer_pixels(1, 2, 28, 3)
    pooled = pr.pool_pixels(s, 14)
    assert pooled.shape == (1, 2, 2, 2) and float(pooled[0, 1, 1, 0]) == float(s[0, 1, 14:, :14].double().sum())
    assert torch.equal(pooled.float().double(), pooled)                    # exact in fp32
    assert torch.equal(pr.ranks(s, "clip", patch=14), pr.ranks(pooled.float(), "clip"))


# ---- thresholds ---------------------------------------------------------------------------------------------------------
def test_thresholds_and_nested_masks():
    from gava_clip_amd import hip
    f, k = hip.perturb_thresholds(64, steps=10)
    assert k == [0, 6, 13, 19, 26, 32, 38, 45, 51, 58, 64] == pr.thresholds(64, pr.linspace_fractions(10))
    assert f == pr.linspace_fractions(10) and f[0] == 0.0 and f[-1] == 1.0
    f, k = hip.perturb_thresholds(1568, fractions=[0, 0.05, 0.5, 1])
    assert k == [0, 78, 784, 1568] and f == [0.0, 0.05, 0.5, 1.0]
    assert hip.perturb_thresholds(3, fractions=torch.tensor([0.0, 0.5, 1.0]))[1] == [0, 2, 3]           # 1.5 rounds up
    # masked sets are nested from step to step, and the clips follow: deletion only ever loses pixels of x, insertion only gains
    x = torch.randn(1, 3, 4, 16, 16) + 3.0
    rk = pr.ranks(pr.regime_scores((1, 4, 4, 4), "randn", 1), "clip")
    ks = hip.perturb_thresholds(64, steps=10)[1]
    d = pr.perturb(x, rk, ks, 4, "deletion")
    i = pr.perturb(x, rk, ks, 4, "insertion")
    kept_d, kept_i = d == x.unsqueeze(1), i == x.unsqueeze(1)
    for s in range(1, len(ks)):
        assert bool((kept_d[:, s] <= kept_d[:, s - 1]).all()) and bool((kept_i[:, s] >= kept_i[:, s - 1]).all())
        assert int((~kept_d[0, s, 0]).sum()) == ks[s] * 16 == int(kept_i[0, s, 0].sum())
    assert torch.equal(d[:, 0], x) and float(d[:, -1].abs().max()) == 0.0
    assert torch.equal(i[:, -1], x) and float(i[:, 0].abs().max()) == 0.0


def test_gaussian_taps():
    from gava_clip_amd import hip
    for sigma, r in ((0.5, 2), (1.0, 3), (5.0, 15)):
        w = hip.gaussian_taps(sigma)
        assert w.dtype == torch.float32 and w.numel() == 2 * r + 1 and torch.equal(w, pr.gaussian_taps(sigma))
        assert abs(float(w.double().sum()) - 1) <= (2 * r + 1) * pr.U and torch.equal(w, w.flip(0))
    with pytest.raises(hip.GavaError, match="radius"):
        hip.gaussian_taps(30.0)
    with pytest.raises(hip.GavaError, match="positive"):
        hip.gaussian_taps(0.0)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 5.0])
def test_fp32_blur_stays_a_factor_of_eight_inside_the_bound(sigma):
    """The bound the kernel is held to, |d| <= 2 (2r + 2) 2^-24 max|x|, against a CPU fp32 convolution in tap order."""
    x = torch.randn(1, 3, 2, 28, 28, generator=torch.Generator().manual_seed(int(sigma * 10)))
    taps = pr.gaussian_taps(sigma)
    ref = pr.blur(x, taps)
    err = float((pr.blur(x, taps, torch.float32).double() - ref).abs().max())
    assert err * 8 <= pr.blur_bound(taps, x), (err, pr.blur_bound(taps, x))
    const = torch.full((1, 3, 1, 28, 28), 2.75)
    assert float((pr.blur(const, taps) - 2.75).abs().max()) <= pr.blur_bound(taps, const)


def test_reference_scores():
    lg = torch.tensor([[1.0, 3.0, 3.0], [0.0, -1.0, 5.0], [2.0, 2.0, 2.0], [4.0, 0.0, 0.0]])
    r = pr.scores_ref(lg, 2, [0.0, 1.0], None, 0)
    assert r["top1"].tolist() == [[1, 2], [0, 0]] and r["target"].tolist() == [1, 0]
    assert r["logit"].tolist() == [[3.0, -1.0], [2.0, 4.0]] and r["auc_logit"].tolist() == [1.0, 3.0]
    r = pr.scores_ref(lg, 2, [0.0, 1.0], torch.tensor([3, 2]), 0)
    assert torch.isnan(r["logit"][0]).all() and torch.isnan(r["auc_prob"][0]) and r["logit"][1].tolist() == [2.0, 0.0]


# ---- argument checks: GavaError, no device ------------------------------------------------------------------------------
def test_bad_fractions_are_refused():
    from gava_clip_amd import hip
    for bad in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.5, 0.5, 1.0], [0.0, 0.7, 0.3, 1.0], [0.0], [0.0, NAN, 1.0], "abc"):
        with pytest.raises(hip.GavaError, match="fractions"):
            hip.perturb_thresholds(64, fractions=bad)
    with pytest.raises(hip.GavaError, match="steps"):
        hip.perturb_thresholds(64, steps=0)
    with pytest.raises(hip.GavaError, match="at most 128"):
        hip.perturb_thresholds(64, steps=128)


def test_wrappers_refuse_wrong_arguments_without_a_device():
    from gava_clip_amd import hip
    f32 = torch.zeros
    with pytest.raises(hip.GavaError, match="scope='frame'"):
        hip.patch_ranks(f32(2, 4), scope="frame")
    with pytest.raises(hip.GavaError, match="scope must be"):
        hip.patch_ranks(f32(2, 4), scope="video")
    with pytest.raises(hip.GavaError, match="contiguous fp32"):
        hip.patch_ranks(f32(2, 4, 4, 4, dtype=torch.float16))
    with pytest.raises(hip.GavaError, match="contiguous fp32"):
        hip.patch_ranks(f32(2, 4, 4))
    with pytest.raises(hip.GavaError, match="square"):
        hip.patch_ranks(f32(2, 4, 4, 6))
    with pytest.raises(hip.GavaError, match="whole patches"):
        hip.patch_ranks(f32(1, 2, 28, 28), patch=16)
    with pytest.raises(hip.GavaError, match="65537 units per ranking, at most 65536"):
        hip.patch_ranks(f32(1, 65537))
    with pytest.raises(hip.GavaError, match="at most 65536"):
        hip.patch_ranks(f32(1, 257, 16, 16))
    assert hip.PERTURB_MAX_UNITS == pr.MAX_UNITS == 65536
    with pytest.raises(hip.GavaError, match="no CPU fallback"):            # everything else in order: only the device is wrong
        hip.patch_ranks(f32(1, 4, 16, 16), scope="frame")

    x, rk = f32(2, 3, 4, 16, 16), torch.zeros(2, 64, dtype=torch.int32)
    with pytest.raises(hip.GavaError, match="mode must be"):
        hip.perturb_clips(x, rk, [0, 64], patch=4, mode="erase")
    with pytest.raises(hip.GavaError, match=r"fp32 \[nb, 3, T, S, S\]"):
        hip.perturb_clips(x.double(), rk, [0, 64], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match=r"fp32 \[nb, 3, T, S, S\]"):
        hip.perturb_clips(x[:, :2], rk, [0, 64], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match="whole patches"):
        hip.perturb_clips(x, rk, [0, 64], patch=5, mode="deletion")
    with pytest.raises(hip.GavaError, match="int32"):
        hip.perturb_clips(x, rk.long(), [0, 64], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match="int32"):
        hip.perturb_clips(x, rk[:, :63].contiguous(), [0, 64], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match="non-decreasing"):
        hip.perturb_clips(x, rk, [0, 9, 8], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match="thresholds, between 1 and 128"):
        hip.perturb_clips(x, rk, [], patch=4, mode="deletion")
    with pytest.raises(hip.GavaError, match="baseline must be"):
        hip.perturb_clips(x, rk, [0, 64], patch=4, mode="deletion", baseline=f32(4))
    with pytest.raises(hip.GavaError, match="no CPU fallback"):
        hip.perturb_clips(x, rk, [0, 64], patch=4, mode="deletion", baseline=f32(3))

    with pytest.raises(hip.GavaError, match=r"fp32 \[B, 3, T, S, S\]"):
        hip.blur_clips(f32(2, 3, 4, 16, 8), pr.gaussian_taps(1.0))
    with pytest.raises(hip.GavaError, match="taps"):
        hip.blur_clips(x, f32(4))
    with pytest.raises(hip.GavaError, match="taps"):
        hip.blur_clips(x, f32(131))
    with pytest.raises(hip.GavaError, match="no CPU fallback"):
        hip.blur_clips(x, pr.gaussian_taps(1.0))

    lg = f32(6, 3)
    with pytest.raises(hip.GavaError, match="whole clips"):
        hip.perturb_scores(lg, [0.0, 0.3, 0.6, 1.0], ref_step=0)
    with pytest.raises(hip.GavaError, match="ref_step"):
        hip.perturb_scores(lg, [0.0, 0.5, 1.0], ref_step=3)
    with pytest.raises(hip.GavaError, match="contiguous rows"):
        hip.perturb_scores(lg.double(), [0.0, 0.5, 1.0], ref_step=0)
    with pytest.raises(hip.GavaError, match="int64"):
        hip.perturb_scores(lg, [0.0, 0.5, 1.0], ref_step=0, target=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(hip.GavaError, match="int64"):
        hip.perturb_scores(lg, [0.0, 0.5, 1.0], ref_step=0, target=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(hip.GavaError, match="no CPU fallback"):
        hip.perturb_scores(lg, [0.0, 0.5, 1.0], ref_step=0, target=torch.zeros(2, dtype=torch.int64))


def test_model_refuses_wrong_arguments_without_a_device():
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.config import TINY
    from gava_clip_amd.hip import GavaError
    from helpers import model_kwargs
    m = VitaCLIP(**model_kwargs(TINY)).eval()
    S, T = TINY.input_size, TINY.num_frames
    g = S // TINY.patch_size
    x, s = torch.zeros(2, 3, T, S, S), torch.zeros(2, T, g, g)
    with pytest.raises(GavaError, match="no_grad"):
        m.perturbation_curves(x, s)
    with pytest.raises(GavaError, match="no_grad"):
        m.faithfulness(x)
    with torch.no_grad():
        with pytest.raises(GavaError, match="eval"):
            m.train().perturbation_curves(x, s)
        m.eval()
        with pytest.raises(GavaError, match="mode must be"):
            m.perturbation_curves(x, s, mode="erase")
        with pytest.raises(GavaError, match="scope='frame'"):
            m.perturbation_curves(x, torch.zeros(2, T), scope="frame")
        with pytest.raises(GavaError, match="scores must be"):
            m.perturbation_curves(x, torch.zeros(2, T, g + 1, g + 1))
        with pytest.raises(GavaError, match="scores must be"):
            m.perturbation_curves(x, s.long())
        with pytest.raises(GavaError, match="clip batch"):
            m.perturbation_curves(x[:, :, :, :-1], s)
        with pytest.raises(GavaError, match="fractions"):
            m.perturbation_curves(x, s, fractions=[0.0, 0.5])
        with pytest.raises(GavaError, match="target 3 is outside the 3 classes"):
            m.perturbation_curves(x, s, target=3)
        with pytest.raises(GavaError, match=r"int64 \[2\]"):
            m.perturbation_curves(x, s, target=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(GavaError, match="baseline must be"):
            m.perturbation_curves(x, s, baseline="mean")
        with pytest.raises(GavaError, match="baseline must be"):
            m.perturbation_curves(x, s, baseline=torch.zeros(4))
        with pytest.raises(GavaError, match="radius"):
            m.perturbation_curves(x, s, baseline="blur", blur_sigma=40.0)
        with pytest.raises(GavaError, match="no CPU fallback"):
            m.perturbation_curves(x, s)
        with pytest.raises(GavaError, match="methods"):
            m.faithfulness(x, methods=("rollout", "lime"))
        with pytest.raises(GavaError, match="mode is not an argument"):
            m.faithfulness(x, mode="deletion")
    assert m.cache_text_features in (True, False) and all(p.grad is None for p in m.parameters())


def test_result_types_are_exported_and_print():
    import gava_clip_amd
    from gava_clip_amd.model import Faithfulness, PerturbationCurves, VitaCLIP
    assert gava_clip_amd.PerturbationCurves is PerturbationCurves and gava_clip_amd.Faithfulness is Faithfulness
    assert callable(VitaCLIP.perturbation_curves) and callable(VitaCLIP.faithfulness)
    z = torch.zeros
    c = PerturbationCurves("deletion", z(3), z(2, 3), z(2, 3), z(2, 3, dtype=torch.int32), z(2), torch.ones(2), z(2, dtype=torch.int64),
                           z(2, 64, dtype=torch.int32))
    assert repr(c).startswith("PerturbationCurves(mode='deletion', fractions=(3,), logit=(2, 3)") and "ranks=(2, 64)" in repr(c)
    t = Faithfulness(relevance=dict(deletion=c, insertion=c), random=dict(deletion=c, insertion=c)).table().splitlines()
    assert len(t) == 3 and t[0].split()[0] == "method" and t[1].split() == ["relevance", "1.0000", "1.0000", "0.0000", "0.0000"]


# ---- ABI ------------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"gava_patch_ranks_args": "PatchRanksArgs", "gava_blur_clips_args": "BlurClipsArgs",
               "gava_perturb_clips_args": "PerturbClipsArgs", "gava_perturb_scores_args": "PerturbScoresArgs"}
NEW_SYMBOLS = ("gava_patch_ranks", "gava_blur_clips", "gava_perturb_clips", "gava_perturb_scores", "gava_perturbation_struct_sizes")


def test_perturbation_structs_match_the_header_and_the_library(tmp_path):
    """sizeof of the four structs as the C compiler sees the header == the ctypes mirrors == what the library reports; the
    constants of the header == the module's."""
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    consts = {"GAVA_PERTURB_MAX_UNITS": hip.PERTURB_MAX_UNITS, "GAVA_PERTURB_MAX_STEPS": hip.PERTURB_MAX_STEPS,
              "GAVA_BLUR_MAX_RADIUS": hip.BLUR_MAX_RADIUS, "GAVA_RANK_PIXEL": hip.RANK_PIXEL, "GAVA_RANK_FRAME": hip.RANK_FRAME,
              "GAVA_SCOPE_FRAME": hip.SCOPE_FRAME, "GAVA_UNITS_FRAME": hip.UNITS_FRAME, "GAVA_PERTURB_INSERTION": hip.PERTURB_INSERTION,
              "GAVA_BASELINE_CHANNEL": hip.BASELINE_CHANNEL, "GAVA_BASELINE_TENSOR": hip.BASELINE_TENSOR}
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in NEW_STRUCTS) + "".join(
        f'printf("{n} %d\\n", (int){n});' for n in consts) + "return 0;}"
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")]).decode().split()
    seen = dict(zip(out[::2], map(int, out[1::2])))
    for n, cls in NEW_STRUCTS.items():
        assert ctypes.sizeof(getattr(hip, cls)) == seen[n], n
    for n, v in consts.items():
        assert seen[n] == v, n
    lib = hip.load()
    sizes = (ctypes.c_size_t * 8)()
    assert lib.gava_perturbation_struct_sizes(sizes, 8) == 4
    assert list(sizes[:4]) == [seen[n] for n in NEW_STRUCTS] and list(sizes[4:]) == [0] * 4
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in hip.EXPORTS, name


def test_load_refuses_a_perturbation_mirror_that_is_out_of_step(monkeypatch):
    from gava_clip_amd import hip
    hip.load()

    class Short(ctypes.Structure):
        _fields_ = hip.PerturbClipsArgs._fields_[:-1]
    monkeypatch.setattr(hip, "PerturbClipsArgs", Short)
    monkeypatch.setattr(hip, "_lib", None)
    with pytest.raises(hip.GavaError, match="out of step"):
        hip.load()
    monkeypatch.undo()
    hip._lib = None
    hip.load()


def test_library_refuses_bad_shapes_before_any_launch():
    """GAVA_EINVAL (-1) from the raw calls, with null or host pointers that are never dereferenced: no device is needed."""
    from gava_clip_amd import hip
    lib = hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = hip.PatchRanksArgs()
    a.scores, a.ranks, a.B, a.T, a.g, a.layout, a.scope = p, p, 1, 65537, 1, hip.RANK_FRAME, hip.SCOPE_CLIP
    assert lib.gava_patch_ranks(ctypes.byref(a), None) == -1                 # one unit too many
    a.T, a.scope = 4, hip.SCOPE_FRAME
    assert lib.gava_patch_ranks(ctypes.byref(a), None) == -1                 # frame scope with frame scores
    a.layout, a.scope, a.T, a.g = hip.RANK_PATCH, hip.SCOPE_CLIP, 257, 16
    assert lib.gava_patch_ranks(ctypes.byref(a), None) == -1
    a.layout, a.T, a.g, a.patch = hip.RANK_PIXEL, 1, 2, 4
    assert lib.gava_patch_ranks(ctypes.byref(a), None) == -1                 # pixel scores without the workspace
    a.scores = None
    assert lib.gava_patch_ranks(ctypes.byref(a), None) == -1
    b = hip.BlurClipsArgs()
    b.x, b.taps, b.tmp, b.out, b.B, b.T, b.size, b.radius = p, p, p, p, 1, 1, 8, 1
    assert lib.gava_blur_clips(ctypes.byref(b), None) == -1                  # x, tmp and out must differ
    b.radius, b.tmp, b.out = 65, ctypes.c_void_p(p.value + 64), ctypes.c_void_p(p.value + 128)
    assert lib.gava_blur_clips(ctypes.byref(b), None) == -1
    c = hip.PerturbClipsArgs()
    c.x, c.ranks, c.out, c.nb, c.T, c.size, c.patch, c.n_steps = p, p, p, 1, 1, 8, 3, 1
    assert lib.gava_perturb_clips(ctypes.byref(c), None) == -1               # 8 pixels are no whole patches of 3
    c.patch, c.n_steps = 4, 129
    assert lib.gava_perturb_clips(ctypes.byref(c), None) == -1
    c.n_steps, c.k[0], c.k[1] = 2, 5, 4
    assert lib.gava_perturb_clips(ctypes.byref(c), None) == -1               # decreasing thresholds
    c.k[1], c.baseline_kind = 6, hip.BASELINE_CHANNEL
    assert lib.gava_perturb_clips(ctypes.byref(c), None) == -1               # a kind that needs a pointer, without one
    d = hip.PerturbScoresArgs()
    d.logits, d.ld, d.logit, d.prob, d.top1, d.auc_logit, d.auc_prob, d.target_out = p, 3, p, p, p, p, p, p
    d.nb, d.n_steps, d.C, d.ref_step = 1, 2, 3, 2
    assert lib.gava_perturb_scores(ctypes.byref(d), None) == -1              # ref_step outside the steps
    d.ref_step, d.ld = 0, 2
    assert lib.gava_perturb_scores(ctypes.byref(d), None) == -1              # rows shorter than the classes
