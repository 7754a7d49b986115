"""CPU: the fp64 restatement of the soft-target criterion (tests/mix_ref.py) reproduces the reference's own criterion under
autograd (tests/golden/soft_loss_ref.npz, written by tools/gen_golden_soft_loss.py from training/loss_utils.py and
CrossEntropyLoss with class probabilities in fp64): every array to 1e-12 relative, the bound tests/test_train_criterion_host.py
holds loss_ref to.  On one-hot targets it is loss_ref.criterion.  Plus ClipMixer's host plan, and the host side of the new C ABI:
names, struct mirrors, and the argument checks of gava_mix_clips / gava_mix_targets / gava_soft_criterion, which return
before any launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import REPO
from loss_ref import criterion
from mix_ref import mix_targets, soft_criterion

NAMES = ("gava_mix_clips", "gava_mix_targets", "gava_soft_criterion", "gava_soft_criterion_backward", "gava_mix_struct_sizes")
STRUCTS = ("gava_mix_desc", "gava_mix_clips_args", "gava_mix_targets_args", "gava_soft_criterion_args")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "soft_loss_ref.npz"))


def _sets(gold):
    for s in range(int(gold["n_sets"])):
        weighted, alpha, gamma, beta, scale = gold[f"params_{s}"]
        yield s, gold[f"logits_{s}"], gold[f"targets_{s}"], dict(weighted=bool(weighted), alpha=alpha, gamma=gamma, beta=beta, scale=scale)


# ---- 1, 2. the restatement ------------------------------------------------------------------------------------------------------

def test_fixture_covers_what_it_should(gold):
    shapes, onehot, offsum, tied_t, zero, tied_z, unweighted, gammas = set(), 0, 0, 0, 0, 0, 0, set()
    for s, z, t, kw in _sets(gold):
        shapes.add(z.shape)
        unweighted += not kw["weighted"]
        gammas.add(float(kw["gamma"]))
        for i in range(z.shape[0]):
            st, sz = np.sort(t[i]), np.sort(z[i])
            onehot += st[-1] == 1.0 and st[-2] == 0.0
            offsum += abs(t[i].sum() - 1.0) > 0.1 and t[i].sum() > 0
            tied_t += st[-1] == st[-2] and st[-1] > 0
            zero += not t[i].any()
            tied_z += sz[-1] == sz[-2]
    assert {(5, 4), (7, 3), (3, 65)} <= shapes and gammas == {1.0, 2.0} and unweighted >= 1
    assert min(onehot, offsum, tied_t, zero, tied_z) >= 1
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "soft_loss_ref.npz")) < 100 * 1024


def test_restatement_reproduces_the_reference(gold):
    for s, z, t, kw in _sets(gold):
        got = soft_criterion(z, t, **kw)
        for key in ("per_sample", "weight", "loss", "dlogits"):
            ref = gold[f"{key}_{s}"]
            assert np.abs(got[key] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (s, key)


def test_restatement_on_one_hot_targets_is_the_label_criterion():
    rng = np.random.default_rng(5)
    for B, C, kw in ((6, 5, dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.5)),
                     (4, 3, dict(weighted=True, alpha=0.5, gamma=1.0, beta=0.0, scale=1.0)), (6, 5, dict(weighted=False))):
        z, y = rng.standard_normal((B, C)) * 2.5, rng.integers(0, C, B)
        t = np.zeros((B, C))
        t[np.arange(B), y] = 1.0
        soft, hard = soft_criterion(z, t, g=0.5, **kw), criterion(z, y, g=0.5, **kw)
        for key in ("loss", "per_sample", "weight", "dlogits"):
            assert np.abs(soft[key] - hard[key]).max() <= 1e-12 * max(1.0, np.abs(hard[key]).max()), key
        assert (soft["top1"] == hard["top1"]).all() and (soft["target1"] == y).all() and soft["hits"] == hard["hits"]
        assert (soft["conf"] == hard["conf"]).all()


def test_restatement_gradient_is_the_derivative():
    """Central differences of the restated loss (away from ties, where both argmaxes are locally constant)."""
    rng = np.random.default_rng(3)
    z = rng.standard_normal((5, 6)) * 2
    t = rng.random((5, 6)) * (rng.random((5, 6)) < 0.6)
    kw = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.5)
    g = soft_criterion(z, t, **kw)["dlogits"]
    h = 1e-6
    for i, c in ((0, 0), (2, 3), (4, 5)):
        zp, zm = z.copy(), z.copy()
        zp[i, c] += h; zm[i, c] -= h
        fd = (soft_criterion(zp, t, **kw)["loss"] - soft_criterion(zm, t, **kw)["loss"]) / (2 * h)
        assert abs(fd - g[i, c]) <= 1e-7 * max(1.0, abs(fd))


def test_restated_targets():
    t = mix_targets([0, 2, 9, 1], [3, 1, 2, 0], [0.25, 0.7, 1.0, 0.0], 3, 0.0)
    assert np.array_equal(t, [[0.25, 0.75, 0], [0, 0, 1], [0, 0, 1], [1, 0, 0]])          # 9 is clamped to class 2; clips 1 and 2 are their own partners
    t = mix_targets([0, 1], [1, 0], [0.5, 0.5], 4, 0.2)
    assert np.allclose(t.sum(1), 1.0) and np.allclose(t[0], [0.45, 0.45, 0.05, 0.05]) and np.array_equal(t[0], t[1])


# ---- 3. the plan ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_plan_properties(B, mode):
    from gava_clip_amd import ClipMixer
    H, W = 12, 20
    for seed, kw in enumerate((dict(), dict(mixup_alpha=0.0), dict(cutmix_alpha=0.0), dict(correct_lam=False), dict(prob=0.5))):
        mixer = ClipMixer(5, mode=mode, seed=seed, **kw)
        twin = ClipMixer(5, mode=mode, seed=seed, **kw)
        for _ in range(8):
            plan, again = mixer.draw(B, H, W), twin.draw(B, H, W)
            partner, lam, box = plan["partner"], plan["lam"], plan["box"]
            assert all(np.array_equal(plan[k], again[k]) for k in ("partner", "lam", "box"))      # same seed, same plan
            assert partner.dtype == np.int32 and lam.dtype == np.float32 and box.dtype == np.int32 and box.shape == (B, 4)
            assert np.array_equal(partner, B - 1 - np.arange(B))
            if B % 2:
                assert partner[B // 2] == B // 2                                                 # its own partner
            assert ((lam >= 0) & (lam <= 1)).all()
            y0, y1, x0, x1 = box.T
            assert ((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W)).all()
            boxed = (y1 > y0) & (x1 > x0)
            assert (box[~boxed] == 0).all()
            if kw.get("mixup_alpha", 1) == 0:
                assert (boxed | (lam == 1)).all()                                                # CutMix or nothing
            if kw.get("cutmix_alpha", 1) == 0:
                assert not boxed.any()
            if kw.get("correct_lam", True):
                area = ((y1 - y0) * (x1 - x0))[boxed]
                assert np.array_equal(lam[boxed], (1.0 - area / float(H * W)).astype(np.float32))
            if mode == "batch":
                assert (lam == lam[0]).all() and (box == box[0]).all()
            if mode in ("batch", "pair"):
                assert np.array_equal(lam, lam[::-1]) and np.array_equal(box, box[::-1])
    off = ClipMixer(5, mode=mode, prob=0.0, seed=1).draw(B, H, W)
    assert (off["lam"] == 1).all() and (off["box"] == 0).all()
    none = ClipMixer(5, mode=mode, mixup_alpha=0.0, cutmix_alpha=0.0, seed=1).draw(B, H, W)
    assert (none["lam"] == 1).all() and (none["box"] == 0).all()


def test_plan_modes_differ_and_both_kinds_are_drawn():
    from gava_clip_amd import ClipMixer
    plan = ClipMixer(5, mode="elem", seed=11).draw(64, 16, 16)
    boxed = (plan["box"][:, 1] > plan["box"][:, 0]) & (plan["box"][:, 3] > plan["box"][:, 2])
    assert 8 <= boxed.sum() <= 56 and len(set(plan["lam"].tolist())) > 32
    pair = ClipMixer(5, mode="pair", seed=11).draw(64, 16, 16)
    assert len(set(pair["lam"].tolist())) > 16
    from gava_clip_amd.hip import GavaError
    with pytest.raises(GavaError, match="mode"):
        ClipMixer(5, mode="clip")


# ---- 4, 5. the ABI's surface ----------------------------------------------------------------------------------------------------

def test_new_names_are_exported_and_declared():
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared and hasattr(raw, name), name
    from gava_clip_amd.build import SOURCES
    assert "mix.hip" in SOURCES
    import gava_clip_amd
    assert gava_clip_amd.ClipMixer.__name__ == "ClipMixer" and gava_clip_amd.SoftTargetCriterion.__name__ == "SoftTargetCriterion"


def test_structs_match_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirrors == what the library reports (gava_mix_struct_sizes)."""
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
    assert lib.gava_mix_struct_sizes(got, 4) == 4
    mirrors = (hip.MixDesc, hip.MixClipsArgs, hip.MixTargetsArgs, hip.SoftCriterionArgs)
    assert [ctypes.sizeof(c) for c in mirrors] == sizes == list(got) and sizes[0] == 24
    assert lib.gava_mix_struct_sizes(None, 0) == 4                    # a zero capacity writes nothing
    sizes17 = (ctypes.c_size_t * 32)()
    assert lib.gava_struct_sizes(sizes17, 32) == 17                   # the closed list stays closed


# ---- 6. every refusal returns before a launch -----------------------------------------------------------------------------------

ONE = 1 << 20     # a non-null, 16-byte aligned stand-in for a device pointer: every call below returns before it is used
EINVAL = -1


def _table(B, rows=None):
    from gava_clip_amd import hip
    t = (hip.MixDesc * B)()
    for i in range(B):
        t[i].partner, t[i].lam = B - 1 - i, 0.5
    for i, kw in (rows or {}).items():
        for k, v in kw.items():
            setattr(t[i], k, v)
    return t


def _mix_args(B=4, planes=3, H=8, W=12, rows=None, out=ONE + (1 << 24), **kw):
    from gava_clip_amd import hip
    a = hip.MixClipsArgs()
    table = _table(max(B, 1), rows)
    a.x, a.out, a.desc, a.desc_host = ONE, out, ONE, ctypes.cast(table, ctypes.c_void_p)
    a.B, a.planes, a.H, a.W = B, planes, H, W
    for k, v in kw.items():
        setattr(a, k, v)
    return a, table


def test_mix_clips_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip
    lib = hip.load()
    fn = lib.gava_mix_clips
    assert fn(None, None) == EINVAL
    bad_rows = [{0: dict(partner=4)}, {1: dict(partner=-1)},                                          # partner out of range
                {0: dict(y0=0, y1=9, x0=0, x1=4)}, {0: dict(y0=0, y1=4, x0=0, x1=13)},                 # box outside the image
                {0: dict(y0=-1, y1=4, x0=0, x1=4)}, {0: dict(y0=0, y1=4, x0=-2, x1=4)},
                {2: dict(y0=5, y1=4, x0=0, x1=4)}, {2: dict(y0=0, y1=4, x0=7, x1=6)},                  # inverted
                {3: dict(lam=1.5)}, {3: dict(lam=-0.25)}, {3: dict(lam=float("nan"))}]                 # lam
    for rows in bad_rows:
        a, keep = _mix_args(rows=rows)
        assert fn(ctypes.byref(a), None) == EINVAL, rows
        a, keep = _mix_args(rows=rows, out=ONE)
        assert fn(ctypes.byref(a), None) == EINVAL, rows
    for kw in (dict(B=0), dict(planes=0), dict(H=0), dict(W=0), dict(B=-1), dict(x=None), dict(out=None), dict(desc=None),
               dict(desc_host=None), dict(planes=1 << 20, H=1 << 10, W=1 << 10)):                     # a clip of 2^40 elements
        a, keep = _mix_args(**kw)
        assert fn(ctypes.byref(a), None) == EINVAL, kw
    rotation = {i: dict(partner=(i + 1) % 4) for i in range(4)}
    a, keep = _mix_args(rows=rotation, out=ONE)                                                       # in place, no involution
    assert fn(ctypes.byref(a), None) == EINVAL
    n_bytes = 4 * 3 * 8 * 12 * 4
    for out in (ONE + 16, ONE + n_bytes - 4, ONE - 16, ONE - n_bytes + 4):                            # partial overlap
        a, keep = _mix_args(out=out)
        assert fn(ctypes.byref(a), None) == EINVAL, out - ONE


def test_mix_targets_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip
    lib = hip.load()

    def make(**kw):
        a = hip.MixTargetsArgs()
        a.labels, a.desc, a.targets, a.ld_targets, a.B, a.C, a.smoothing = ONE, ONE, ONE, 5, 4, 5, 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.gava_mix_targets(None, None) == EINVAL
    for kw in (dict(labels=None), dict(desc=None), dict(targets=None), dict(B=0), dict(C=0), dict(ld_targets=4), dict(smoothing=-0.1),
               dict(smoothing=1.5), dict(smoothing=float("nan"))):
        assert lib.gava_mix_targets(ctypes.byref(make(**kw)), None) == EINVAL, kw


def test_soft_criterion_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip
    lib = hip.load()

    def make(**kw):
        a = hip.SoftCriterionArgs()
        for f in ("logits", "targets", "loss", "per_sample", "weight", "top1", "target1", "hits", "saved", "grad_loss", "dlogits"):
            setattr(a, f, ONE)
        a.B, a.C, a.ld_logits, a.ld_targets, a.ld_dlogits, a.weighted = 2, 3, 3, 3, 3, 1
        a.alpha, a.gamma, a.beta, a.scale = 0.25, 2.0, 0.2, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    fwd, bwd = lib.gava_soft_criterion, lib.gava_soft_criterion_backward
    assert fwd(None, None) == EINVAL and bwd(None, None) == EINVAL
    for kw in (dict(gamma=0.5), dict(gamma=float("nan")), dict(C=1, ld_logits=1, ld_targets=1, ld_dlogits=1), dict(B=0), dict(C=0),
               dict(ld_logits=2), dict(ld_targets=2)):
        assert fwd(ctypes.byref(make(**kw)), None) == EINVAL, kw
        assert bwd(ctypes.byref(make(**kw)), None) == EINVAL, kw
    assert bwd(ctypes.byref(make(ld_dlogits=2)), None) == EINVAL
    for f in ("logits", "targets", "loss", "per_sample", "weight", "top1", "target1", "hits", "saved"):
        assert fwd(ctypes.byref(make(**{f: None})), None) == EINVAL, f
    for f in ("logits", "targets", "saved", "grad_loss", "dlogits"):
        assert bwd(ctypes.byref(make(**{f: None})), None) == EINVAL, f


def test_objects_refuse_on_the_host():
    import torch
    from gava_clip_amd import ClipMixer, SoftTargetCriterion
    from gava_clip_amd.hip import GavaError
    with pytest.raises(GavaError, match="gamma"):
        SoftTargetCriterion(focal_ordinal=True, gamma=0.5)
    crit = SoftTargetCriterion(focal_ordinal=True, beta=0.2)
    with pytest.raises(GavaError, match="TrainCriterion"):
        crit(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(GavaError, match="device fp32"):
        crit(torch.zeros(2, 3), torch.full((2, 3), 1 / 3))
    mixer = ClipMixer(3, seed=0)
    with pytest.raises(GavaError, match="device"):
        mixer(torch.zeros(2, 3, 2, 4, 4), torch.zeros(2, dtype=torch.int64))
