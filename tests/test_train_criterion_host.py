"""CPU: the fp64 restatement of the training criterion (tests/loss_ref.py) reproduces the reference's own criterion under
autograd (tests/golden/loss_ref.npz, written by tools/gen_golden_loss.py from training/loss_utils.py and CrossEntropyLoss in
fp64): values to 1e-12, dlogits to 1e-10.  The GPU tests measure the kernels against the restatement; this test pins the
restatement - the tie row, beta = 0 and the unweighted set included.  Plus the host side of the new C ABI: struct mirrors,
argument checks that return before any launch, the Python refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import REPO
from loss_ref import criterion


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "loss_ref.npz"))


def _sets(gold):
    for s in range(int(gold["n_sets"])):
        weighted, alpha, gamma, beta, scale = gold[f"params_{s}"]
        yield s, gold[f"logits_{s}"], gold[f"labels_{s}"], dict(weighted=bool(weighted), alpha=alpha, gamma=gamma, beta=beta, scale=scale)


def test_fixture_covers_what_it_should(gold):
    shapes, betas, unweighted, tie, sure, far = set(), set(), 0, 0, 0, 0
    for s, z, y, kw in _sets(gold):
        shapes.add(z.shape)
        unweighted += not kw["weighted"]
        if kw["weighted"]:
            betas.add(float(kw["beta"]))
        for i in range(z.shape[0]):
            top = np.sort(z[i])
            tie += top[-1] == top[-2]
            p = np.exp(z[i] - z[i].max()); p /= p.sum()
            sure += (1 - p[y[i]]) < 1e-6
            far += abs(int(y[i]) - int(z[i].argmax())) == z.shape[1] - 1
    assert {c for _, c in shapes} == {3, 4, 400} and {b for b, _ in shapes} == {1, 7}
    assert betas == {0.0, 0.2} and unweighted >= 1 and tie >= 1 and sure >= 1 and far >= 1
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "loss_ref.npz")) < 100 * 1024


def test_restatement_reproduces_the_reference(gold):
    for s, z, y, kw in _sets(gold):
        got = criterion(z, y, **kw)
        for key in ("per_sample", "weight", "loss"):
            ref = gold[f"{key}_{s}"]
            assert np.abs(got[key] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (s, key)
        ref = gold[f"dlogits_{s}"]
        assert np.abs(got["dlogits"] - ref).max() <= 1e-10, s


def test_restatement_gradient_is_the_derivative():
    """Central differences of the restated loss (away from ties, where the argmax is locally constant)."""
    rng = np.random.default_rng(3)
    z, y = rng.standard_normal((5, 6)) * 2, rng.integers(0, 6, 5)
    kw = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.5)
    g = criterion(z, y, **kw)["dlogits"]
    h = 1e-6
    for i, c in ((0, 0), (2, 3), (4, 5)):
        zp, zm = z.copy(), z.copy()
        zp[i, c] += h; zm[i, c] -= h
        fd = (criterion(zp, y, **kw)["loss"] - criterion(zm, y, **kw)["loss"]) / (2 * h)
        assert abs(fd - g[i, c]) <= 1e-7 * max(1.0, abs(fd))


def test_train_structs_match_header_and_library(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "gava_hip.h"\n'
                   'int main(){printf("%zu %zu\\n", sizeof(gava_train_criterion_args), sizeof(gava_train_head_args));return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    c_crit, c_head = map(int, subprocess.check_output([exe]).decode().split())
    assert ctypes.sizeof(hip.TrainCriterionArgs) == c_crit and ctypes.sizeof(hip.TrainHeadArgs) == c_head
    lib = hip.load()
    sizes = (ctypes.c_size_t * 4)()
    assert lib.gava_train_struct_sizes(sizes, 4) == 2 and (sizes[0], sizes[1]) == (c_crit, c_head)
    assert {"gava_train_criterion", "gava_train_criterion_backward", "gava_train_head", "gava_train_head_backward"} <= set(hip.EXPORTS)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every check below returns GAVA_EINVAL on the host, so it runs without a GPU (the pointers are never dereferenced)."""
    from gava_clip_amd import hip
    lib = hip.load()
    einval = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = hip.TrainCriterionArgs()
    assert lib.gava_train_criterion(None, None) == einval and lib.gava_train_criterion_backward(None, None) == einval
    for f in ("logits", "labels", "loss", "per_sample", "weight", "top1", "hits", "saved", "grad_loss", "dlogits"):
        setattr(a, f, p)
    a.B, a.C, a.ld_logits, a.ld_dlogits, a.weighted, a.alpha, a.gamma, a.beta, a.scale = 2, 3, 3, 3, 1, 0.25, 0.5, 0.2, 1.0
    assert lib.gava_train_criterion(ctypes.byref(a), None) == einval            # gamma < 1
    a.gamma, a.C, a.ld_logits = 2.0, 1, 1
    assert lib.gava_train_criterion(ctypes.byref(a), None) == einval            # one class has no ordinal distance
    a.C, a.ld_logits, a.B = 3, 3, 0
    assert lib.gava_train_criterion(ctypes.byref(a), None) == einval
    a.B, a.ld_logits = 2, 2
    assert lib.gava_train_criterion(ctypes.byref(a), None) == einval            # rows overlap
    a.ld_logits = 3
    for f in ("logits", "labels", "loss", "per_sample", "weight", "top1", "hits", "saved"):
        setattr(a, f, None)
        assert lib.gava_train_criterion(ctypes.byref(a), None) == einval, f
        setattr(a, f, p)
    for f in ("logits", "labels", "saved", "grad_loss", "dlogits"):
        setattr(a, f, None)
        assert lib.gava_train_criterion_backward(ctypes.byref(a), None) == einval, f
        setattr(a, f, p)
    h = hip.TrainHeadArgs()
    assert lib.gava_train_head(None, None) == einval and lib.gava_train_head_backward(None, None) == einval
    for f, _ in hip.TrainHeadArgs._fields_:
        if f not in ("B", "C", "P", "E"):
            setattr(h, f, p)
    h.B, h.C, h.P, h.E = 2, 3, 3, 6
    assert lib.gava_train_head(ctypes.byref(h), None) == einval                 # E % 4
    assert lib.gava_train_head_backward(ctypes.byref(h), None) == einval
    h.E = 8
    for f in ("video", "text", "class_offsets", "logit_scale", "logits", "text_features", "video_norm", "text_inv", "class_mean"):
        setattr(h, f, None)
        assert lib.gava_train_head(ctypes.byref(h), None) == einval, f
        setattr(h, f, p)
    for f in ("dlogits", "dvideo", "dtext", "dlogit_scale", "workspace", "video_inv", "text_norm"):
        setattr(h, f, None)
        assert lib.gava_train_head_backward(ctypes.byref(h), None) == einval, f
        setattr(h, f, p)


def test_criterion_refuses_soft_labels_and_small_gamma():
    import torch
    from gava_clip_amd import TrainCriterion
    from gava_clip_amd.hip import GavaError
    with pytest.raises(GavaError, match="gamma"):
        TrainCriterion(focal_ordinal=True, gamma=0.5)
    crit = TrainCriterion(focal_ordinal=True, beta=0.2)
    with pytest.raises(GavaError, match="soft"):
        crit(torch.zeros(2, 3), torch.full((2, 3), 1 / 3))
    with pytest.raises(GavaError, match="device fp32"):
        crit(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_train_head_switch_defaults_and_environment(monkeypatch):
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.config import TINY
    from helpers import model_kwargs
    monkeypatch.delenv("GAVA_TRAIN_HEAD", raising=False)
    assert VitaCLIP(**model_kwargs(TINY)).train_head == "torch"
    monkeypatch.setenv("GAVA_TRAIN_HEAD", "hip")
    assert VitaCLIP(**model_kwargs(TINY)).train_head == "hip"
