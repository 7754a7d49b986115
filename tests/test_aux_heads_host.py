"""CPU: the host side of the auxiliary heads on the device (VitaCLIP.aux_heads, gava_clip_amd.AuxCriterion, the gava_nte_head /
gava_memory_head / gava_sigmoid_criterion / gava_nte_diag_loss entry points).

The fp64 restatement of the sigmoid (focal) loss (tests/aux_ref.py) reproduces the reference's own sigmoid_focal_loss under
autograd (tests/golden/aux_loss_ref.npz, written by tools/gen_golden_aux_loss.py): values to 1e-12, dlogits to 1e-10.  The GPU
tests measure the kernels against the restatement; this test pins it.  Plus the C ABI's surface (names, struct mirrors, argument
checks that return before any launch) and the Python refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from aux_ref import sigmoid_loss
from gava_clip_amd.config import TINY
from helpers import REPO, CLASSES_3, model_kwargs

AUX_NAMES = ("gava_nte_head", "gava_nte_head_backward", "gava_memory_head", "gava_memory_head_backward", "gava_sigmoid_criterion",
             "gava_sigmoid_criterion_backward", "gava_nte_diag_loss", "gava_nte_diag_loss_backward")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "aux_loss_ref.npz"))


def _sets(gold):
    for s in range(int(gold["n_sets"])):
        focal, alpha, gamma, scale = gold[f"params_{s}"]
        yield s, gold[f"logits_{s}"], gold[f"labels_{s}"], dict(use_focal=bool(focal), alpha=alpha, gamma=gamma, scale=scale)


def test_fixture_covers_what_it_should(gold):
    shapes, focal, big, ends = set(), set(), 0, set()
    for s, z, y, kw in _sets(gold):
        shapes.add(z.shape)
        focal.add(kw["use_focal"])
        big += int((np.abs(z) > 29).sum())
        ends |= {("first" if int(v) == 0 else "last") for v in y if int(v) in (0, z.shape[1] - 1)}
    assert {c for _, c in shapes} == {1, 3, 4} and {m for m, _ in shapes} == {1, 7}
    assert focal == {False, True} and big >= 1 and ends == {"first", "last"}
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "aux_loss_ref.npz")) < 100 * 1024


def test_restatement_reproduces_the_reference(gold):
    for s, z, y, kw in _sets(gold):
        got = sigmoid_loss(z, y, **kw)
        for key in ("per_sample", "loss"):
            ref = gold[f"{key}_{s}"]
            assert np.abs(got[key] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (s, key)
        assert np.abs(got["dlogits"] - gold[f"dlogits_{s}"]).max() <= 1e-10, s


def test_restatement_gradient_is_the_derivative():
    rng = np.random.default_rng(5)
    z, y = rng.standard_normal((4, 5)) * 2, rng.integers(0, 5, 4)
    for focal in (False, True):
        kw = dict(use_focal=focal, alpha=0.3, gamma=2.5, scale=1.5)
        g = sigmoid_loss(z, y, **kw)["dlogits"]
        h = 1e-6
        for i, c in ((0, 0), (1, int(y[1])), (3, 4)):
            zp, zm = z.copy(), z.copy()
            zp[i, c] += h; zm[i, c] -= h
            fd = (sigmoid_loss(zp, y, **kw)["loss"] - sigmoid_loss(zm, y, **kw)["loss"]) / (2 * h)
            assert abs(fd - g[i, c]) <= 1e-7 * max(1.0, abs(fd))


def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in AUX_NAMES + ("gava_aux_struct_sizes",):
        assert name in hip.EXPORTS and name in declared, name
    build_src = open(os.path.join(REPO, "gava_clip_amd", "build.py")).read()
    assert "aux_heads.hip" in build_src


def test_aux_structs_match_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirrors == what the library reports (gava_aux_struct_sizes)."""
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    names = {"gava_nte_head_args": hip.NteHeadArgs, "gava_memory_head_args": hip.MemoryHeadArgs,
             "gava_sigmoid_criterion_args": hip.SigmoidCriterionArgs, "gava_nte_diag_args": hip.NteDiagArgs}
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}"
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")]).decode().split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    lib = hip.load()
    got = (ctypes.c_size_t * 4)()
    assert lib.gava_aux_struct_sizes(got, 4) == 4
    for (n, cls), sz in zip(names.items(), got):
        assert ctypes.sizeof(cls) == sizes[n] == sz, n
    assert lib.gava_nte_head_backward_workspace_floats(5, 128) == 5 * (5 + 128 + 3)
    assert lib.gava_memory_head_backward_workspace_floats(7, 3, 128) == 7 * 3 + 3 * 7 * 48 + 3 * 48 + 14


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    for name in AUX_NAMES:
        assert getattr(lib, name)(None, None) == -1, name
    one = ctypes.c_void_p(16)                                     # a non-null, aligned stand-in: the checks below fail before it is used
    s = hip.SigmoidCriterionArgs()
    s.logits = s.labels = s.loss = s.per_sample = s.grad_loss = s.dlogits = one
    s.M, s.C, s.ld_logits, s.ld_dlogits, s.use_focal, s.gamma = 4, 3, 3, 3, 1, 0.5
    assert lib.gava_sigmoid_criterion(ctypes.byref(s), None) == -1             # gamma < 1 with use_focal
    assert lib.gava_sigmoid_criterion_backward(ctypes.byref(s), None) == -1
    s.use_focal, s.ld_logits = 0, 2
    assert lib.gava_sigmoid_criterion(ctypes.byref(s), None) == -1             # rows closer than C
    n = hip.NteHeadArgs()
    for f, _ in hip.NteHeadArgs._fields_:
        if f not in ("B", "D", "E", "K"):
            setattr(n, f, one)
    for B, D, E, K in ((0, 128, 128, 70), (2, 130, 128, 70), (2, 128, 126, 70), (2, 128, 2048, 70), (2, 128, 128, 0)):
        n.B, n.D, n.E, n.K = B, D, E, K
        assert lib.gava_nte_head(ctypes.byref(n), None) == -1, (B, D, E, K)
        assert lib.gava_nte_head_backward(ctypes.byref(n), None) == -1, (B, D, E, K)
    m = hip.MemoryHeadArgs()
    for f, _ in hip.MemoryHeadArgs._fields_:
        if f not in ("M", "S", "C", "E"):
            setattr(m, f, one)
    for M, S, Cn, E in ((0, 5, 3, 128), (2, 0, 3, 128), (2, 5, 0, 128), (2, 5, 3, 120)):
        m.M, m.S, m.C, m.E = M, S, Cn, E
        assert lib.gava_memory_head(ctypes.byref(m), None) == -1, (M, S, Cn, E)
        assert lib.gava_memory_head_backward(ctypes.byref(m), None) == -1, (M, S, Cn, E)
    d = hip.NteDiagArgs()
    d.logits_vm = d.loss = d.grad_loss = d.dlogits_vm = one
    d.B = 0
    assert lib.gava_nte_diag_loss(ctypes.byref(d), None) == -1 and lib.gava_nte_diag_loss_backward(ctypes.byref(d), None) == -1


def test_aux_criterion_refusals():
    from gava_clip_amd import AuxCriterion
    from gava_clip_amd.hip import GavaError
    with pytest.raises(GavaError, match="gamma >= 1"):
        AuxCriterion(sigmoid=True, use_focal=True, gamma=0.5)
    AuxCriterion(sigmoid=True, use_focal=False, gamma=0.5)        # gamma is not used without the focal factor
    z = torch.randn(4, 3)
    for crit in (AuxCriterion(), AuxCriterion(sigmoid=True)):
        with pytest.raises(GavaError, match="soft"):
            crit(logits_mt=z, mt_labels=torch.softmax(z, -1))
        with pytest.raises(GavaError):                            # CPU logits: no fallback
            crit(logits_mt=z, mt_labels=torch.tensor([0, 1, 2, 1]))
        with pytest.raises(GavaError):
            crit(logits_vm=torch.randn(3, 3))
        assert crit() == (None, None)


def test_aux_heads_route_names(monkeypatch):
    from gava_clip_amd import VitaCLIP, hip
    kw = dict(model_kwargs(TINY, CLASSES_3), add_nte=True, use_support_memory=True, num_classes=3)
    m = VitaCLIP(**kw)
    assert m.aux_heads == "torch"
    m.aux_heads = "hip"
    assert m.aux_heads == "hip"
    with pytest.raises(hip.GavaError, match="aux_heads"):
        m.aux_heads = "triton"
    assert m.aux_heads == "hip"
    monkeypatch.setenv("GAVA_AUX_HEADS", "hip")
    assert VitaCLIP(**kw).aux_heads == "hip"
    monkeypatch.setenv("GAVA_AUX_HEADS", "eager")
    with pytest.raises(hip.GavaError, match="aux_heads"):
        VitaCLIP(**kw)


def test_aux_heads_is_validated_on_every_host_class():
    """The switch lives on the class that initialises it, so the stand-alone encoders refuse a bad route as VitaCLIP does."""
    from gava_clip_amd import hip, model
    assert isinstance(vars(model._HipHost)["aux_heads"], property) and "aux_heads" not in vars(model.VitaCLIP)
    host = model._HipHost.__new__(model._HipHost)
    host.aux_heads = "hip"
    with pytest.raises(hip.GavaError, match="aux_heads"):
        host.aux_heads = "eager"
    assert host.aux_heads == "hip"


def test_wrappers_refuse_cpu_tensors():
    from gava_clip_amd import hip
    with pytest.raises(hip.GavaError, match="HIP device"):
        hip.nte_head(torch.randn(2, 128), torch.randn(128, 128), torch.randn(128), torch.randn(2, 70, 128), torch.tensor(100.0))
    with pytest.raises(hip.GavaError, match="HIP device"):
        hip.memory_head(torch.randn(2, 5, 128), torch.randn(3, 128), [torch.randn(32, 128)] * 4, torch.zeros(12, dtype=torch.int64),
                        torch.tensor(100.0))
