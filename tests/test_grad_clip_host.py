"""CPU: the host side of gradient clipping inside the fused AdamW step (gava_grad_norm, gava_adamw_step_clipped,
FusedAdamW(max_grad_norm=...)).

The fp64 restatement (tests/grad_clip_ref.py) reproduces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=False) on
float64 tensors to 1e-12 * max(1, |x|), the bound tests/test_fused_adamw_host.py states for the step alone: both sides are fp64
with a different order of a handful of operations, and the sums of squares here have a few dozen terms.  The GPU tests measure
the kernels against the restatement; this test pins it.  Plus the C ABI's surface (names, the struct mirror, the argument checks
that return before any launch) and the Python side of max_grad_norm."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers import REPO
from grad_clip_ref import clipped_adamw_step, grad_norm

NAMES = ("gava_grad_norm", "gava_adamw_step_clipped", "gava_grad_clip_struct_sizes")
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]
SHAPES = [(5,), (3, 4), (1,), (7,)]
GROUP_OF = [0, 1, 1, 0]


def _grads(rng):
    grads = [0.01 * rng.standard_normal(s) for s in SHAPES]
    grads[2] = None                                                # one parameter never has a gradient
    return grads


@pytest.mark.parametrize("fraction", [0.3, 4.0])                   # max_norm as a fraction of the first step's norm: coef < 1, coef == 1
def test_restatement_reproduces_torch_clip_and_adamw(fraction):
    rng = np.random.default_rng(21)
    p0 = [0.02 * rng.standard_normal(s) for s in SHAPES]
    tp = [torch.nn.Parameter(torch.tensor(a, dtype=torch.float64)) for a in p0]
    opt = torch.optim.AdamW([dict(params=[tp[0], tp[3]], **GROUPS[0]), dict(params=[tp[1], tp[2]], **GROUPS[1])], foreach=False)
    max_norm = fraction * grad_norm(_grads(np.random.default_rng(22)), math.inf)[1]
    rng = np.random.default_rng(22)
    ref, state = [a.copy() for a in p0], [{} for _ in p0]
    for step in range(5):
        grads = _grads(rng)
        for q, g in zip(tp, grads):
            q.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        want_norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False))
        opt.step()
        tn, norm, coef, nonfinite = clipped_adamw_step(ref, grads, state, GROUPS, GROUP_OF, max_norm)
        assert abs(norm - want_norm) <= 1e-12 * want_norm and not nonfinite
        assert (coef < 0.5) if fraction < 1 else (coef == 1.0), coef           # 5 draws of 17 normals: the norm stays within 2x
        for i, g in enumerate(grads):                                          # tp[i].grad now holds the clipped gradient
            if g is None:
                assert tn[i] == 0.0
                continue
            assert abs(tn[i] - np.linalg.norm(g)) <= 1e-12 * tn[i]
            assert np.abs(tp[i].grad.numpy() - g * coef).max() <= 1e-12 * np.abs(g).max()
    for i, q in enumerate(tp):
        want = q.detach().numpy()
        assert np.abs(ref[i] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), i
        if i == 2:
            assert state[i] == {} and np.array_equal(ref[i], p0[i])
            continue
        assert state[i]["step"] == float(opt.state[q]["step"]) == 5.0
        for key in ("exp_avg", "exp_avg_sq"):
            w = opt.state[q][key].numpy()
            assert np.abs(state[i][key] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (i, key)


def test_restatement_scale_skip_and_measure_only():
    rng = np.random.default_rng(23)
    groups, p0, g = [GROUPS[1]], rng.standard_normal(9), rng.standard_normal(9)
    a, sa, b, sb = [p0.copy()], [{}], [p0.copy()], [{}]
    ra = clipped_adamw_step(a, [g], sa, groups, [0], 0.5)
    rb = clipped_adamw_step(b, [g * 512.0], sb, groups, [0], 0.5, grad_scale=512.0, found_inf=0.0)
    assert ra == rb and ra[2] < 1.0 and np.array_equal(a[0], b[0]) and np.array_equal(sa[0]["exp_avg_sq"], sb[0]["exp_avg_sq"])
    assert grad_norm([g * 512.0], 0.5, grad_scale=512.0, fp32_product=True)[1] == grad_norm([g.astype(np.float32)], 0.5)[1]
    # found_inf: nothing changes, the stats are the same
    assert clipped_adamw_step(b, [g], sb, groups, [0], 0.5, found_inf=1.0) == ra
    assert np.array_equal(a[0], b[0]) and sb[0]["step"] == 1.0
    # a non-finite gradient: flag set, coefficient 1, nothing changes
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[4] = bad
        tn, norm, coef, nonfinite = clipped_adamw_step(b, [h], sb, groups, [0], 0.5)
        assert nonfinite and coef == 1.0 and not np.isfinite(norm) and np.array_equal(a[0], b[0]) and sb[0]["step"] == 1.0
    # inf measures only; zeros give norm 0 and coefficient 1; 1e25 squares past fp32 and stays finite
    assert grad_norm([g], math.inf)[2] == 1.0 and grad_norm([np.zeros(4)], 1.0)[1:] == (0.0, 1.0, False)
    tn, norm, coef, nonfinite = grad_norm([np.full(16, 1e25, dtype=np.float32)], 1.0)
    assert not nonfinite and abs(norm - 4.0 * float(np.float32(1e25))) <= 1e-12 * norm and 0.0 < coef < 1e-25


def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    lib = hip.load()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_grad_clip_struct_matches_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirror == what the library reports (gava_grad_clip_struct_sizes);
    the optimizer's own list keeps its three entries."""
    from gava_clip_amd import hip
    names = {"gava_grad_norm_args": hip.GradNormArgs, "gava_adamw_args": hip.AdamWArgs, "gava_adamw_tensor": hip.AdamWTensor}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gava_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + \
        'printf("max_norm %zu\\n", offsetof(gava_grad_norm_args, max_norm));printf("stats %zu\\n", offsetof(gava_grad_norm_args, stats));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")]).decode().split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    lib = hip.load()
    got = (ctypes.c_size_t * 4)()
    assert lib.gava_grad_clip_struct_sizes(got, 4) == 1 and got[0] == sizes["gava_grad_norm_args"] == ctypes.sizeof(hip.GradNormArgs)
    assert lib.gava_grad_clip_struct_sizes(got, 0) == 1
    assert sizes["max_norm"] == hip.GradNormArgs.max_norm.offset and sizes["stats"] == hip.GradNormArgs.stats.offset
    assert lib.gava_optim_struct_sizes(got, 4) == 3
    assert [got[0], got[1]] == [sizes["gava_adamw_tensor"], sizes["gava_adamw_args"]] == [ctypes.sizeof(hip.AdamWTensor), ctypes.sizeof(hip.AdamWArgs)]


ONE = 64      # a non-null, aligned stand-in for a device pointer: every call below returns before it is used


def _tensor(hip, n, **kw):
    t = hip.AdamWTensor()
    t.p = t.g = t.m = t.v = t.step = ONE
    t.n = n
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _norm_args(hip, tensors, n_groups=2, **kw):
    tab = (hip.AdamWTensor * max(len(tensors), 1))(*tensors)
    a = hip.GradNormArgs()
    a.table, a.table_host, a.chunks = ONE, tab, ONE
    a.n_tensors, a.n_chunks, a.n_groups = len(tensors), 1, n_groups
    a.max_norm, a.workspace, a.tensor_norm, a.stats = 1.0, ONE, ONE, ONE
    for k, v in kw.items():
        setattr(a, k, v)
    return a, tab


def test_grad_norm_refuses_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    norm = lambda a: lib.gava_grad_norm(ctypes.byref(a), None)
    assert lib.gava_grad_norm(None, None) == -1                                    # null args
    for field in ("table", "table_host", "chunks", "stats", "workspace"):
        a, _tab = _norm_args(hip, [_tensor(hip, 16)], **{field: None})
        assert norm(a) == -1, field
    for bad in (0.0, -0.0, -1.0, -math.inf, math.nan):
        a, _tab = _norm_args(hip, [_tensor(hip, 16)], max_norm=bad)
        assert norm(a) == -1, bad
    a, _tab = _norm_args(hip, [_tensor(hip, 16)], n_chunks=-1)
    assert norm(a) == -1
    a, _tab = _norm_args(hip, [_tensor(hip, 16)], workspace=ONE + 4)               # doubles live there
    assert norm(a) == -1
    # whatever the step's table check rejects
    for group in (-1, 2, 8):
        a, _tab = _norm_args(hip, [_tensor(hip, 16), _tensor(hip, 16, group=group)])
        assert norm(a) == -1, group
    for n_groups in (0, 9):
        a, _tab = _norm_args(hip, [_tensor(hip, 16)], n_groups=n_groups)
        assert norm(a) == -1, n_groups
    a, _tab = _norm_args(hip, [_tensor(hip, -1)])
    assert norm(a) == -1
    for kw in (dict(m=None), dict(rows=4, cols=5, copy_bf16_t=ONE, ld_bf16_t=8), dict(rows=2, cols=8, copy_bf16_t=ONE, ld_bf16_t=1),
               dict(rows=4, cols=4, copy16=ONE, ld16=4, prec16=7)):
        a, _tab = _norm_args(hip, [_tensor(hip, 16, **kw)])
        assert norm(a) == -1, kw
    # nothing to do and nothing to write is not an error and launches nothing
    a, _tab = _norm_args(hip, [], table=None, chunks=None, n_chunks=0, stats=None, workspace=None, tensor_norm=None, max_norm=math.inf)
    assert norm(a) == 0


def test_clipped_step_refuses_bad_arguments_before_any_launch():
    from gava_clip_amd import hip
    lib = hip.load()

    def args(tensors, n_groups=2):
        tab = (hip.AdamWTensor * max(len(tensors), 1))(*tensors)
        a = hip.AdamWArgs()
        a.table, a.table_host, a.chunks = ONE, tab, ONE
        a.n_tensors, a.n_chunks, a.n_groups = len(tensors), 1, n_groups
        return a, tab

    a, _tab = args([_tensor(hip, 16)])
    assert lib.gava_adamw_step_clipped(ctypes.byref(a), None, None) == -1          # null stats, everything else in order
    assert lib.gava_adamw_step_clipped(None, ONE, None) == -1
    for field in ("table", "table_host", "chunks"):
        a, _tab = args([_tensor(hip, 16)])
        setattr(a, field, None)
        assert lib.gava_adamw_step_clipped(ctypes.byref(a), ONE, None) == -1, field
    a, _tab = args([_tensor(hip, 16, group=2)])
    assert lib.gava_adamw_step_clipped(ctypes.byref(a), ONE, None) == -1
    a, _tab = args([])
    a.table = a.chunks = None
    a.n_chunks = 0
    assert lib.gava_adamw_step_clipped(ctypes.byref(a), ONE, None) == 0            # an empty table: nothing to do, as for the plain step


def test_max_grad_norm_validation():
    from gava_clip_amd import FusedAdamW, optim
    from gava_clip_amd.hip import GavaError
    w = torch.nn.Parameter(torch.zeros(4))
    for bad in (0, 0.0, -1.0, -math.inf, math.nan, True, "1.0", [1.0], torch.ones(1)):
        with pytest.raises(GavaError, match="max_grad_norm"):
            optim.check_max_grad_norm(bad)
        with pytest.raises(GavaError, match="max_grad_norm"):
            FusedAdamW([w], max_grad_norm=bad)                                     # refused before anything else is looked at
    with pytest.raises(TypeError):
        FusedAdamW([w], 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, False, False, False, 1.0)      # keyword-only
    assert optim.check_max_grad_norm(None) is None and optim.check_max_grad_norm(2) == 2.0
    assert optim.check_max_grad_norm(math.inf) == math.inf and optim.check_max_grad_norm(1e-3) == 1e-3


def _host_optimizer(monkeypatch, **kw):
    """A FusedAdamW over host tensors: construction and state handling launch nothing, only the device check stands in the way."""
    from gava_clip_amd import FusedAdamW, optim
    monkeypatch.setattr(optim, "check_param", lambda p: None)
    ps = [torch.nn.Parameter(torch.full(s, 0.5)) for s in [(6,), (2, 3), (1,)]]
    return ps, FusedAdamW([dict(params=ps[:2], lr=1e-3), dict(params=ps[2:], lr=3e-4, weight_decay=0.2)], **kw)


def test_max_grad_norm_is_an_attribute_and_nothing_else(monkeypatch):
    from gava_clip_amd.hip import GavaError
    ps, opt = _host_optimizer(monkeypatch, max_grad_norm=1.5)
    _ps, plain = _host_optimizer(monkeypatch)
    assert opt.max_grad_norm == 1.5 and plain.max_grad_norm is None and opt.last == {} and opt.grad_norms() == {}
    assert all("max_grad_norm" not in g for g in opt.param_groups) and "max_grad_norm" not in opt.defaults
    assert [sorted(g) for g in opt.param_groups] == [sorted(g) for g in plain.param_groups]
    sd, sp = opt.state_dict(), plain.state_dict()
    assert set(sd) == set(sp) == {"state", "param_groups"} and sd["param_groups"] == sp["param_groups"]
    assert "max_grad_norm" not in repr(sd)
    opt.max_grad_norm = math.inf                                                   # settable between steps, checked when set
    assert opt.max_grad_norm == math.inf
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None
    with pytest.raises(GavaError, match="max_grad_norm"):
        opt.max_grad_norm = -2.0
    assert opt.max_grad_norm is None
    plain.load_state_dict(sd)
    assert plain.max_grad_norm is None                                             # loading does not carry it either


def test_state_dict_written_with_clipping_on_loads_into_torch_adamw(monkeypatch):
    ps, opt = _host_optimizer(monkeypatch, max_grad_norm=0.25)
    steps = torch.zeros(len(ps))
    for i, p in enumerate(ps[:2]):                                                 # the state a step leaves: a view of one step vector, two moments
        steps[i] = 3.0
        opt.state[p] = dict(step=steps[i], exp_avg=torch.full_like(p, 0.01), exp_avg_sq=torch.full_like(p, 1e-4))
    sd = opt.state_dict()
    assert len(sd["state"]) == 2 and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = torch.optim.AdamW([dict(params=qs[:2]), dict(params=qs[2:])], foreach=False)
    topt.load_state_dict(sd)
    assert [g["lr"] for g in topt.param_groups] == [1e-3, 3e-4] and topt.param_groups[1]["weight_decay"] == 0.2
    for q in qs:
        q.grad = torch.full_like(q, 0.1)
    topt.step()
    assert [float(topt.state[q]["step"]) for q in qs] == [4.0, 4.0, 1.0]
    assert all(not torch.equal(q, p) for q, p in zip(qs, ps))
    # and back: torch's state dict loads into an optimizer that clips
    ps2, back = _host_optimizer(monkeypatch, max_grad_norm=0.25)
    back.load_state_dict(topt.state_dict())
    assert back.max_grad_norm == 0.25 and [float(back.state[p]["step"]) for p in ps2] == [4.0, 4.0, 1.0]
