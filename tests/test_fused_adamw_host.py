"""CPU: the host side of the fused AdamW step (gava_clip_amd.FusedAdamW, gava_adamw_plan / gava_adamw_step).

The fp64 restatement of the step (tests/optim_ref.py) reproduces torch.optim.AdamW(foreach=False) on float64 tensors to
1e-12 * max(1, |x|): both are fp64 with a different order of a handful of operations.  The GPU tests measure the kernel against
the restatement; this test pins it.  Plus the C ABI's surface (names, struct mirrors, the chunk plan, argument checks that
return before any launch) and the Python refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers import REPO
from optim_ref import adamw_step

NAMES = ("gava_adamw_step", "gava_adamw_plan", "gava_optim_struct_sizes")


def test_restatement_reproduces_torch_adamw():
    rng = np.random.default_rng(11)
    shapes = [(5,), (3, 4), (1,), (7,)]
    p0 = [0.02 * rng.standard_normal(s) for s in shapes]
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]
    group_of = [0, 1, 1, 0]
    tp = [torch.nn.Parameter(torch.tensor(a, dtype=torch.float64)) for a in p0]
    opt = torch.optim.AdamW([dict(params=[tp[0], tp[3]], **groups[0]), dict(params=[tp[1], tp[2]], **groups[1])], foreach=False)
    ref, state = [a.copy() for a in p0], [{} for _ in p0]
    for step in range(5):
        grads = [0.01 * rng.standard_normal(s) for s in shapes]
        grads[2] = None                                            # one parameter never has a gradient
        for q, g in zip(tp, grads):
            q.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        opt.step()
        adamw_step(ref, grads, state, groups, group_of)
    for i, q in enumerate(tp):
        want = q.detach().numpy()
        assert np.abs(ref[i] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), i
        if i == 2:
            assert state[i] == {} and len(opt.state[q]) == 0 and np.array_equal(ref[i], p0[i])
            continue
        assert state[i]["step"] == float(opt.state[q]["step"]) == 5.0
        for key in ("exp_avg", "exp_avg_sq"):
            w = opt.state[q][key].numpy()
            assert np.abs(state[i][key] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (i, key)


def test_restatement_scale_and_found_inf():
    rng = np.random.default_rng(12)
    groups, p0, g = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)], rng.standard_normal(9), rng.standard_normal(9)
    a, sa, b, sb = [p0.copy()], [{}], [p0.copy()], [{}]
    adamw_step(a, [g], sa, groups, [0])
    adamw_step(b, [g * 512.0], sb, groups, [0], grad_scale=512.0, found_inf=0.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(sa[0]["exp_avg_sq"], sb[0]["exp_avg_sq"])
    adamw_step(b, [g], sb, groups, [0], found_inf=1.0)
    assert np.array_equal(a[0], b[0]) and sb[0]["step"] == 1.0


def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    assert "optimizer.hip" in open(os.path.join(REPO, "gava_clip_amd", "build.py")).read()
    from gava_clip_amd.build import SOURCES
    assert "optimizer.hip" in SOURCES
    import gava_clip_amd
    assert gava_clip_amd.FusedAdamW.__name__ == "FusedAdamW" and gava_clip_amd.FusedAdamW._step_supports_amp_scaling is True


def test_optim_structs_match_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirrors == what the library reports (gava_optim_struct_sizes)."""
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    names = {"gava_adamw_tensor": hip.AdamWTensor, "gava_adamw_args": hip.AdamWArgs, "gava_adamw_chunk": hip.AdamWChunk}
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + 'printf("groups %d\\n", GAVA_ADAMW_MAX_GROUPS);return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")]).decode().split()
    sizes = dict(zip(out[::2], map(int, out[1::2])))
    lib = hip.load()
    got = (ctypes.c_size_t * 3)()
    assert lib.gava_optim_struct_sizes(got, 3) == 3
    for (n, cls), sz in zip(names.items(), got):
        assert ctypes.sizeof(cls) == sizes[n] == sz, n
    assert sizes["groups"] == hip.ADAMW_MAX_GROUPS == 8


ONE = 64      # a non-null, aligned stand-in for a device pointer: every call below returns before it is used


def _tensor(hip, n, **kw):
    t = hip.AdamWTensor()
    t.p = t.g = t.m = t.v = t.step = ONE
    t.n = n
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _args(hip, tensors, n_groups=2):
    tab = (hip.AdamWTensor * max(len(tensors), 1))(*tensors)
    a = hip.AdamWArgs()
    a.table, a.table_host, a.chunks = ONE, tab, ONE
    a.n_tensors, a.n_chunks, a.n_groups = len(tensors), 1, n_groups
    for i in range(n_groups):
        a.groups[i].lr, a.groups[i].beta1, a.groups[i].beta2, a.groups[i].eps = 1e-3, 0.9, 0.999, 1e-8
    return a, tab


def test_chunk_plan():
    from gava_clip_amd import hip
    lib = hip.load()
    tensors = [_tensor(hip, 1), _tensor(hip, 196613), _tensor(hip, 128 * 128, rows=128, cols=128, copy_bf16_t=ONE, ld_bf16_t=384),
               _tensor(hip, 80 * 48, rows=80, cols=48, copy_bf16_t=ONE, ld_bf16_t=80), _tensor(hip, 0), _tensor(hip, 9000, g=None)]
    tab = (hip.AdamWTensor * len(tensors))(*tensors)
    want = 1 + 49 + 4 + 2
    assert lib.gava_adamw_plan(tab, len(tensors), 1, None, 0) == want
    ch = (hip.AdamWChunk * want)()
    assert lib.gava_adamw_plan(tab, len(tensors), 1, ch, want) == want
    got = [(c.tensor, c.a, c.b) for c in ch]
    assert got[0] == (0, 0, 1) and got[1] == (1, 0, 4096) and got[49] == (1, 48 * 4096, 196613 - 48 * 4096)
    assert got[50:54] == [(2, 0, 0), (2, 0, 64), (2, 64, 0), (2, 64, 64)] and got[54:] == [(3, 0, 0), (3, 64, 0)]
    covered = sum(c.b for c in ch if c.tensor == 1)
    assert covered == 196613
    assert lib.gava_adamw_plan(tab, len(tensors), 1, ch, 3) == want        # a short buffer is not overrun, the count still comes back
    assert lib.gava_adamw_plan(None, 1, 1, None, 0) == -1 and lib.gava_adamw_plan(tab, len(tensors), 0, None, 0) == -1


def test_step_refuses_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    step = lambda a: lib.gava_adamw_step(ctypes.byref(a), None)
    assert lib.gava_adamw_step(None, None) == -1                                   # null args
    a, _tab = _args(hip, [_tensor(hip, 16)])
    a.table = None
    assert step(a) == -1                                                           # null table with n_tensors > 0
    a, _tab = _args(hip, [_tensor(hip, 16)])
    a.table_host = None
    assert step(a) == -1
    for group in (-1, 2, 8):
        a, _tab = _args(hip, [_tensor(hip, 16), _tensor(hip, 16, group=group)])
        assert step(a) == -1, group                                                # group index out of range
    for n_groups in (0, 9):
        a, _tab = _args(hip, [_tensor(hip, 16)], n_groups=1)
        a.n_groups = n_groups
        assert step(a) == -1, n_groups
    for prec in (-1, 2, 7):
        a, _tab = _args(hip, [_tensor(hip, 16, rows=4, cols=4, copy16=ONE, ld16=4, prec16=prec)])
        assert step(a) == -1, prec                                                 # prec16 outside {F16, BF16}
    for field, ld in (("copy_f32", "ld_f32"), ("copy16", "ld16"), ("copy_bf16", "ld_bf16"), ("copy_bf16_t", "ld_bf16_t")):
        a, _tab = _args(hip, [_tensor(hip, 16, rows=4, cols=5, **{field: ONE, ld: 8})])
        assert step(a) == -1, field                                                # a copy target with rows * cols != n
        a, _tab = _args(hip, [_tensor(hip, 16, rows=2, cols=8, **{field: ONE, ld: 1})])
        assert step(a) == -1, field                                                # rows of the copy would overlap
    a, _tab = _args(hip, [_tensor(hip, 16, m=None)])
    assert step(a) == -1
    a, _tab = _args(hip, [_tensor(hip, 16)])
    a.chunks = None
    assert step(a) == -1
    # nothing to do is not an error and launches nothing: an empty table, and rows * cols is not looked at without a gradient
    a, _tab = _args(hip, [])
    a.table = a.chunks = None
    a.n_chunks = 0
    assert step(a) == 0
    assert lib.gava_adamw_plan((hip.AdamWTensor * 1)(_tensor(hip, 16, g=None, rows=3, cols=3, copy16=ONE, prec16=9)), 1, 1, None, 0) == 0


def test_python_refusals():
    from gava_clip_amd import FusedAdamW, optim
    from gava_clip_amd.hip import GavaError
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(GavaError, match="device"):
        FusedAdamW([w])                                                            # not on the device
    with pytest.raises(GavaError, match="fp32"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(GavaError, match="fp32"):
        FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=1e-3)])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(GavaError, match=flag):
            FusedAdamW([w], **{flag: True})
        with pytest.raises(GavaError, match=flag):
            FusedAdamW([dict(params=[w], **{flag: True})])
    with pytest.raises(GavaError, match="at most 8"):
        FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(2))]) for _ in range(9)])
    sparse = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(GavaError, match="sparse"):
        optim.check_grad(w, sparse)
    with pytest.raises(GavaError, match="gradient"):
        optim.check_grad(w, torch.zeros(4, dtype=torch.float16))
    import inspect
    assert "grad_scaler" not in inspect.signature(FusedAdamW.step).parameters      # GradScaler's deprecated keyword is not taken
