"""GPU: clipping by global norm inside the fused AdamW step (gava_grad_norm, gava_adamw_step_clipped, FusedAdamW(max_grad_norm=...))
against the fp64 restatement tests/grad_clip_ref.py.

Tolerances.
  Norms and the coefficient: one fp32 ulp of the reference value.  The kernels accumulate exact squares of fp32 values in
  double, at most 2^25 terms here, so the sum's relative error stays below 2^25 * 2^-53 < 4e-9, far under 2^-24; what is left is
  the one rounding of the square root (or of the quotient) to fp32, and a reference that sits within 4e-9 of a rounding boundary
  may land on the neighbour.
  The clipped trajectory: the rule tests/test_gpu_fused_adamw.py states, with torch's clip_grad_norm_ + AdamW in fp32 on the
  same device as the other leg:  max |fused - ref| <= 2 * max |torch - ref| + one fp32 ulp of the largest |ref|.
  Everything else is bit for bit.

The shape set is the chunk geometry's edge list: linear tensors of 1, 7, 8, 9, 4095, 4096, 4097 and 2 * 4096 + 3 elements
(a lane's group of 8, a chunk of 4096 and their neighbours), tensors with a transposed copy of 64 x 64, 65 x 63 and 130 x 70
(the tile form: whole, ragged in both directions, several tiles), two param groups, an entry without a gradient, an entry
with no elements, and two entries whose gradient and parameter sit one element past a 16-byte boundary."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import FusedAdamW, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from grad_clip_ref import clipped_adamw_step, grad_norm  # noqa: E402
from helpers import synth_torch_state  # noqa: E402
from test_gpu_fused_adamw import GROUPS, _check_rule, _make_model, _offset_one, _values  # noqa: E402

# (shape, group, kind): "tile" carries copy_bf16_t (and the three row-major copies), "none" has g == NULL, "off" is misaligned
ENTRIES = [((1,), 0, ""), ((7,), 1, ""), ((64, 64), 0, "tile"), ((8,), 1, ""), ((9,), 0, ""), ((33,), 1, "none"), ((4095,), 0, ""),
           ((65, 63), 1, "tile"), ((4096,), 0, ""), ((0,), 1, ""), ((4097,), 1, "off"), ((130, 70), 0, "tile off"), ((2 * 4096 + 3,), 1, "")]
GROUP_OF = [e[1] for e in ENTRIES]
N_TOTAL = sum(int(np.prod(s)) for s, _g, kind in ENTRIES if kind != "none")
SENTINEL16 = 0x7A5C


def _dev(t, kind):
    if t.numel() == 0:
        return torch.zeros(1, device="cuda")[:0]           # no elements, a real address (_ptr)
    return _offset_one(t) if "off" in kind else t.cuda()


def _ptr(t):
    """data_ptr() of a tensor without elements is null: such an entry points at the element its view starts from."""
    return t.data_ptr() if t.numel() else t._base.data_ptr()


class _Set:
    """The table's tensors on the device.  grad(i, shape) -> fp32 host tensor; the state starts as after three steps."""

    def __init__(self, grad, seed=0):
        self.p, self.g, self.m, self.v, self.copies, descs = [], [], [], [], [], []
        self.steps = torch.full((len(ENTRIES),), 3.0, device="cuda")
        for i, (shape, group, kind) in enumerate(ENTRIES):
            n = int(np.prod(shape))
            self.p.append(_dev(_values(seed + 10 * i, shape, 0.02), kind))
            self.m.append(_values(seed + 10 * i + 1, shape, 0.01).cuda() if n else _dev(torch.empty(0), kind))
            self.v.append((_values(seed + 10 * i + 2, shape, 0.01) ** 2 + 1e-6).cuda() if n else _dev(torch.empty(0), kind))
            self.g.append(None if kind == "none" else _dev(grad(i, shape).float(), kind))
            d = hip.AdamWTensor()
            d.p, d.m, d.v, d.step = _ptr(self.p[i]), _ptr(self.m[i]), _ptr(self.v[i]), self.steps.data_ptr() + 4 * i
            d.g = None if self.g[i] is None else _ptr(self.g[i])
            d.n, d.group = n, group
            if "tile" in kind:
                rows, cols = shape
                c16, cb = (torch.full((rows, cols + 8), SENTINEL16, dtype=torch.int16, device="cuda") for _ in range(2))
                cbt = torch.full((cols, rows + 8), SENTINEL16, dtype=torch.int16, device="cuda")
                c32 = torch.full((rows, cols + 4), 12345.0, device="cuda")
                d.rows, d.cols, d.prec16 = rows, cols, hip.PREC_F16
                d.copy16, d.ld16, d.copy_bf16, d.ld_bf16 = c16.data_ptr(), cols + 8, cb.data_ptr(), cols + 8
                d.copy_bf16_t, d.ld_bf16_t, d.copy_f32, d.ld_f32 = cbt.data_ptr(), rows + 8, c32.data_ptr(), cols + 4
                self.copies += [c16, cb, cbt, c32]
            descs.append(d)
        lib = hip.load()
        self.tab = (hip.AdamWTensor * len(descs))(*descs)
        self.n_chunks = lib.gava_adamw_plan(self.tab, len(descs), 2, None, 0)
        assert self.n_chunks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1 + 2 + 6 + 3       # per entry with elements and a gradient, in table order
        chunks = (hip.AdamWChunk * self.n_chunks)()
        assert lib.gava_adamw_plan(self.tab, len(descs), 2, chunks, self.n_chunks) == self.n_chunks
        self.dev = torch.frombuffer(bytearray(bytes(self.tab) + bytes(chunks)), dtype=torch.uint8).cuda()
        # the outputs and the workspace start as NaN: nothing may rely on a memset or on an earlier call
        self.ws = torch.full((self.n_chunks + len(descs),), math.nan, dtype=torch.float64, device="cuda")
        self.tensor_norm = torch.full((len(descs),), math.nan, device="cuda")
        self.stats = torch.full((4,), math.nan, device="cuda")

    def state(self):
        return self.p + self.m + self.v + [self.steps] + self.copies

    def grads64(self):
        return [None if g is None else g.double().cpu().numpy() for g in self.g]

    def norm(self, max_norm, grad_scale=None, tensor_norm=True):
        a = hip.GradNormArgs()
        a.table, a.table_host, a.chunks = self.dev.data_ptr(), self.tab, self.dev.data_ptr() + C.sizeof(self.tab)
        a.n_tensors, a.n_chunks, a.n_groups = len(self.tab), self.n_chunks, 2
        a.grad_scale, a.max_norm = hip.ptr(grad_scale), max_norm
        a.workspace, a.stats = self.ws.data_ptr(), self.stats.data_ptr()
        a.tensor_norm = self.tensor_norm.data_ptr() if tensor_norm else None
        hip.check(hip.load().gava_grad_norm(C.byref(a), hip.stream_ptr()), "gava_grad_norm")
        torch.cuda.synchronize()
        return self.stats.cpu().numpy(), self.tensor_norm.cpu().numpy()

    def step(self, clipped, grad_scale=None, found_inf=None):
        a = hip.AdamWArgs()
        a.table, a.table_host, a.chunks = self.dev.data_ptr(), self.tab, self.dev.data_ptr() + C.sizeof(self.tab)
        a.n_tensors, a.n_chunks, a.n_groups = len(self.tab), self.n_chunks, 2
        for k, g in enumerate(GROUPS):
            a.groups[k].lr, a.groups[k].eps, a.groups[k].weight_decay = g["lr"], g["eps"], g["weight_decay"]
            a.groups[k].beta1, a.groups[k].beta2 = g["betas"]
        a.grad_scale, a.found_inf = hip.ptr(grad_scale), hip.ptr(found_inf)
        lib = hip.load()
        if clipped:
            hip.check(lib.gava_adamw_step_clipped(C.byref(a), self.stats.data_ptr(), hip.stream_ptr()), "gava_adamw_step_clipped")
        else:
            hip.check(lib.gava_adamw_step(C.byref(a), hip.stream_ptr()), "gava_adamw_step")
        torch.cuda.synchronize()


def _seeded(i, shape):
    g = _values(500 + i, shape, 0.01)
    if g.numel() > 2:
        g.view(-1)[::7] = 0.0
    return g


def _ones(i, shape):
    return torch.ones(shape)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _stepped(s):
    """The step counts say which entries a step touched: all with a gradient, or none."""
    got = s.steps.tolist()
    if got == [3.0] * len(ENTRIES):
        return False
    assert got == [3.0 if kind == "none" else 4.0 for _s, _g, kind in ENTRIES]
    return True


# ---- the norm ----------------------------------------------------------------------------------------------------------------

def test_every_element_is_counted_exactly_once():
    s = _Set(_ones)
    stats, tn = s.norm(math.inf)
    for i, (shape, _g, kind) in enumerate(ENTRIES):
        n = 0 if kind == "none" else int(np.prod(shape))
        assert tn[i] == np.float32(math.sqrt(n)) and round(float(tn[i]) ** 2) == n, (i, shape, tn[i])
    assert stats[0] == np.float32(math.sqrt(N_TOTAL)) and round(float(stats[0]) ** 2) == N_TOTAL
    assert stats.tolist()[1:] == [1.0, 0.0, 0.0]
    sums = s.ws.cpu().numpy()                                                  # the workspace: chunk partials, then tensor sums
    assert sums[:s.n_chunks].sum() == N_TOTAL and sums[s.n_chunks:].sum() == N_TOTAL and sums[:s.n_chunks].max() <= 4096
    # through the optimizer, the linear shapes and two groups
    ps = [torch.nn.Parameter(_dev(_values(i, shape, 0.02), kind)) for i, (shape, _g, kind) in enumerate(ENTRIES) if "tile" not in kind and shape != (0,)]
    kinds = [kind for shape, _g, kind in ENTRIES if "tile" not in kind and shape != (0,)]
    for p, kind in zip(ps, kinds):
        p.grad = None if kind == "none" else _dev(torch.ones(p.shape), kind)
    opt = FusedAdamW([dict(params=ps[::2], **GROUPS[0]), dict(params=ps[1::2], **GROUPS[1])], max_grad_norm=math.inf)
    opt.step()
    norms = opt.grad_norms()
    assert set(norms) == set(ps)
    for p, kind in zip(ps, kinds):
        n = 0 if kind == "none" else p.numel()
        assert norms[p].ndim == 0 and float(norms[p]) == float(np.float32(math.sqrt(n))), (tuple(p.shape), float(norms[p]))
    total = sum(p.numel() for p, kind in zip(ps, kinds) if kind != "none")
    assert float(opt.last["grad_norm"]) == float(np.float32(math.sqrt(total)))
    assert float(opt.last["clip_coef"]) == 1.0 and float(opt.last["nonfinite"]) == 0.0


@pytest.mark.parametrize("grad_scale", [None, 1000.0])
def test_norm_and_coefficient_within_one_ulp(grad_scale):
    scale = 1.0 if grad_scale is None else grad_scale
    s = _Set(lambda i, shape: _seeded(i, shape) * scale)
    gs = None if grad_scale is None else torch.full((1,), grad_scale, device="cuda")
    grads = [None if g is None else g.cpu().numpy() for g in s.g]
    _tn, ref_norm, _c, _nf = grad_norm(grads, math.inf, grad_scale, fp32_product=True)
    for max_norm in (0.3 * ref_norm, 3.0 * ref_norm):
        tn_ref, norm, coef, nonfinite = grad_norm(grads, max_norm, grad_scale, fp32_product=True)
        stats, tn = s.norm(max_norm, gs)
        print(f"norm {stats[0]!r} ref {norm!r}  coef {stats[1]!r} ref {coef!r}")
        assert abs(float(stats[0]) - norm) <= _ulp(norm) and abs(float(stats[1]) - coef) <= _ulp(coef)
        assert (coef < 0.31) == (max_norm < ref_norm) and stats[2] == 0.0 and stats[3] == 0.0 and not nonfinite
        for i, r in enumerate(tn_ref):
            assert abs(float(tn[i]) - r) <= _ulp(r), (i, tn[i], r)
    stats2, _ = s.norm(3.0 * ref_norm, gs, tensor_norm=False)                      # tensor_norm is optional
    assert np.array_equal(stats, stats2)


def test_squares_past_fp32_and_zeros():
    s = _Set(lambda i, shape: torch.full(shape, 1e25))
    big = float(np.float32(1e25))
    stats, tn = s.norm(1.0)
    ref = math.sqrt(N_TOTAL) * big
    assert math.isfinite(float(stats[0])) and abs(float(stats[0]) - ref) <= _ulp(ref)
    assert abs(float(stats[1]) - 1.0 / ref) <= _ulp(1.0 / ref) and stats[2] == 0.0
    assert abs(float(tn[8]) - 64.0 * big) <= _ulp(64.0 * big)
    s.step(clipped=True)
    assert _stepped(s)
    z = _Set(lambda i, shape: torch.zeros(shape))
    before = [t.clone() for t in z.state()]
    stats, tn = z.norm(1.0)
    assert stats.tolist() == [0.0, 1.0, 0.0, 0.0] and not tn.any()
    z.step(clipped=True)
    assert _stepped(z)                                                         # the step runs: counts go up, the second group decays
    assert not torch.equal(z.p[12], before[12])


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
@pytest.mark.parametrize("where", [(6, 4094), (11, 130 * 70 - 1)])              # last element of a linear chunk; last of a ragged tile
def test_one_nonfinite_gradient_skips_the_step(bad, where):
    i, e = where

    def grad(j, shape):
        g = _seeded(j, shape)
        if j == i:
            g.view(-1)[e] = bad
        return g

    s = _Set(grad)
    before = [t.clone() for t in s.state()]
    stats, tn = s.norm(0.01)
    assert stats[2] == 1.0 and stats[1] == 1.0 and stats[3] == 0.0 and not math.isfinite(float(stats[0]))
    assert not math.isfinite(float(tn[i])) and all(math.isfinite(float(t)) for j, t in enumerate(tn) if j != i)
    s.step(clipped=True)
    assert not _stepped(s) and _same(s.state(), before)


# ---- the clipped step ---------------------------------------------------------------------------------------------------------

def test_coefficient_one_is_the_plain_step_bit_for_bit():
    plain = _Set(_seeded)
    plain.step(clipped=False)
    assert _stepped(plain)
    ref_norm = grad_norm(plain.grads64(), math.inf)[1]
    for max_norm in (math.inf, 1.5 * ref_norm):
        s = _Set(_seeded)
        stats, _ = s.norm(max_norm)
        assert stats[1] == 1.0
        s.step(clipped=True)
        assert _same(s.state(), plain.state()), max_norm
    clipped = _Set(_seeded)                                                    # and below the norm it is not
    assert clipped.norm(0.3 * ref_norm)[0][1] < 0.31
    clipped.step(clipped=True)
    assert _stepped(clipped) and not torch.equal(clipped.p[12], plain.p[12])


def test_power_of_two_scale_is_exact():
    a = _Set(_seeded)
    ref_norm = grad_norm(a.grads64(), math.inf)[1]
    stats_a, tn_a = a.norm(0.3 * ref_norm)
    a.step(clipped=True)
    b = _Set(lambda i, shape: _seeded(i, shape) * 2.0 ** 12)
    scale = torch.full((1,), 2.0 ** 12, device="cuda")
    stats_b, tn_b = b.norm(0.3 * ref_norm, scale)
    b.step(clipped=True, grad_scale=scale, found_inf=torch.zeros(1, device="cuda"))
    assert stats_a[1] < 0.31 and np.array_equal(stats_a, stats_b) and np.array_equal(tn_a, tn_b)
    assert _stepped(a) and _same(a.state(), b.state())


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        s = _Set(_seeded)
        stats, tn = s.norm(0.02)
        s.step(clipped=True)
        runs.append((stats, tn, s.ws.clone(), s.state()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][0][1] < 1.0
    assert torch.equal(runs[0][2], runs[1][2]) and _same(runs[0][3], runs[1][3])


def test_found_inf_with_finite_gradients_changes_nothing_but_the_stats():
    s = _Set(_seeded)
    want, want_tn = _Set(_seeded).norm(0.02)
    before = [t.clone() for t in s.state()]
    stats, tn = s.norm(0.02)
    s.step(clipped=True, found_inf=torch.ones(1, device="cuda"))
    assert np.array_equal(stats, want) and np.array_equal(tn, want_tn) and stats[2] == 0.0 and 0.0 < stats[1] < 1.0
    assert not _stepped(s) and _same(s.state(), before)
    s.step(clipped=True, found_inf=torch.zeros(1, device="cuda"))
    assert _stepped(s)


# ---- through FusedAdamW -----------------------------------------------------------------------------------------------------

T_SHAPES = [(4095,), (7,), (4097,), (2 * 4096 + 3,), (33,), (4096,), (1,)]      # (4097,) at storage offset 1, (33,) without a gradient
T_GROUP_OF = [0, 1, 0, 1, 1, 0, 1]
T_NONE, T_OFF = 4, 2


def _t_params():
    return [torch.nn.Parameter(_offset_one(_values(i, s, 0.02)) if i == T_OFF else _values(i, s, 0.02).cuda()) for i, s in enumerate(T_SHAPES)]


def _t_grad(step, i):
    return _values(2000 * (step + 1) + i, T_SHAPES[i], 0.01)


def _t_groups(ps):
    return [dict(params=[p for p, gi in zip(ps, T_GROUP_OF) if gi == k], **GROUPS[k]) for k in range(2)]


def test_five_clipped_steps_match_torch_within_its_own_error():
    grads = [[None if i == T_NONE else _t_grad(step, i) for i in range(len(T_SHAPES))] for step in range(5)]
    max_norm = 0.3 * grad_norm([None if g is None else g.numpy() for g in grads[0]], math.inf)[1]
    fps, tps = _t_params(), [torch.nn.Parameter(p.detach().clone()) for p in _t_params()]
    fopt, topt = FusedAdamW(_t_groups(fps), max_grad_norm=max_norm), torch.optim.AdamW(_t_groups(tps), foreach=False)
    ref, state = [_values(i, s, 0.02).double().numpy() for i, s in enumerate(T_SHAPES)], [{} for _ in T_SHAPES]
    for step in range(5):
        for ps in (fps, tps):
            for i, p in enumerate(ps):
                p.grad = None if grads[step][i] is None else (_offset_one(grads[step][i]) if i == T_OFF and ps is fps else grads[step][i].cuda())
        held = [None if p.grad is None else p.grad.clone() for p in fps]
        fopt.step()
        assert all(g is None or torch.equal(p.grad, g) for p, g in zip(fps, held))       # the gradient is read only
        torch.nn.utils.clip_grad_norm_(tps, max_norm, foreach=False)
        topt.step()
        tn, norm, coef, nonfinite = clipped_adamw_step(ref, [None if g is None else g.double().numpy() for g in grads[step]], state,
                                                       GROUPS, T_GROUP_OF, max_norm)
        assert coef < 0.5 and not nonfinite
        assert abs(float(fopt.last["grad_norm"]) - norm) <= _ulp(norm) and abs(float(fopt.last["clip_coef"]) - coef) <= _ulp(coef)
        got = fopt.grad_norms()
        assert all(abs(float(got[p]) - tn[i]) <= _ulp(tn[i]) for i, p in enumerate(fps))
    idx = [i for i in range(len(T_SHAPES)) if i != T_NONE]
    _check_rule([fps[i].detach().cpu().numpy() for i in idx], [tps[i].detach().cpu().numpy() for i in idx], [ref[i] for i in idx], "p")
    for key in ("exp_avg", "exp_avg_sq"):
        _check_rule([fopt.state[fps[i]][key].cpu().numpy() for i in idx], [topt.state[tps[i]][key].cpu().numpy() for i in idx],
                    [state[i][key] for i in idx], key)
    assert all(float(fopt.state[fps[i]]["step"]) == 5.0 for i in idx) and len(fopt.state[fps[T_NONE]]) == 0


def _scaled_backward(scaler, ps, w):
    for p in ps:
        p.grad = None
    scaler.scale(sum((p * q).sum() for p, q in zip(ps, w))).backward()


@pytest.mark.parametrize("max_norm_fraction", [0.3, math.inf])
def test_grad_scaler_round_trip_with_and_without_unscale(max_norm_fraction):
    shapes = [(300,), (40, 24), (1,), (4097,)]
    w = [_values(60 + i, s, 0.01).cuda() for i, s in enumerate(shapes)]             # the unscaled gradient of sum(p * w) is w
    tn_ref, norm, _c, _nf = grad_norm([q.cpu().numpy() for q in w], math.inf)
    max_norm = max_norm_fraction * norm
    coef = grad_norm([q.cpu().numpy() for q in w], max_norm)[2]
    results = []
    for unscale in (False, True):
        ps = [torch.nn.Parameter(_values(50 + i, s, 0.02).cuda()) for i, s in enumerate(shapes)]
        opt = FusedAdamW(ps, lr=1e-3, max_grad_norm=max_norm)
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
        _scaled_backward(scaler, ps, w)
        if unscale:
            scaler.unscale_(opt)
            assert all(torch.equal(p.grad, q) for p, q in zip(ps, w))
        held = [p.grad.clone() for p in ps]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)                                                        # no host wait with the clip on either
        finally:
            torch.cuda.set_sync_debug_mode("default")
        scaler.update()
        assert all(torch.equal(p.grad, g) for p, g in zip(ps, held))                # p.grad is never written
        assert not hasattr(opt, "grad_scale") and scaler.get_scale() == 2.0 ** 16
        assert abs(float(opt.last["grad_norm"]) - norm) <= _ulp(norm) and abs(float(opt.last["clip_coef"]) - coef) <= _ulp(coef)
        assert float(opt.last["nonfinite"]) == 0.0 and (coef < 0.31 or max_norm_fraction == math.inf)
        got = opt.grad_norms()
        assert all(abs(float(got[p]) - r) <= _ulp(r) for p, r in zip(ps, tn_ref))
        for p, q in zip(ps, w):                                                     # exp_avg = (1 - beta1) * the clipped unscaled gradient
            assert torch.allclose(opt.state[p]["exp_avg"], q * (0.1 * coef), rtol=2e-6, atol=0.0)
        results.append([p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in ("exp_avg", "exp_avg_sq")]
                       + [opt.last[k].clone() for k in ("grad_norm", "clip_coef")])
        # a non-finite gradient: skipped on the device, the scale backs off, the flag is up
        _scaled_backward(scaler, ps, w)
        ps[1].grad[3, 5] = float("inf")
        if unscale:
            scaler.unscale_(opt)
        after = [p.detach().clone() for p in ps]
        scaler.step(opt)
        scaler.update()
        assert all(torch.equal(p.detach(), a) for p, a in zip(ps, after)) and [float(opt.state[p]["step"]) for p in ps] == [1.0] * 4
        assert float(opt.last["nonfinite"]) == 1.0 and scaler.get_scale() == 2.0 ** 15
    assert _same(results[0], results[1])            # dividing by 2^16 is exact: with or without unscale_, the same bits


def test_max_grad_norm_is_settable_between_steps():
    ps = [torch.nn.Parameter(_values(90 + i, s, 0.02).cuda()) for i, s in enumerate([(300,), (4097,)])]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, qs):
        p.grad = _values(95, tuple(p.shape), 0.01).cuda()
        q.grad = p.grad.clone()
    opt, plain = FusedAdamW(ps, lr=1e-3), FusedAdamW(qs, lr=1e-3)
    opt.step(); plain.step()
    assert opt.last == {} and opt.grad_norms() == {}
    opt.max_grad_norm = math.inf                 # the table is built already: the buffers come with the first clipped step
    opt.step(); plain.step()
    assert float(opt.last["clip_coef"]) == 1.0 and float(opt.last["grad_norm"]) > 0.0 and _same([p.detach() for p in ps], [q.detach() for q in qs])
    opt.max_grad_norm = 1e-3
    opt.step(); plain.step()
    assert float(opt.last["clip_coef"]) < 1.0 and not torch.equal(ps[1].detach(), qs[1].detach())
    opt.max_grad_norm = None
    opt.step()
    assert opt.last == {} and [float(opt.state[p]["step"]) for p in ps] == [4.0, 4.0]
    sd = opt.state_dict()
    assert "max_grad_norm" not in repr(sd)
    topt = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-3, foreach=False)
    topt.load_state_dict(sd)                     # written by an optimizer that clipped: loads into torch's


# ---- with the model ---------------------------------------------------------------------------------------------------------

def test_tiny_model_trains_with_the_clip_on():
    sd = synth_torch_state(TINY, 3)
    x = torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda()
    y = torch.tensor([0, 2], device="cuda")
    model = _make_model(sd, "fp16")
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.01, max_grad_norm=math.inf)
    names = {p: n for n, p in model.named_parameters()}
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(x)[0], y).backward()
        grads = {p: p.grad.clone() for p in model.parameters() if p.grad is not None}
        total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values()))
        opt.max_grad_norm = 0.3 * total
        opt.step()
        assert all(torch.equal(p.grad, g) for p, g in grads.items())
        assert abs(float(opt.last["grad_norm"]) - total) <= _ulp(total) and float(opt.last["nonfinite"]) == 0.0
        coef = min(1.0, 0.3 * total / (total + 1e-6))
        assert abs(float(opt.last["clip_coef"]) - coef) <= _ulp(coef)
        norms = opt.grad_norms()
        assert set(norms) == set(model.parameters())
        for p in model.parameters():
            ref = float(torch.linalg.vector_norm(grads[p].double())) if p in grads else 0.0
            assert abs(float(norms[p]) - ref) <= _ulp(ref), (names[p], float(norms[p]), ref)
        assert all(float(opt.state[p]["step"]) == step + 1.0 for p in grads)
        # the packed 16-bit copies of the summary projections are gava_convert_h16 of the updated parameters
        fw, bw = model._packed, model._bwd_packs["vision"][1]
        bits = lambda t: t.view(torch.int16)
        trained = 0
        for i, blk in enumerate(model.visual.blocks):
            sa = blk.summary_attn_layer
            trained += sum(p in grads for p in sa.parameters())
            qkv = torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]).detach()
            out = sa.out_proj.weight.detach()
            assert torch.equal(bits(fw["w_sqkv"][i]), bits(hip.convert_h16(qkv, model.prec)))
            assert torch.equal(bits(fw["w_sout"][i]), bits(hip.convert_h16(out, model.prec)))
            assert torch.equal(fw["b_sqkv"][i], torch.cat([sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias]).detach())
            L = bw["layers"][i]
            qb, ob = bits(hip.convert_h16(qkv, hip.PREC_BF16)), bits(hip.convert_h16(out, hip.PREC_BF16))
            assert torch.equal(bits(L["w_sqkv"]), qb) and torch.equal(bits(L["w_sqkv_t"]), qb.t())
            assert torch.equal(bits(L["w_sout"]), ob) and torch.equal(bits(L["w_sout_t"]), ob.t())
        assert trained > 0
