"""GPU: the fused AdamW step (gava_adamw_step, gava_clip_amd.FusedAdamW) against the fp64 restatement tests/optim_ref.py.

Tolerance rule.  The kernel and torch.optim.AdamW(foreach=False) are two valid fp32 evaluation orders of the same formula and
neither is the reference, so the kernel is measured against torch's OWN error: for each of p, exp_avg and exp_avg_sq
    max |fused - ref|  <=  2 * max |torch fp32 on the same device - ref|  +  one fp32 ulp of the largest |ref|
with ref the fp64 restatement.  The maxima run over the whole tensor set and, in addition, over every single tensor of at least
1000 elements (the maximum over a handful of elements is a coin flip between two evaluation orders, over a thousand it is not).
The 16-bit copies are compared bit for bit with hip.convert_h16 of the updated parameter."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import FusedAdamW, VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402
from optim_ref import adamw_step  # noqa: E402

GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)]
SHAPES = [(1,), (7,), (196613,), (1030,), (128, 128), (80, 48), (33,)]      # (1030,) lives at storage offset 1, (33,) has no gradient
GROUP_OF = [0, 1, 0, 1, 0, 1, 1]
NO_GRAD = 6


def _values(seed, shape, scale):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).float()


def _grad(step, i):
    g = _values(1000 * step + i, SHAPES[i], 0.01)
    g.view(-1)[::7] = 0.0                                                          # exact zeros
    if i == 2:
        g[4099] = 1e4                                                              # one outlier
    return g


def _offset_one(t):
    """A device copy of `t` at storage offset 1: 4-byte alignment only."""
    base = torch.empty(t.numel() + 1, device="cuda")
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _param_set(misaligned=True):
    ps = []
    for i, s in enumerate(SHAPES):
        v = _values(i, s, 0.02)
        ps.append(torch.nn.Parameter(_offset_one(v) if (misaligned and i == 3) else v.cuda()))
    return ps


def _set_grads(ps, step, misaligned=True, scale=1.0):
    for i, p in enumerate(ps):
        if i == NO_GRAD:
            p.grad = None
            continue
        g = _grad(step, i) * scale
        p.grad = _offset_one(g) if (misaligned and i == 3) else g.cuda()


def _groups(ps):
    return [dict(params=[p for p, gi in zip(ps, GROUP_OF) if gi == k], **GROUPS[k]) for k in range(2)]


def _ref_steps(steps):
    ref = [_values(i, s, 0.02).double().numpy() for i, s in enumerate(SHAPES)]
    state = [{} for _ in SHAPES]
    for step in steps:
        grads = [None if i == NO_GRAD else _grad(step, i).double().numpy() for i in range(len(SHAPES))]
        adamw_step(ref, grads, state, GROUPS, GROUP_OF)
    return ref, state


def _check_rule(fused, torch_, ref, what):
    """fused / torch_ / ref: lists of arrays, one per tensor.  Prints every figure before it asserts."""
    ef = [np.abs(f.astype(np.float64) - r).max() for f, r in zip(fused, ref)]
    et = [np.abs(t.astype(np.float64) - r).max() for t, r in zip(torch_, ref)]
    big = [float(np.abs(r).max()) for r in ref]
    cases = [("set", max(ef), max(et), max(big))] + [(f"tensor {i} {r.shape}", ef[i], et[i], big[i]) for i, r in enumerate(ref) if r.size >= 1000]
    bad = []
    for name, f, t, b in cases:
        bound = 2.0 * t + float(np.spacing(np.float32(b)))
        print(f"{what} {name}: fused err {f:.3e}  torch err {t:.3e}  bound {bound:.3e}")
        if not f <= bound:
            bad.append((what, name, f, bound))
    assert not bad, bad


def _compare(fps, fopt, tps, topt, ref, state, skip=()):
    idx = [i for i in range(len(ref)) if state[i] and i not in skip]
    _check_rule([fps[i].detach().cpu().numpy() for i in idx], [tps[i].detach().cpu().numpy() for i in idx], [ref[i] for i in idx], "p")
    for key in ("exp_avg", "exp_avg_sq"):
        _check_rule([fopt.state[fps[i]][key].cpu().numpy() for i in idx], [topt.state[tps[i]][key].cpu().numpy() for i in idx],
                    [state[i][key] for i in idx], key)
    for i in idx:
        assert float(fopt.state[fps[i]]["step"]) == state[i]["step"] == float(topt.state[tps[i]]["step"])


def test_five_steps_on_plain_tensors_match_torch_within_its_own_error():
    fps, tps = _param_set(), _param_set(misaligned=False)
    fopt, topt = FusedAdamW(_groups(fps)), torch.optim.AdamW(_groups(tps), foreach=False)
    frozen = fps[NO_GRAD].detach().clone()
    assert fps[3].data_ptr() % 16 == 4
    for step in range(5):
        _set_grads(fps, step)
        _set_grads(tps, step, misaligned=False)
        ver = [p._version for p in fps]
        fopt.step()
        topt.step()
        assert [p._version > v for p, v in zip(fps, ver)] == [i != NO_GRAD for i in range(len(fps))]
    ref, state = _ref_steps(range(5))
    _compare(fps, fopt, tps, topt, ref, state)
    assert torch.equal(fps[NO_GRAD], frozen) and len(fopt.state[fps[NO_GRAD]]) == 0       # no gradient: bitwise unchanged, no state
    steps = [fopt.state[p]["step"] for i, p in enumerate(fps) if i != NO_GRAD]
    assert all(s.is_cuda and s.dtype == torch.float32 and s.untyped_storage().data_ptr() == steps[0].untyped_storage().data_ptr()
               for s in steps)                                                                # views of one device vector
    assert float(fopt._steps[fopt._index[id(fps[NO_GRAD])]]) == 0.0


def test_cosine_schedule_drives_it():
    fps, tps = _param_set(), _param_set(misaligned=False)
    fopt, topt = FusedAdamW(_groups(fps)), torch.optim.AdamW(_groups(tps), foreach=False)
    fs, ts = (torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=4) for o in (fopt, topt))
    ref = [_values(i, s, 0.02).double().numpy() for i, s in enumerate(SHAPES)]
    state = [{} for _ in SHAPES]
    for step in range(3):
        _set_grads(fps, step)
        _set_grads(tps, step, misaligned=False)
        groups = [dict(g, lr=topt.param_groups[k]["lr"]) for k, g in enumerate(GROUPS)]
        assert [g["lr"] for g in fopt.param_groups] == [g["lr"] for g in groups]
        adamw_step(ref, [None if i == NO_GRAD else _grad(step, i).double().numpy() for i in range(len(SHAPES))], state, groups, GROUP_OF)
        fopt.step(); topt.step(); fs.step(); ts.step()
    assert fopt.param_groups[0]["lr"] < 1e-3
    _compare(fps, fopt, tps, topt, ref, state)


# ---- the C ABI directly -------------------------------------------------------------------------------------------------

def _c_step(descs, groups, grad_scale=None, found_inf=None):
    lib = hip.load()
    tab = (hip.AdamWTensor * len(descs))(*descs)
    n = lib.gava_adamw_plan(tab, len(descs), len(groups), None, 0)
    assert n > 0
    chunks = (hip.AdamWChunk * n)()
    assert lib.gava_adamw_plan(tab, len(descs), len(groups), chunks, n) == n
    dev = torch.frombuffer(bytearray(bytes(tab) + bytes(chunks)), dtype=torch.uint8).cuda()
    a = hip.AdamWArgs()
    a.table, a.table_host, a.chunks = dev.data_ptr(), tab, dev.data_ptr() + C.sizeof(tab)
    a.n_tensors, a.n_chunks, a.n_groups = len(descs), n, len(groups)
    for k, g in enumerate(groups):
        a.groups[k].lr, a.groups[k].eps, a.groups[k].weight_decay = g["lr"], g["eps"], g["weight_decay"]
        a.groups[k].beta1, a.groups[k].beta2 = g["betas"]
    a.grad_scale, a.found_inf = hip.ptr(grad_scale), hip.ptr(found_inf)
    hip.check(lib.gava_adamw_step(C.byref(a), hip.stream_ptr()), "gava_adamw_step")
    torch.cuda.synchronize()


SENTINEL16, SENTINEL32 = 0x7A5C, 12345.0


class _Matrix:
    """One rows x cols parameter with all four copy targets, each a block of a wider sentinel-filled buffer."""

    def __init__(self, rows, cols, seed, prec, group, grad_scale=1.0):
        self.rows, self.cols, self.prec = rows, cols, prec
        self.p = _values(seed, (rows, cols), 0.02).cuda()
        self.g = (_values(seed + 1, (rows, cols), 0.01) * grad_scale).cuda()
        self.m = _values(seed + 2, (rows, cols), 0.01).cuda()
        self.v = (_values(seed + 3, (rows, cols), 0.01) ** 2 + 1e-6).cuda()
        self.step = torch.tensor([3.0], device="cuda")
        self.c16 = torch.full((rows, 3 * cols), SENTINEL16, dtype=torch.int16, device="cuda")       # q inside w_sqkv ...
        self.cbt = torch.full((cols, 3 * rows), SENTINEL16, dtype=torch.int16, device="cuda")       # ... and inside w_sqkv_t
        self.cb = torch.full((rows, cols), SENTINEL16, dtype=torch.int16, device="cuda")
        self.c32 = torch.full((rows, cols + 4), SENTINEL32, device="cuda")
        d = hip.AdamWTensor()
        d.p, d.g, d.m, d.v, d.step = (t.data_ptr() for t in (self.p, self.g, self.m, self.v, self.step))
        d.n, d.group, d.rows, d.cols, d.prec16 = rows * cols, group, rows, cols, prec
        d.copy16, d.ld16 = self.c16.data_ptr() + 2 * cols, 3 * cols
        d.copy_bf16_t, d.ld_bf16_t = self.cbt.data_ptr() + 2 * rows, 3 * rows
        d.copy_bf16, d.ld_bf16 = self.cb.data_ptr(), cols
        d.copy_f32, d.ld_f32 = self.c32.data_ptr(), cols + 4
        self.desc = d

    def tensors(self):
        return [self.p, self.m, self.v, self.step, self.c16, self.cbt, self.cb, self.c32]


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("prec", [hip.PREC_F16, hip.PREC_BF16])
def test_copies_are_bit_identical_to_convert_h16_of_the_updated_parameter(prec):
    mats = [_Matrix(128, 128, 10, prec, 0), _Matrix(80, 48, 20, prec, 1)]
    before = [mt.p.clone() for mt in mats]
    ref = [mt.p.double().cpu().numpy() for mt in mats]
    state = [dict(step=3.0, exp_avg=mt.m.double().cpu().numpy(), exp_avg_sq=mt.v.double().cpu().numpy()) for mt in mats]
    adamw_step(ref, [mt.g.double().cpu().numpy() for mt in mats], state, GROUPS, [0, 1])
    _c_step([mt.desc for mt in mats], GROUPS)
    for mt, p0, r, st in zip(mats, before, ref, state):
        R, Cn = mt.rows, mt.cols
        assert not torch.equal(mt.p, p0) and float(mt.step) == 4.0
        # one step from a random state: the update is at most ~1e-2 with a relative rounding of a few 2^-24, the parameter ~0.1
        for got, want in ((mt.p, r), (mt.m, st["exp_avg"]), (mt.v, st["exp_avg_sq"])):
            assert np.abs(got.double().cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()
        h, hb = hip.convert_h16(mt.p, prec), hip.convert_h16(mt.p, hip.PREC_BF16)
        assert torch.equal(mt.c16[:, Cn:2 * Cn], _bits(h))
        assert torch.equal(mt.cb, _bits(hb))
        assert torch.equal(mt.cbt[:, R:2 * R], _bits(hb).t())
        assert torch.equal(mt.c32[:, :Cn], mt.p)
        for wide, lo, hi in ((mt.c16, Cn, 2 * Cn), (mt.cbt, R, 2 * R)):                      # the neighbours inside the wider buffers
            assert bool((wide[:, :lo] == SENTINEL16).all()) and bool((wide[:, hi:] == SENTINEL16).all())
        assert bool((mt.c32[:, Cn:] == SENTINEL32).all())


def test_found_inf_changes_nothing():
    mats = [_Matrix(128, 128, 10, hip.PREC_F16, 0), _Matrix(80, 48, 20, hip.PREC_BF16, 1)]
    before = [[t.clone() for t in mt.tensors()] for mt in mats]
    _c_step([mt.desc for mt in mats], GROUPS, found_inf=torch.ones(1, device="cuda"))
    for mt, old in zip(mats, before):
        for t, o in zip(mt.tensors(), old):
            assert torch.equal(t, o)
    _c_step([mt.desc for mt in mats], GROUPS, found_inf=torch.zeros(1, device="cuda"))          # the same call with found_inf = 0 does step
    assert all(float(mt.step) == 4.0 and not torch.equal(mt.p, old[0]) for mt, old in zip(mats, before))


def test_power_of_two_grad_scale_is_exact():
    plain = [_Matrix(128, 128, 10, hip.PREC_F16, 0), _Matrix(80, 48, 20, hip.PREC_BF16, 1)]
    scaled = [_Matrix(128, 128, 10, hip.PREC_F16, 0, grad_scale=512.0), _Matrix(80, 48, 20, hip.PREC_BF16, 1, grad_scale=512.0)]
    _c_step([mt.desc for mt in plain], GROUPS)
    _c_step([mt.desc for mt in scaled], GROUPS, grad_scale=torch.full((1,), 512.0, device="cuda"), found_inf=torch.zeros(1, device="cuda"))
    for a, b in zip(plain, scaled):
        for t, u in zip(a.tensors(), b.tensors()):
            assert torch.equal(t, u)


def test_a_skipped_tensor_and_unaligned_pointers_through_the_abi():
    """g == NULL: no decay, no step increment, no copy.  A 1030-element tensor whose p and g sit 4 bytes past a 16-byte boundary
    takes the element-wise path and gets the same bits as an aligned one."""
    skip = _Matrix(80, 48, 30, hip.PREC_F16, 1)
    skip.desc.g = None
    vals = [_values(40 + k, (1030,), s) for k, s in enumerate((0.02, 0.01, 0.01, 0.01))]
    vals[3] = vals[3] ** 2
    al = [t.cuda() for t in vals]
    un = [_offset_one(t) for t in vals]
    descs = []
    steps = torch.zeros(2, device="cuda")
    for k, ts in enumerate((al, un)):
        d = hip.AdamWTensor()
        d.p, d.g, d.m, d.v = (t.data_ptr() for t in ts)
        d.step, d.n, d.group = steps.data_ptr() + 4 * k, 1030, 1
        descs.append(d)
    before = [t.clone() for t in skip.tensors()]
    _c_step([skip.desc] + descs, GROUPS)
    for t, o in zip(skip.tensors(), before):
        assert torch.equal(t, o)
    assert steps.tolist() == [1.0, 1.0]
    for k in (0, 2, 3):
        assert torch.equal(al[k], un[k]) and not torch.equal(al[k].cpu(), vals[k])


# ---- GradScaler -----------------------------------------------------------------------------------------------------------

def _scaled_backward(scaler, ps, w):
    for p in ps:
        p.grad = None
    scaler.scale(sum((p * q).sum() for p, q in zip(ps, w))).backward()


def test_grad_scaler_round_trip():
    ps = [torch.nn.Parameter(_values(50 + i, s, 0.02).cuda()) for i, s in enumerate([(300,), (40, 24), (1,)])]
    w = [_values(60 + i, tuple(p.shape), 0.01).cuda() for i, p in enumerate(ps)]
    opt = FusedAdamW(ps, lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    start = [p.detach().clone() for p in ps]
    _scaled_backward(scaler, ps, w)
    scaler.step(opt)
    scaler.update()
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    after = [p.detach().clone() for p in ps]
    assert all(not torch.equal(a, s) for a, s in zip(after, start)) and scaler.get_scale() == 2.0 ** 16
    assert [float(opt.state[p]["step"]) for p in ps] == [1.0, 1.0, 1.0]
    # the scale was divided out (exactly: it is a power of two): exp_avg = (1 - beta1) * the unscaled gradient, which is w
    for p, q in zip(ps, w):
        assert torch.allclose(opt.state[p]["exp_avg"], q * 0.1, rtol=1e-6, atol=0.0)
    state = [[opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq")] for p in ps]
    _scaled_backward(scaler, ps, w)
    ps[1].grad[3, 5] = float("inf")
    scaler.step(opt)                                                                     # skipped on the device
    scaler.update()
    for p, a, st in zip(ps, after, state):
        assert torch.equal(p.detach(), a) and float(opt.state[p]["step"]) == 1.0
        assert torch.equal(opt.state[p]["exp_avg"], st[0]) and torch.equal(opt.state[p]["exp_avg_sq"], st[1])
    assert scaler.get_scale() == 2.0 ** 15


def test_scaler_step_does_not_synchronise():
    ps = [torch.nn.Parameter(_values(70 + i, s, 0.02).cuda()) for i, s in enumerate([(300,), (40, 24)])]
    w = [_values(80 + i, tuple(p.shape), 0.01).cuda() for i, p in enumerate(ps)]
    opt = FusedAdamW(ps, lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    probe = torch.ones(1, device="cuda")
    held = []
    try:
        for it in range(3):
            held.append([p.grad for p in ps])           # keep the old gradients alive: the new ones get new addresses, so the
            _scaled_backward(scaler, ps, w)             # descriptor table is rebuilt and uploaded inside the guarded region
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            if it == 0:
                with pytest.raises(RuntimeError):
                    probe.item()                        # the mode is honoured: a deliberate sync raises
            scaler.step(opt)
            torch.cuda.set_sync_debug_mode("default")
            scaler.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0, 3.0]


# ---- checkpoint interchange -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_dict_interchange(direction):
    make = {"fused": lambda ps: FusedAdamW(_groups(ps)), "torch": lambda ps: torch.optim.AdamW(_groups(ps), foreach=False)}
    first, second = ("torch", "fused") if direction == "torch_to_fused" else ("fused", "torch")
    aps, bps = _param_set(misaligned=False), _param_set(misaligned=False)      # a: two steps of `first`, then one of `second`; b: torch throughout
    aopt, bopt = make[first](aps), make["torch"](bps)
    for step in range(2):
        _set_grads(aps, step, misaligned=False)
        _set_grads(bps, step, misaligned=False)
        aopt.step(); bopt.step()
    sd = aopt.state_dict()
    assert len(sd["state"]) == len(SHAPES) - 1 and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    copt = make[second](aps)
    copt.load_state_dict(sd)
    _set_grads(aps, 2, misaligned=False)
    _set_grads(bps, 2, misaligned=False)
    copt.step(); bopt.step()
    ref, state = _ref_steps(range(3))
    assert all(float(copt.state[p]["step"]) == 3.0 for i, p in enumerate(aps) if i != NO_GRAD)
    fused_opt = copt if second == "fused" else None
    idx = [i for i in range(len(ref)) if i != NO_GRAD]
    _check_rule([aps[i].detach().cpu().numpy() for i in idx], [bps[i].detach().cpu().numpy() for i in idx], [ref[i] for i in idx], "p")
    for key in ("exp_avg", "exp_avg_sq"):
        _check_rule([copt.state[aps[i]][key].cpu().numpy() for i in idx], [bopt.state[bps[i]][key].cpu().numpy() for i in idx],
                    [state[i][key] for i in idx], key)
    if first == "fused":                                                                  # the state_dict handed out copies, not views
        assert all(float(aopt.state[aps[i]]["step"]) == 2.0 for i in idx)
    if fused_opt is not None:                                                             # the loaded steps moved into the device vector
        s = [fused_opt.state[aps[i]]["step"] for i in idx]
        assert all(t.is_cuda and t.untyped_storage().data_ptr() == s[0].untyped_storage().data_ptr() for t in s)


# ---- with the model: the packed copies ----------------------------------------------------------------------------------------

def _make_model(state, dtype):
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
    m.load_state_dict(state, strict=True)
    m.set_operand_dtype(dtype)
    return m.cuda().train()


def _summary_copies(m):
    fw, bw = m._packed, m._bwd_packs["vision"][1]
    out = {}
    for i in range(len(m.visual.blocks)):
        for k in ("w_sqkv", "w_sout", "b_sqkv"):
            out[f"fw {k} {i}"] = fw[k][i]
        for k in ("w_sqkv", "w_sqkv_t", "w_sout", "w_sout_t"):
            out[f"bw {k} {i}"] = bw["layers"][i][k]
    return out


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp16+wlo"])
def test_model_step_refreshes_the_packed_copies(dtype):
    sd = synth_torch_state(TINY, 3)
    x = torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda()
    y = torch.tensor([0, 2], device="cuda")
    ce = torch.nn.functional.cross_entropy
    a, b = _make_model(sd, dtype), _make_model(sd, dtype)
    ce(a(x)[0], y).backward()                           # builds a's forward and backward packs
    for pa, pb in zip(a.parameters(), b.parameters()):  # the gradients are not run-to-run deterministic: both optimizers see these
        pb.grad = None if pa.grad is None else pa.grad.clone()
    fopt = FusedAdamW(a, lr=1e-3, weight_decay=0.01)
    topt = torch.optim.AdamW(b.parameters(), lr=1e-3, weight_decay=0.01, foreach=False)
    aps, bps = list(a.parameters()), list(b.parameters())
    trained = [i for i, p in enumerate(aps) if p.grad is not None]
    assert any("summary_attn_layer" in n for n, p in a.named_parameters() if p.grad is not None)
    ref = [aps[i].detach().double().cpu().numpy() for i in trained]
    state = [{} for _ in trained]
    adamw_step(ref, [aps[i].grad.double().cpu().numpy() for i in trained], state, [dict(GROUPS[1])], [0] * len(trained))
    key = a._pack_key()
    ptrs = {k: t.data_ptr() for k, t in _summary_copies(a).items()}
    fopt.step(); topt.step()
    assert a._pack_key() == key
    ver = a._summary_weight_versions()
    assert a._bwd_packs["vision"][1]["summary_ver"] == ver
    if "wlo" in dtype:
        assert a._packed["summary_ver"] != ver          # the weight-lo set is not written by the kernel: the host refresh still runs
    else:
        assert a._packed["summary_ver"] == ver
    _check_rule([aps[i].detach().cpu().numpy() for i in trained], [bps[i].detach().cpu().numpy() for i in trained], ref, "p")
    for k in ("exp_avg", "exp_avg_sq"):
        _check_rule([fopt.state[aps[i]][k].cpu().numpy() for i in trained], [topt.state[bps[i]][k].cpu().numpy() for i in trained],
                    [s[k] for s in state], k)
    fresh = _make_model({k: v.detach().clone() for k, v in a.state_dict().items()}, dtype)
    floss = ce(fresh(x)[0], y)
    floss.backward()
    mine, theirs = _summary_copies(a), _summary_copies(fresh)
    for k in mine:                                      # written in place by the kernel, before any forward could refresh them
        assert mine[k].data_ptr() == ptrs[k] and torch.equal(mine[k], theirs[k]), k
    loss = ce(a(x)[0], y)
    assert abs(float(loss.detach()) - float(floss.detach())) <= 1e-5 * abs(float(floss.detach()))
    if "wlo" in dtype:
        assert a._packed["summary_ver"] == ver
        for k in ("w_sqkv_wlo", "w_sout_wlo", "b_sqkv_wlo"):
            for t, u in zip(a._packed[k], fresh._packed[k]):
                assert torch.equal(t, u), k
