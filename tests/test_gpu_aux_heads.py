"""GPU: the auxiliary NTE and support-memory heads and their loss terms on the device (gava_nte_head*, gava_memory_head*,
gava_sigmoid_criterion*, gava_nte_diag_loss*, training.NteHeadFn / MemoryHeadFn, gava_clip_amd.AuxCriterion,
VitaCLIP.aux_heads = "hip").

Bounds (those of tests/test_gpu_train_head.py): every case is computed three ways - by the kernels, by torch fp32 ops on the GPU
(the model's "torch" route written out: the bmm over the 70 combinations, the loop over the classes) and in fp64 (tests/aux_ref.py,
a restatement in another form) - and values and gradients are judged against fp64.  The kernels pass when their error is at most
4 x the torch-fp32 route's (both are fp32 sums in different orders); they are never held below 1e-5 * max(1, max|ref|) for values
(largest element-wise error) or below 1e-6 norm-wise for gradients.  A gradient whose fp64 norm is below 1e-12 must come out below
1e-6.  Both routes' errors are printed per case ([aux-head-error] lines).

Model level: against the reference's own outputs and gradients (tests/golden/tiny_aux_grads.npz) with the bounds of
tests/test_gpu_backward.py::test_gradients_match_reference_with_auxiliary_heads, and the two routes against each other with 2e-2
norm-wise per parameter (the suite's bound for two routes of one computation)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import aux_ref  # noqa: E402
from gava_clip_amd import AuxCriterion, VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from gava_clip_amd.training import MemoryHeadFn, NteHeadFn  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402

MARGIN, VALUE_FLOOR, GRAD_FLOOR = 4.0, 1e-5, 1e-6
ROUTE_TOL = 2e-2
K_NTE = 70


def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def check_value(tag, name, new, old, ref):
    new, old, ref = _d(new), _d(old), _d(ref)
    assert new.shape == ref.shape, (tag, name)
    e_new, e_old = float((new - ref).abs().max()), float((old - ref).abs().max())
    print(f"\n[aux-head-error] {tag} {name}: kernels {e_new:.3e} torch-fp32 {e_old:.3e} (max abs, max|ref| {float(ref.abs().max()):.3e})")
    assert e_new <= max(MARGIN * e_old, VALUE_FLOOR * max(1.0, float(ref.abs().max()))), (tag, name, e_new, e_old)


def check_grad(tag, name, new, old, ref):
    new, old, ref = _d(new), _d(old), _d(ref)
    assert new.shape == ref.shape, (tag, name)
    if float(ref.norm()) < 1e-12:
        print(f"\n[aux-head-error] {tag} {name}: fp64 norm {float(ref.norm()):.1e}, kernels' norm {float(new.norm()):.3e}")
        assert float(new.norm()) < 1e-6, (tag, name, float(new.norm()))
        return
    e_new, e_old = float((new - ref).norm() / ref.norm()), float((old - ref).norm() / ref.norm())
    print(f"\n[aux-head-error] {tag} {name}: kernels {e_new:.3e} torch-fp32 {e_old:.3e} (norm-wise)")
    assert e_new <= max(MARGIN * e_old, GRAD_FLOOR), (tag, name, e_new, e_old)


# ---- 1. NTE head op ------------------------------------------------------------------------------------------------------------

def invalid_clip(E, gen):
    """[70, E] integer-valued rows in triples 2a, -a, -a (22 of them) plus one 3a, -a, -a, -a, a in [-8, 8]^E: the element sum is
    exactly zero in any summation order, every row has a norm, and the mean unit row (-a / |a| per triple) is not zero."""
    rows = []
    for t in range(23):
        a = torch.randint(-8, 9, (E,), generator=gen).float()
        a[0] = a[0] if a[0] != 0 else 1.0
        rows += [2 * a, -a, -a] if t < 22 else [3 * a, -a, -a, -a]
    return torch.stack(rows)


NTE_CASES = [(1, 128, 128, None), (2, 128, 128, None), (5, 128, 128, 3), (17, 128, 128, None), (65, 768, 512, 40), (3, 1024, 768, None)]
SCALES = [100.0, math.log(10.0)]


def nte_inputs(B, D, E, bad, scale):
    g = torch.Generator().manual_seed(B * 31 + D + E)
    nte = torch.randn(B, K_NTE, E, generator=g)
    if bad is not None:
        nte[bad] = invalid_clip(E, g)
        assert float(nte[bad].sum()) == 0.0 and float(nte[bad].flip(0).t().contiguous().sum()) == 0.0
    return dict(summary=torch.randn(B, D, generator=g), weight=(torch.rand(E, D, generator=g) * 2 - 1) / math.sqrt(D),
                bias=(torch.rand(E, generator=g) * 2 - 1) / math.sqrt(D), scale=torch.tensor(scale), nte=nte,
                w=torch.randn(B, B, generator=g))


def nte_torch(summary, weight, bias, video_nte, scale):
    """The model's torch route (VitaCLIP._forward_impl), op for op."""
    sp = F.linear(summary, weight, bias)
    sp = sp / sp.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        valid_idx = ((video_nte.sum(dim=-1).sum(dim=-1)) != 0).float()
        valid_mat = valid_idx.unsqueeze(1) * valid_idx.unsqueeze(0)
    video_nte = video_nte / video_nte.norm(dim=-1, keepdim=True)
    similarity = torch.bmm(sp.unsqueeze(0).expand(K_NTE, -1, -1), video_nte.permute(1, 2, 0)).mean(0)
    logits_mat = scale * (similarity * valid_mat)
    return F.log_softmax(logits_mat, dim=-1) + F.log_softmax(logits_mat, dim=-2)


def nte_route(d, fn, dtype, device):
    leaves = {k: d[k].to(device=device, dtype=dtype).requires_grad_() for k in ("summary", "weight", "bias", "scale")}
    out = fn(leaves["summary"], leaves["weight"], leaves["bias"], d["nte"].to(device=device, dtype=dtype), leaves["scale"])
    (out * d["w"].to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items()}


_REFS = {}


def cached(key, make):
    """fp64 references are computed once per case and shared between the tests that need them."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


@pytest.mark.parametrize("scale", SCALES, ids=["scale100", "scale_log10"])
@pytest.mark.parametrize("B,D,E,bad", NTE_CASES, ids=[f"B{b}_D{d}_E{e}" + ("" if x is None else f"_invalid{x}") for b, d, e, x in NTE_CASES])
def test_nte_head_matches_fp64(B, D, E, bad, scale):
    tag = f"nte B{B} D{D} E{E} scale{scale:.3g}"
    d = cached(("nte_in", B, D, E, bad, scale), lambda: nte_inputs(B, D, E, bad, scale))
    ref, ref_g = cached(("nte", B, D, E, bad, scale), lambda: nte_route(d, aux_ref.nte_head, torch.float64, "cpu"))
    got, got_g = nte_route(d, NteHeadFn.apply, torch.float32, "cuda")
    old, old_g = nte_route(d, nte_torch, torch.float32, "cuda")
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all())
    if bad is not None and B > 1:                    # the test's precondition: the mask matters for this input (2.6 at scale 100,
        # 0.05 at log 10 - against a value floor of 1e-4)
        unmasked = dict(d, nte=d["nte"].clone())
        unmasked["nte"][bad, 0, 0] += 1.0
        assert float((nte_route(unmasked, aux_ref.nte_head, torch.float64, "cpu")[0] - ref).abs().max()) > 0.01
    if B == 1:
        assert float(got.abs().max()) == 0.0
    check_value(tag, "logits_vm", got, old, ref)
    for name in got_g:
        check_grad(tag, "d" + name, got_g[name], old_g[name], ref_g[name])


# ---- 2. support-memory head op -------------------------------------------------------------------------------------------------

MEM_CASES = [(1, 1, 1, 128), (2, 5, 3, 128), (7, 3, 4, 128), (65, 2, 3, 512), (3, 1, 65, 128), (4, 2, 3, 768)]
PAR = ("w1", "b1", "w2", "b2")


def mem_inputs(M, S, C, E):
    g = torch.Generator().manual_seed(M * 131 + S * 17 + C * 5 + E)
    H1, H2 = E // 4, E // 8
    u = lambda *s, fan: (torch.rand(*s, generator=g) * 2 - 1) / math.sqrt(fan)
    tf = torch.randn(C, E, generator=g)
    d = dict(memory=torch.randn(M, S, E, generator=g), tf=tf / tf.norm(dim=-1, keepdim=True),
             tf_w1=u(H1, E, fan=E), tf_b1=u(H1, fan=E), tf_w2=u(H2, H1, fan=H1), tf_b2=u(H2, fan=H1),
             mem_w1=u(C, H1, E, fan=E), mem_b1=u(C, H1, fan=E), mem_w2=u(C, H2, H1, fan=H1), mem_b2=u(C, H2, fan=H1),
             w=torch.randn(M, C, generator=g))
    return d


def mem_torch(memory, tf, tf_params, per_class, scale, bias):
    """The model's torch route, op for op (the loop over the classes)."""
    tf_project = lambda x: F.linear(torch.tanh(F.linear(x, tf_params[0], tf_params[1])), tf_params[2], tf_params[3])
    memory = memory.mean(dim=1)
    logits_mt = torch.empty(memory.size(0), 0).to(memory.device)
    for cid, (w1, b1, w2, b2) in enumerate(per_class):
        t = tf_project(tf[cid])
        t = t / t.norm(dim=-1, keepdim=True)
        memo = F.linear(torch.tanh(F.linear(memory, w1, b1)), w2, b2)
        memo = memo / memo.norm(dim=-1, keepdim=True)
        logits_mt = torch.concat([logits_mt, (scale * memo @ t.t()).unsqueeze(-1)], dim=1)
    logits_mt = F.log_softmax(logits_mt, dim=-1)
    if bias is not None:
        logits_mt = logits_mt + bias
    return logits_mt


def mem_route(d, kind, dtype, device, bias, with_tf):
    """kind: "ref" (stacked parameters, one batched product), "torch" (the loop) or "hip" (MemoryHeadFn).  -> outputs and the
    gradients, memory_project's stacked over the classes."""
    C = d["tf"].shape[0]
    to = lambda t: t.to(device=device, dtype=dtype)
    leaves = {k: to(d[k]).requires_grad_() for k in ("tf_w1", "tf_b1", "tf_w2", "tf_b2")}
    leaves["scale"] = to(torch.tensor(100.0 if bias is None else math.log(10.0))).requires_grad_()
    if bias is not None:
        leaves["bias"] = to(torch.tensor(bias)).requires_grad_()
    tf = to(d["tf"])
    if with_tf:
        leaves["tf"] = tf = tf.requires_grad_()
    tf_params = [leaves[k] for k in ("tf_w1", "tf_b1", "tf_w2", "tf_b2")]
    if kind == "ref":
        stacked = [to(d["mem_" + k]).requires_grad_() for k in PAR]
        out = aux_ref.memory_head(to(d["memory"]), tf, tf_params, stacked, leaves["scale"], leaves.get("bias"))
    else:
        per_class = [[to(d["mem_" + k][c]).clone().requires_grad_() for k in PAR] for c in range(C)]
        if kind == "torch":
            out = mem_torch(to(d["memory"]), tf, tf_params, per_class, leaves["scale"], leaves.get("bias"))
        else:
            flat = [q for cls in per_class for q in cls]
            table = hip.pointer_table(flat, device)
            out = MemoryHeadFn.apply(to(d["memory"]), tf, leaves["scale"], leaves.get("bias"), table, *tf_params, *flat)
    (out * to(d["w"])).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    for i, k in enumerate(PAR):
        grads["mem_" + k] = stacked[i].grad if kind == "ref" else torch.stack([per_class[c][i].grad for c in range(C)])
    return out.detach(), grads


@pytest.mark.parametrize("bias,with_tf", [(None, True), (-10.0, True), (None, False), (-10.0, False)],
                         ids=["nobias_dtf", "bias_dtf", "nobias_nodtf", "bias_nodtf"])
@pytest.mark.parametrize("M,S,C,E", MEM_CASES, ids=[f"M{m}_S{s}_C{c}_E{e}" for m, s, c, e in MEM_CASES])
def test_memory_head_matches_fp64(M, S, C, E, bias, with_tf):
    tag = f"mem M{M} S{S} C{C} E{E} bias{bias} dtf{int(with_tf)}"
    d = cached(("mem_in", M, S, C, E), lambda: mem_inputs(M, S, C, E))
    ref, ref_g = cached(("mem", M, S, C, E, bias, with_tf), lambda: mem_route(d, "ref", torch.float64, "cpu", bias, with_tf))
    got, got_g = mem_route(d, "hip", torch.float32, "cuda", bias, with_tf)
    old, old_g = mem_route(d, "torch", torch.float32, "cuda", bias, with_tf)
    assert set(got_g) == set(ref_g) and ("tf" in got_g) == with_tf
    if C == 1:
        assert float((got - (bias or 0.0)).abs().max()) == 0.0
    check_value(tag, "logits_mt", got, old, ref)
    for name in got_g:
        assert got_g[name] is not None, name
        check_grad(tag, "d" + name, got_g[name], old_g[name], ref_g[name])


# ---- 3. loss terms --------------------------------------------------------------------------------------------------------------

def _golden_sets():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aux_loss_ref.npz"))
    out = []
    for s in range(int(gold["n_sets"])):
        focal, alpha, gamma, scale = [float(v) for v in gold[f"params_{s}"]]
        out.append((f"golden{s}", gold[f"logits_{s}"].astype(np.float32), gold[f"labels_{s}"],
                    dict(use_focal=bool(focal), alpha=alpha, gamma=gamma, scale=scale)))
    return out


SIGMOID_SETS = _golden_sets()


def sigmoid_torch(x, y, *, use_focal, alpha, gamma, scale):
    """The loss as a training loop writes it in torch ops (fp32 on the GPU), per sample."""
    t = F.one_hot(y, num_classes=x.shape[-1]).float()
    ce = -F.logsigmoid((t * 2 - 1.0) * x)
    if use_focal:
        p = torch.sigmoid(x)
        p_t = p * t + (1.0 - p) * (1.0 - t)
        ce = (alpha * t + (1.0 - alpha) * (1.0 - t)) * (1.0 - p_t) ** gamma * ce
    return ce.sum(-1) * scale


@pytest.mark.parametrize("tag,z,y,kw", SIGMOID_SETS, ids=[s[0] for s in SIGMOID_SETS])
def test_sigmoid_criterion_matches_fp64(tag, z, y, kw):
    ref = aux_ref.sigmoid_loss(z, y, **kw)                       # fp64 on the fp32 logits the kernel reads
    logits, labels = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    padded = torch.zeros(z.shape[0], z.shape[1] + 3, device="cuda")
    padded[:, :z.shape[1]] = logits
    out = hip.sigmoid_criterion(logits, labels, **kw)
    out_p = hip.sigmoid_criterion(padded[:, :z.shape[1]], labels, **kw)          # a row stride of its own
    assert torch.equal(out["per_sample"], out_p["per_sample"]) and torch.equal(out["loss"], out_p["loss"])
    lt = logits.clone().requires_grad_()
    per_t = sigmoid_torch(lt, labels, **kw)
    per_t.mean().backward()
    check_value(tag, "per_sample", out["per_sample"], per_t, ref["per_sample"])
    check_value(tag, "loss", out["loss"], per_t.mean(), ref["loss"])
    d1 = hip.sigmoid_criterion_backward(logits, out["labels"], torch.ones((), device="cuda"), **kw)
    d8 = hip.sigmoid_criterion_backward(padded[:, :z.shape[1]], out["labels"], torch.full((), 0.125, device="cuda"), **kw)
    assert torch.equal(d8, d1 * 0.125)
    check_grad(tag, "dlogits", d1, lt.grad, ref["dlogits"])


def test_sigmoid_criterion_refuses_small_gamma():
    logits, labels = torch.randn(4, 3, device="cuda"), torch.tensor([0, 1, 2, 1], device="cuda")
    with pytest.raises(hip.GavaError, match="GAVA_EINVAL"):
        hip.sigmoid_criterion(logits, labels, use_focal=True, gamma=0.5)
    with pytest.raises(hip.GavaError, match="soft"):
        hip.sigmoid_criterion(logits, torch.softmax(logits, -1))


@pytest.mark.parametrize("B", [1, 5, 65])
def test_nte_diag_loss_matches_fp64(B):
    g = torch.Generator().manual_seed(B)
    lv = torch.randn(B, B, generator=g) * 3 - 4
    crit = AuxCriterion(vnte_loss_weight=0.7)
    lt = lv.cuda().requires_grad_()
    mid = lt * 1.0                                   # a non-leaf input, as a model's logits are
    _, loss = crit(logits_vm=mid)
    (loss * 0.5).backward()
    l64 = lv.double().requires_grad_()
    ref = aux_ref.nte_diag(l64, 0.7)
    (ref * 0.5).backward()
    l32 = lv.cuda().requires_grad_()
    old = -0.7 * torch.diag(l32).mean()
    (old * 0.5).backward()
    check_value(f"nte_diag B{B}", "loss", loss, old, ref)
    check_grad(f"nte_diag B{B}", "dlogits_vm", lt.grad, l32.grad, l64.grad)
    assert int((lt.grad != 0).sum()) == B


@pytest.mark.parametrize("sigmoid", [False, True], ids=["ce", "sigmoid"])
def test_aux_criterion_under_autograd_and_gradscaler(sigmoid):
    z = torch.randn(7, 3, generator=torch.Generator().manual_seed(11)) * 2
    y = torch.tensor([0, 2, 1, 1, 0, 2, 2])
    w = 0.6
    crit = AuxCriterion(memory_loss_weight=w, sigmoid=sigmoid)
    lt = z.cuda().requires_grad_()
    loss, none = crit(logits_mt=lt * 1.0, mt_labels=y.cuda())
    assert none is None and loss.dim() == 0 and loss.is_cuda
    torch.amp.GradScaler("cuda", init_scale=512.0).scale(loss / 2).backward()
    z64 = z.double().requires_grad_()
    if sigmoid:                                      # the reference's double weighting: scale = w inside, times w outside
        ref = (w * aux_ref_sigmoid_torch64(z64, y, w)).mean()
    else:
        ref = (w * F.cross_entropy(z64, y, reduction="none")).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert float((lt.grad.cpu().double() / 256.0 - z64.grad).norm() / z64.grad.norm()) <= 1e-5


def aux_ref_sigmoid_torch64(x, y, scale):
    t = F.one_hot(y, num_classes=x.shape[-1]).double()
    return (-F.logsigmoid((t * 2 - 1.0) * x)).sum(-1) * scale


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------

def test_same_bits_on_every_run():
    B, D, E, bad = NTE_CASES[3]
    d = cached(("nte_in", B, D, E, bad, 100.0), lambda: nte_inputs(B, D, E, bad, 100.0))
    a, b = (nte_route(d, NteHeadFn.apply, torch.float32, "cuda") for _ in range(2))
    assert torch.equal(a[0], b[0])
    for name in a[1]:
        assert torch.equal(a[1][name], b[1][name]), name
    M, S, C, E = MEM_CASES[2]
    d = cached(("mem_in", M, S, C, E), lambda: mem_inputs(M, S, C, E))
    a, b = (mem_route(d, "hip", torch.float32, "cuda", -10.0, True) for _ in range(2))
    assert torch.equal(a[0], b[0])
    for name in a[1]:
        assert torch.equal(a[1][name], b[1][name]), name
    tag, z, y, kw = SIGMOID_SETS[1]
    logits, labels = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    runs = []
    for _ in range(2):
        out = hip.sigmoid_criterion(logits, labels, **kw)
        runs.append((out["loss"], out["per_sample"], hip.sigmoid_criterion_backward(logits, out["labels"], torch.full((), 0.5, device="cuda"), **kw)))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    lv = torch.randn(65, 65, generator=torch.Generator().manual_seed(1)).cuda()
    g = torch.full((), 0.25, device="cuda")
    assert torch.equal(hip.nte_diag_loss(lv, 0.7), hip.nte_diag_loss(lv, 0.7))
    assert torch.equal(hip.nte_diag_loss_backward(65, g, 0.7), hip.nte_diag_loss_backward(65, g, 0.7))


def test_heads_give_the_same_bits_with_and_without_grad():
    """The heads' forward kernels do not depend on whether autograd records them: the same inputs under torch.no_grad() and with
    grad give torch.equal outputs (at model level the towers in front of them run other kernels without grad, so this is pinned here)."""
    B, D, E, bad = NTE_CASES[2]
    d = cached(("nte_in", B, D, E, bad, 100.0), lambda: nte_inputs(B, D, E, bad, 100.0))
    args = [d[k].cuda() for k in ("summary", "weight", "bias", "nte", "scale")]
    with torch.no_grad():
        plain = NteHeadFn.apply(*args)
    live = NteHeadFn.apply(*[a.clone().requires_grad_() if i != 3 else a for i, a in enumerate(args)])
    assert not plain.requires_grad and live.requires_grad and torch.equal(plain, live.detach())
    M, S, C, E = MEM_CASES[2]
    d = cached(("mem_in", M, S, C, E), lambda: mem_inputs(M, S, C, E))
    flat = [d["mem_" + k][c].cuda().clone() for c in range(C) for k in PAR]
    tf_params = [d[k].cuda() for k in ("tf_w1", "tf_b1", "tf_w2", "tf_b2")]
    table = hip.pointer_table(flat, "cuda")
    scale, bias = torch.tensor(100.0, device="cuda"), torch.tensor(-10.0, device="cuda")
    with torch.no_grad():
        plain = MemoryHeadFn.apply(d["memory"].cuda(), d["tf"].cuda(), scale, bias, table, *tf_params, *flat)
    live = MemoryHeadFn.apply(d["memory"].cuda(), d["tf"].cuda().requires_grad_(), scale.clone().requires_grad_(), bias, table,
                              *[q.requires_grad_() for q in tf_params], *[q.requires_grad_() for q in flat])
    assert not plain.requires_grad and live.requires_grad and torch.equal(plain, live.detach())
    # a class count that differs between text_features and memory_project's table is refused with a message
    with pytest.raises(hip.GavaError, match="classes"):
        hip.memory_head(d["memory"].cuda(), d["tf"].cuda()[:C - 1], tf_params, table, scale)
    with pytest.raises(hip.GavaError, match="do not fit"):
        hip.nte_head(args[0], args[1], args[2], args[3][:, :, :E - 4], args[4])


# ---- 5. model level -------------------------------------------------------------------------------------------------------------

def _graph_has(fn, name):
    seen, stack = set(), [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if name in type(f).__name__:
            return True
        stack.extend(n for n, _ in f.next_functions)
    return False


def _tiny(**ctor):
    def make():
        kw = dict(add_nte=True, use_support_memory=True, detach_features=False, num_classes=3)
        kw.update(ctor)
        m = VitaCLIP(**model_kwargs(TINY, CLASSES_3), **kw)
        sd = synth_torch_state(TINY, 3)
        sd.update({k: torch.from_numpy(v) for k, v in synth.synth_aux_state(TINY, 3).items()})
        if kw.get("use_sigmoid_loss"):
            sd.update(logit_bias=torch.tensor(-10.0), logit_bias_mt=torch.tensor(-10.0), logit_scale=torch.tensor(math.log(math.log(10.0))))
        m.load_state_dict(sd, strict=True)
        return m.cuda().train()
    return make


@pytest.fixture(scope="module")
def clip():
    return torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda()


def _aux(n_mem=2):
    nte, _ = synth.synth_aux_inputs(2, TINY.embed_dim)
    _, mem = synth.synth_aux_inputs(n_mem, TINY.embed_dim)
    return dict(memory=torch.from_numpy(mem).cuda(), video_nte=torch.from_numpy(nte).cuda())


@pytest.mark.parametrize("train_head", ["torch", "hip"])
def test_gradients_match_reference_with_hip_auxiliary_heads(golden_dir, clip, train_head):
    """tests/test_gpu_backward.py::test_gradients_match_reference_with_auxiliary_heads with aux_heads = "hip": the reference
    model's outputs (2e-3 of the largest entry) and every gradient (4e-2 norm-wise)."""
    from test_gpu_backward import _check_against_reference_grads
    gold = np.load(os.path.join(golden_dir, "tiny_aux_grads.npz"))
    m = _tiny()()
    m.aux_heads, m.train_head = "hip", train_head
    logits, lmt, lvm = m(clip, **_aux())
    for got, key in ((logits, "logits"), (lvm, "logits_vm"), (lmt, "logits_mt")):
        ref = torch.from_numpy(gold[key])
        assert (got.detach().cpu() - ref).abs().max() <= 2e-3 * ref.abs().max(), key
    loss = (logits * torch.from_numpy(gold["w_logits"]).cuda()).sum() + (lvm * torch.from_numpy(gold["w_vm"]).cuda()).sum() \
        + (lmt * torch.from_numpy(gold["w_mt"]).cuda()).sum()
    assert _graph_has(loss.grad_fn, "NteHeadFn") and _graph_has(loss.grad_fn, "MemoryHeadFn")
    loss.backward()
    _check_against_reference_grads(m, gold)


def _torch_aux_terms(lmt, y_mt, lvm, sigmoid, w_mt, w_vm):
    """loss_mt and loss_vm of training/train.py:454-475 in torch ops."""
    if sigmoid:
        loss_mt = (w_mt * sigmoid_torch(lmt, y_mt, use_focal=False, alpha=0.25, gamma=2.0, scale=w_mt)).mean()
    else:
        loss_mt = (w_mt * F.cross_entropy(lmt, y_mt, reduction="none")).mean()
    return loss_mt, -w_vm * torch.diag(lvm).mean()


def _both_routes(make, run, y, y_mt, sigmoid, scale=None, train_head="torch"):
    res = {}
    for route in ("hip", "torch"):
        m = make()
        m.aux_heads, m.train_head = route, train_head
        logits, lmt, lvm = run(m)
        loss = F.cross_entropy(logits, y)
        if route == "hip":
            loss_mt, loss_vm = AuxCriterion(memory_loss_weight=0.8, vnte_loss_weight=0.5, sigmoid=sigmoid)(lmt, y_mt, lvm)
        else:
            loss_mt, loss_vm = _torch_aux_terms(lmt, y_mt, lvm, sigmoid, 0.8, 0.5)
        tot = loss + loss_mt + loss_vm
        assert (_graph_has(tot.grad_fn, "NteHeadFn") and _graph_has(tot.grad_fn, "MemoryHeadFn")) == (route == "hip")
        if scale is not None:
            torch.amp.GradScaler("cuda", init_scale=scale).scale(tot).backward()
        else:
            tot.backward()
        res[route] = ((lmt.detach(), lvm.detach(), loss_mt.detach(), loss_vm.detach()), {n: p.grad for n, p in m.named_parameters()})
    (oh, gh), (ot, gt) = res["hip"], res["torch"]
    for a, b in zip(oh, ot):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))
    n = 0
    for name, g_ref in gt.items():
        if g_ref is None:
            assert gh[name] is None, name
            continue
        assert gh[name] is not None and bool(torch.isfinite(gh[name]).all()), name
        if float(g_ref.norm()) < 1e-12:
            assert float(gh[name].norm()) < 1e-6 * (scale or 1.0), name
            continue
        n += 1
        r = float((gh[name] - g_ref).norm() / g_ref.norm())
        assert r <= ROUTE_TOL, (name, r)
    assert n > 20 and all(gh[k] is not None for k in ("sum_proj.weight", "tf_project.0.weight", "memory_project.2.2.bias", "logit_scale_vm"))
    return res


LABELS = dict(y=[2, 0], y_mt=[1, 2])


@pytest.mark.parametrize("detach", [False, True], ids=["attached", "detach_features"])
@pytest.mark.parametrize("sigmoid", [False, True], ids=["ce", "sigmoid"])
def test_model_hip_aux_heads_equal_torch_aux_heads(clip, sigmoid, detach):
    y, y_mt = (torch.tensor(v, device="cuda") for v in LABELS.values())
    aux = _aux()
    _both_routes(_tiny(detach_features=detach), lambda m: m(clip, **aux), y, y_mt, sigmoid)


def test_model_hip_aux_heads_with_logit_bias_mt(clip):
    """use_sigmoid_loss=True gives the memory head its logit_bias_mt.  The torch route adds it in place to log_softmax's output
    (as the reference does), which torch's autograd refuses in the backward, so the routes are compared without grad; under
    autograd the new route returns every gradient - logit_bias_mt's is the sum of d logits_mt, which the sigmoid criterion makes
    (scale / M) * sum of -t sigmoid(-t x): compared with that sum in torch ops to the op tests' floor."""
    aux = _aux()
    y, y_mt = (torch.tensor(v, device="cuda") for v in LABELS.values())
    m = _tiny(use_sigmoid_loss=True)()
    with torch.no_grad():
        _, lmt_t, lvm_t = m(clip, **aux)
        m.aux_heads = "hip"
        _, lmt_h, lvm_h = m(clip, **aux)
    assert float((lmt_h - lmt_t).abs().max()) <= 1e-5 * float(lmt_t.abs().max())
    assert float((lvm_h - lvm_t).abs().max()) <= 1e-5 * max(1.0, float(lvm_t.abs().max()))
    logits, lmt, lvm = m(clip, **aux)
    loss_mt, loss_vm = AuxCriterion(memory_loss_weight=0.8, sigmoid=True)(lmt, y_mt, lvm)
    (F.cross_entropy(logits, y) + loss_mt + loss_vm).backward()
    x = lmt.detach().double()
    t = F.one_hot(y_mt, 3).double() * 2 - 1
    want = float((-t * torch.sigmoid(-t * x)).sum() * 0.8 * 0.8 / x.shape[0])
    assert abs(float(m.logit_bias_mt.grad) - want) <= 1e-5 * max(1.0, abs(want))
    for name, p in m.named_parameters():
        if name.startswith(("sum_proj", "tf_project", "memory_project", "logit_scale_vm", "logit_scale_mt", "logit_bias_mt")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_model_hip_aux_heads_under_gradscaler_with_the_hip_head(clip):
    y, y_mt = (torch.tensor(v, device="cuda") for v in LABELS.values())
    aux = _aux()
    _both_routes(_tiny(), lambda m: m(clip, **aux), y, y_mt, False, scale=1024.0, train_head="hip")


def test_model_hip_aux_heads_with_three_memories_beside_two_clips(clip):
    y, y_mt = torch.tensor([2, 0], device="cuda"), torch.tensor([1, 2, 0], device="cuda")
    aux = _aux(n_mem=3)
    res = _both_routes(_tiny(), lambda m: m(clip, **aux), y, y_mt, True)
    assert res["hip"][0][0].shape == (3, 3)


def test_model_hip_aux_heads_through_forward_frames():
    import train_preprocess_ref as ref
    from gava_clip_amd.preprocess import ClipPreprocessor
    pre = ClipPreprocessor(num_frames=TINY.num_frames, sampling_rate=2, spatial_size=TINY.input_size)
    vids = [ref.video(11, 90, 130, 500).cuda(), ref.video(6, 120, 80, 501).cuda()]
    y, y_mt = (torch.tensor(v, device="cuda") for v in LABELS.values())
    aux = _aux()
    _both_routes(_tiny(), lambda m: m.forward_frames(vids, pre, **aux), y, y_mt, False)


def test_model_hip_aux_heads_without_grad_and_without_inputs(clip):
    aux = _aux()
    m = _tiny()()
    m.aux_heads = "hip"
    _, lmt, lvm = m(clip, **aux)
    with torch.no_grad():
        _, lmt0, lvm0 = m(clip, **aux)
        assert not lmt0.requires_grad and not lvm0.requires_grad
        # the towers run their inference kernels without grad and their training kernels with it: two routes of the same fp16
        # forward, held to the bound the golden test above holds either of them to (2e-3 of the largest entry)
        near = lambda a, b: float((a - b).abs().max()) <= 2e-3 * float(b.abs().max())
        assert near(lmt0, lmt.detach()) and near(lvm0, lvm.detach())
        m.eval()
        _, lmt1, lvm1 = m(clip, **aux)
        assert near(lmt1, lmt0) and near(lvm1, lvm0)
        assert m(clip)[1:] == (None, None)
        assert m(clip, memory=aux["memory"])[2] is None and m(clip, video_nte=aux["video_nte"])[1] is None
        half = m(clip, memory=aux["memory"].double()[:, :, :], video_nte=aux["video_nte"].half())      # converted, not refused
        assert half[1].dtype == torch.float32 and float((half[1] - lmt1).abs().max()) <= 1e-5
        with pytest.raises(hip.GavaError, match="HIP device"):
            m(clip, memory=aux["memory"].cpu())
        with pytest.raises(hip.GavaError, match="HIP device"):
            m(clip, video_nte=aux["video_nte"].cpu())
    t = _tiny()()
    assert t.aux_heads == "torch"
    out = t(clip, **aux)
    assert not _graph_has(out[1].grad_fn, "MemoryHeadFn") and not _graph_has(out[2].grad_fn, "NteHeadFn")
