"""GPU: the training head and criterion on the device (gava_train_criterion*, gava_train_head*, training.HeadFn,
gava_clip_amd.TrainCriterion, VitaCLIP.train_head = "hip").

Values (loss, per_sample, weight, logits, text_features) against fp64: rtol 1e-5 / atol 1e-5, the bound of the similarity-head and
view-score tests.  top1, hits, conf: exact.

Gradient bound: every gradient is computed twice per case - by the new kernels and by torch fp32 ops on the GPU (what the step
did before) - and both are judged norm-wise against fp64.  The kernels pass when their error is at most 4 x the torch route's
(both are fp32 sums in different orders) and in no case are they held below 1e-6 (the tightest bound of this kind in the suite;
it keeps a lucky torch result from failing a correct kernel).  The errors of both routes are printed per case
([train-head-error] lines).

Model level: the two routes of the same computation must agree as tests/test_gpu_backward.py asks of two routes (2e-2 norm-wise
per parameter: its batch-additivity test; the DDP test uses the same figure)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import TrainCriterion, VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from gava_clip_amd.training import HeadFn  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402
from loss_ref import criterion as criterion_ref  # noqa: E402

GRAD_MARGIN, GRAD_FLOOR = 4.0, 1e-6
ROUTE_TOL = 2e-2          # tests/test_gpu_backward.py: two routes of the same computation, norm-wise per parameter


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def close(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return bool(((got - ref).abs() <= 1e-5 + 1e-5 * ref.abs()).all())


def check_grad(tag, name, new, old, ref):
    e_new, e_old = rel(new, ref), rel(old, ref)
    print(f"\n[train-head-error] {tag} {name}: kernels {e_new:.3e} torch-fp32 {e_old:.3e}")
    assert e_new <= max(GRAD_MARGIN * e_old, GRAD_FLOOR), (tag, name, e_new, e_old)


# ---- 1. criterion op ---------------------------------------------------------------------------------------------------------

def torch_criterion(logits, labels, *, weighted, alpha, gamma, beta, scale):
    """The criterion written out in torch ops: what a training loop runs without the kernel (fp32 on the GPU)."""
    ce = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    if not weighted:
        return ce.mean()
    C = logits.shape[-1]
    p = logits.softmax(-1)
    onehot = torch.nn.functional.one_hot(labels, C)
    frac = ((labels - p.argmax(-1)).abs() / (C - 1)).float()
    w = ((beta * frac.unsqueeze(-1) + alpha * (1 - p) ** gamma) * onehot).sum(-1) * scale
    return (ce * w).mean()


def _golden_sets():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_ref.npz"))
    out = []
    for s in range(int(gold["n_sets"])):
        weighted, alpha, gamma, beta, scale = [float(v) for v in gold[f"params_{s}"]]
        out.append((f"golden{s}", gold[f"logits_{s}"].astype(np.float32), gold[f"labels_{s}"],
                    dict(weighted=bool(weighted), alpha=alpha, gamma=gamma, beta=beta, scale=scale)))
    return out


def _synthetic_sets():
    out = []
    for B, C in ((1, 3), (5, 4), (67, 400), (3, 1000)):       # one row per wave; a partial last workgroup; C past 64 lanes
        rng = np.random.default_rng(B * 1000 + C)
        z = (rng.standard_normal((B, C)) * 2.5).astype(np.float32)
        y = rng.integers(0, C, B)
        for i in range(B):                                    # keep the top two at least 1e-2 apart
            o = np.argsort(z[i])
            if z[i, o[-1]] - z[i, o[-2]] < 1e-2:
                z[i, o[-1]] += 0.05
        if B >= 5:
            z[1, C - 1] = z[1, 0] = z[1].max() + 1.0          # the deliberate exact tie: class 0 wins
            y[1] = C - 1
            y[2] = int(np.argmax(z[2]))                        # a hit
        out.append((f"synth{B}x{C}", z, y, dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)))
    out.append(("synth67x400_plain", out[2][1], out[2][2], dict(weighted=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0)))
    return out


CRITERION_SETS = _golden_sets() + _synthetic_sets()


@pytest.mark.parametrize("tag,z,y,kw", CRITERION_SETS, ids=[s[0] for s in CRITERION_SETS])
def test_criterion_matches_fp64(tag, z, y, kw):
    if tag.startswith("synth"):
        top = np.sort(z.astype(np.float64), axis=1)
        gap = top[:, -1] - top[:, -2]
        assert ((gap >= 1e-3) | (gap == 0)).all() and (gap == 0).sum() == (1 if z.shape[0] >= 5 else 0)   # the test's precondition
    ref = criterion_ref(z, y, **kw)                            # fp64 on the fp32 logits the kernel reads
    logits = torch.from_numpy(z).cuda()
    padded = torch.zeros(z.shape[0], z.shape[1] + 5, device="cuda")
    padded[:, :z.shape[1]] = logits
    labels = torch.from_numpy(y).cuda()
    C = z.shape[1]
    conf = torch.zeros(C, C, dtype=torch.int32, device="cuda")
    out = hip.train_criterion(padded[:, :C], labels, conf=conf, **kw)           # a row stride of its own
    out2 = hip.train_criterion(logits, labels, conf=conf, check_labels=True, **kw)
    assert torch.equal(out["top1"].cpu().long(), torch.from_numpy(ref["top1"]))
    assert int(out["hits"]) == ref["hits"]
    assert torch.equal(conf.cpu().long(), 2 * torch.from_numpy(ref["conf"]))    # two calls: the matrix accumulates
    for key in ("loss", "per_sample", "weight"):
        assert close(out[key], ref[key]), (tag, key)
        assert torch.equal(out[key], out2[key]), (tag, key)
    # backward: upstream gradient on the device
    g1 = torch.ones((), device="cuda")
    d1 = hip.train_criterion_backward(logits, out2["labels"], out2["saved"], g1)
    d8 = hip.train_criterion_backward(padded[:, :C], out["labels"], out["saved"], torch.full((), 0.125, device="cuda"))
    assert torch.equal(d8, d1 * 0.125)
    lt = logits.clone().requires_grad_()
    torch_criterion(lt, labels, **kw).backward()
    check_grad(tag, "dlogits", d1, lt.grad, ref["dlogits"])


def test_criterion_refuses_small_gamma_and_clamps_labels():
    logits = torch.randn(4, 3, device="cuda")
    labels = torch.tensor([0, 1, 2, 1], device="cuda")
    with pytest.raises(hip.GavaError, match="GAVA_EINVAL"):
        hip.train_criterion(logits, labels, weighted=True, gamma=0.5)
    wild = torch.tensor([-5, 1, 99, 1], device="cuda")
    with pytest.raises(hip.GavaError, match="labels outside"):
        hip.train_criterion(logits, wild, weighted=True, check_labels=True)
    a = hip.train_criterion(logits, wild, weighted=True, beta=0.2)               # clamped on the device, never read past the row
    b = hip.train_criterion(logits, torch.tensor([0, 1, 2, 1], device="cuda"), weighted=True, beta=0.2)
    assert torch.equal(a["per_sample"], b["per_sample"]) and torch.equal(a["loss"], b["loss"])


def test_train_criterion_object_under_autograd_and_gradscaler():
    z = torch.randn(6, 5, device="cuda")
    y = torch.tensor([0, 4, 2, 2, 1, 3], device="cuda")
    kw = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)
    ref = criterion_ref(z.cpu().numpy(), y.cpu().numpy(), **kw)
    crit = TrainCriterion(focal_ordinal=True, beta=0.2, track_confusion=True)
    lt = (z * 1.0).requires_grad_()
    mid = lt * 1.0                                     # a non-leaf input, as a model's logits are
    loss = crit(mid, y)
    scaler = torch.amp.GradScaler("cuda", init_scale=512.0)
    scaler.scale(loss / 2).backward()
    assert close(loss.detach(), ref["loss"])
    assert rel(lt.grad / 256.0, ref["dlogits"]) <= 1e-5
    assert set(crit.last) == {"per_sample", "weight", "top1", "hits", "conf"} and all(t.is_cuda for t in crit.last.values())
    assert int(crit.last["hits"]) == ref["hits"] and torch.equal(crit.last["conf"].cpu().long(), torch.from_numpy(ref["conf"]))
    plain = TrainCriterion()
    assert close(plain(z, y), torch.nn.functional.cross_entropy(z.double(), y))
    assert plain.last["conf"] is None
    with pytest.raises(hip.GavaError, match="soft"):
        crit(z, torch.softmax(z, -1))


# ---- 2. head op --------------------------------------------------------------------------------------------------------------

def head_plain(video, text, ls, lb, counts):
    """The head as the plain expression (VitaCLIP_model.py:248,255,287-293), any dtype / device."""
    A = torch.zeros(sum(counts), len(counts), dtype=video.dtype, device=video.device)
    r = 0
    for c, k in enumerate(counts):
        A[r:r + k, c] = 1.0 / k
        r += k
    vn = video / video.norm(dim=-1, keepdim=True)
    tn = text / text.norm(dim=-1, keepdim=True)
    m = A.t() @ tn
    logits = ls.exp() * vn @ m.t()
    if lb is not None:
        logits = logits + lb
    return logits, m / m.norm(dim=-1, keepdim=True)


HEAD_CASES = [(1, [1] * 3, 128), (5, [5] * 3, 512), (17, [1, 3, 2, 5], 768), (33, [1] * 400, 512), (64, [2] * 37, 128)]


@pytest.fixture(scope="module")
def head_refs():
    """fp64 inputs, outputs and gradients of every head case (with bias and with a gradient into text_features), computed once."""
    refs = {}
    for B, counts, E in HEAD_CASES:
        g = torch.Generator().manual_seed(B * 7 + E)
        P, C = sum(counts), len(counts)
        d = dict(video=torch.randn(B, E, generator=g) * 1.7, text=torch.randn(P, E, generator=g) * 0.6 + 0.1,
                 ls=torch.tensor(2.3), lb=torch.tensor(0.37), w_logits=torch.randn(B, C, generator=g), w_tf=torch.randn(C, E, generator=g))
        refs[(B, C, E)] = d
    return refs


def _head_route(d, counts, dtype, device, bias, with_tf, kernels):
    leaves = {k: d[k].to(device=device, dtype=dtype).requires_grad_() for k in ("video", "text", "ls") + (("lb",) if bias else ())}
    lb = leaves.get("lb")
    if kernels:
        off = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=device)
        logits, tf = HeadFn.apply(leaves["video"], leaves["text"], leaves["ls"], lb, off)
    else:
        logits, tf = head_plain(leaves["video"], leaves["text"], leaves["ls"], lb, counts)
    loss = (logits * d["w_logits"].to(device=device, dtype=dtype)).sum()
    if with_tf:
        loss = loss + (tf * d["w_tf"].to(device=device, dtype=dtype)).sum()
    loss.backward()
    return logits.detach(), tf.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("bias,with_tf", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("B,counts,E", HEAD_CASES, ids=[f"B{b}_C{len(c)}_P{sum(c)}_E{e}" for b, c, e in HEAD_CASES])
def test_head_matches_fp64_and_the_inference_head(head_refs, B, counts, E, bias, with_tf):
    C, P = len(counts), sum(counts)
    d = head_refs[(B, C, E)]
    tag = f"head B{B} C{C} P{P} E{E} bias{int(bias)} dtf{int(with_tf)}"
    ref_logits, ref_tf, ref_g = _head_route(d, counts, torch.float64, "cpu", bias, with_tf, kernels=False)
    logits, tf, got = _head_route(d, counts, torch.float32, "cuda", bias, with_tf, kernels=True)
    _, _, old = _head_route(d, counts, torch.float32, "cuda", bias, with_tf, kernels=False)
    assert close(logits, ref_logits) and close(tf, ref_tf)
    if len(set(counts)) == 1:            # equal counts: the bits of gava_similarity_head
        v, t = d["video"].cuda(), d["text"].cuda()
        lg, tfe, vn = torch.empty(B, C, device="cuda"), torch.empty(C, E, device="cuda"), torch.empty(B, E, device="cuda")
        ls, lb = d["ls"].cuda().reshape(1), (d["lb"].cuda().reshape(1) if bias else None)
        hip.check(hip.load().gava_similarity_head(hip.ptr(v), hip.ptr(t), hip.ptr(ls), hip.ptr(lb), B, C, counts[0], E, hip.ptr(lg),
                                                  hip.ptr(tfe), hip.ptr(vn), hip.stream_ptr()), "gava_similarity_head")
        assert torch.equal(logits, lg) and torch.equal(tf, tfe)
    for name in got:
        assert got[name].shape == ref_g[name].shape
        check_grad(tag, "d" + name, got[name], old[name], ref_g[name])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------

def test_same_bits_on_every_run(head_refs):
    tag, z, y, kw = [s for s in CRITERION_SETS if s[0] == "synth67x400"][0]
    logits, labels = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    runs = []
    for _ in range(2):
        out = hip.train_criterion(logits, labels, conf=torch.zeros(400, 400, dtype=torch.int32, device="cuda"), **kw)
        out["dlogits"] = hip.train_criterion_backward(logits, out["labels"], out["saved"], torch.full((), 0.5, device="cuda"))
        runs.append(out)
    for key in ("loss", "per_sample", "weight", "top1", "hits", "conf", "saved", "dlogits"):
        assert torch.equal(runs[0][key], runs[1][key]), key
    B, counts, E = HEAD_CASES[3]
    d = head_refs[(B, len(counts), E)]
    a = _head_route(d, counts, torch.float32, "cuda", True, True, kernels=True)
    b = _head_route(d, counts, torch.float32, "cuda", True, True, kernels=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for name in a[2]:
        assert torch.equal(a[2][name], b[2][name]), name


# ---- 4. model level ----------------------------------------------------------------------------------------------------------

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


def _both_routes(make, x, y, crit_kw, fwd_kw=None, scale=None, aux_weights=None):
    """forward + criterion + backward with train_head = "hip" + TrainCriterion, and with "torch" + the criterion in torch ops."""
    res = {}
    for route in ("hip", "torch"):
        m = make()
        m.train_head = route
        out = m(x, **(fwd_kw or {}))
        logits = out[0]
        if route == "hip":
            crit = TrainCriterion(focal_ordinal=crit_kw["weighted"], alpha=crit_kw["alpha"], gamma=crit_kw["gamma"], beta=crit_kw["beta"],
                                  scale=crit_kw["scale"])
            loss = crit(logits, y)
            assert _graph_has(loss.grad_fn, "HeadFn") and _graph_has(loss.grad_fn, "_CriterionFn") and m.last["head_fn_calls"] == 1
            assert crit.last["hits"].is_cuda
        else:
            loss = torch_criterion(logits, y, **crit_kw)
            assert not _graph_has(loss.grad_fn, "HeadFn") and "head_fn_calls" not in m.last
        if aux_weights is not None:                      # the auxiliary terms stay torch code on the caller's side
            loss = loss + (out[1] * aux_weights[0]).sum() + (out[2] * aux_weights[1]).sum()
        if scale is not None:
            torch.amp.GradScaler("cuda", init_scale=scale).scale(loss).backward()
        else:
            loss.backward()
        res[route] = (logits.detach(), loss.detach(), {n: p.grad for n, p in m.named_parameters()}, m.text_features.detach())
    (lh, loss_h, gh, tfh), (lt, loss_t, gt, tft) = res["hip"], res["torch"]
    assert (lh - lt).abs().max() <= 1e-5 * max(1.0, float(lt.abs().max()))
    assert (tfh - tft).abs().max() <= 1e-5
    assert abs(float(loss_h) - float(loss_t)) <= 1e-5 * max(1.0, abs(float(loss_t)))
    n = 0
    for name, g_ref in gt.items():
        if g_ref is None:
            assert gh[name] is None, name
            continue
        assert gh[name] is not None and bool(torch.isfinite(gh[name]).all()), name
        if float(g_ref.norm()) < 1e-12:
            assert float(gh[name].norm()) < 1e-6, name
            continue
        n += 1
        assert rel(gh[name], g_ref) <= ROUTE_TOL, (name, rel(gh[name], g_ref))
    assert n > 20 and gh["logit_scale"] is not None
    return res


CRIT_KW = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)


def _tiny(extra_kw=None, extra_state=None, **ctor):
    def make():
        m = VitaCLIP(**{**model_kwargs(TINY, CLASSES_3), **(extra_kw or {})}, **ctor)
        sd = synth_torch_state(TINY, 3)
        sd.update(extra_state or {})
        m.load_state_dict(sd, strict=True)
        return m.cuda().train()
    return make


@pytest.fixture(scope="module")
def clip_and_labels():
    return torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda(), torch.tensor([2, 0], device="cuda")


@pytest.mark.parametrize("scale", [None, 1024.0], ids=["plain", "gradscaler"])
def test_model_hip_head_equals_torch_head(clip_and_labels, scale):
    x, y = clip_and_labels
    _both_routes(_tiny(), x, y, CRIT_KW, scale=scale)


def test_model_hip_head_unweighted_criterion(clip_and_labels):
    x, y = clip_and_labels
    _both_routes(_tiny(), x, y, dict(CRIT_KW, weighted=False, beta=0.0))


@pytest.mark.parametrize("descriptor", [False, True], ids=["kapt_n_kv3", "ragged_descriptors"])
def test_model_hip_head_with_several_prompts_per_class(clip_and_labels, tmp_path, monkeypatch, descriptor):
    x, y = clip_and_labels
    if descriptor:
        synth.synth_descriptor_files(str(tmp_path), "updrs", (2, 3, 1))
    else:
        synth.synth_knowledge_files(str(tmp_path), "updrs", 3, ["v1", "v2", "v3"])
    monkeypatch.chdir(tmp_path)
    kw = {"text_prompt_init": "cntn_split_uni_disc", "knowledge_version": ["v1", "v2", "v3"]}
    if descriptor:
        kw["use_descriptor"] = True
    state = {k: torch.from_numpy(v) for k, v in synth.synth_kapt_state(TINY, 3).items()}
    res = _both_routes(_tiny(kw, state), x, y, CRIT_KW)
    assert any("context_prompt_learner.projector" in k and g is not None for k, g in res["hip"][2].items())


def test_model_hip_head_with_auxiliary_heads(clip_and_labels):
    """memory / video_nte supplied: the support-memory head reads text_features, so HeadFn's second output carries a gradient."""
    x, y = clip_and_labels
    state = {k: torch.from_numpy(v) for k, v in synth.synth_aux_state(TINY, 3).items()}
    nte, mem = synth.synth_aux_inputs(2, TINY.embed_dim)
    fwd = dict(memory=torch.from_numpy(mem).cuda(), video_nte=torch.from_numpy(nte).cuda())
    g = torch.Generator().manual_seed(2)
    make = _tiny(None, state, add_nte=True, use_support_memory=True, detach_features=False, num_classes=3)
    probe = make()
    with torch.no_grad():
        _, lmt, lvm = probe.eval()(x, **fwd)
    w = (torch.randn(lmt.shape, generator=g).cuda(), torch.randn(lvm.shape, generator=g).cuda())
    res = _both_routes(make, x, y, CRIT_KW, fwd_kw=fwd, aux_weights=w)
    assert any(n.startswith("tf_project") and g is not None for n, g in res["hip"][2].items())      # the memory head was live
