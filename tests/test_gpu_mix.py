"""GPU: Mixup / CutMix on the device and the criterion for soft targets (gava_mix_clips, gava_mix_targets, gava_soft_criterion*,
gava_clip_amd.ClipMixer, gava_clip_amd.SoftTargetCriterion) against the fp64 restatement tests/mix_ref.py.

Clips: CutMix pixels, self-partnered clips and Mixup with lam in {0, 1} are compared bit for bit; the other Mixup pixels meet
|delta| <= 2^-22 (lam |a| + (1 - lam) |b|) against fp64 on the fp32 lam the kernel reads - three fp32 roundings (1 - lam, one
product, the final fma) of 2^-24 relative each, plus one spare.  In place equals out of place bit for bit, and so does a
second call.

Targets: rtol 1e-6 (formed in fp64 and rounded once: 6e-8, plus eps as fp32), exact where lam in {0, 1} and eps == 0.

Criterion: loss, per_sample, weight against fp64 on the fp32 inputs at rtol 1e-5 / atol 1e-5, the bound of
tests/test_gpu_train_head.py; top1, target1, hits, conf exact.  The gradient follows that file's rule: computed by the kernels
and by the same expression in torch fp32 on the GPU, both judged norm-wise against fp64; the kernels pass at
max(4 x the torch route's error, 1e-6); both errors are printed ([soft-criterion-error] lines).  Synthetic sets: row i is of
kind i % 6 - one-hot, targets summing to 1.7, all-zero targets, two equal largest logits, two equal largest targets, a
confident row (top logit 30 above the rest) - so a set of fewer than six rows holds the first B kinds.

Model level: one TINY step by ClipMixer + SoftTargetCriterion against the same step with the mix and the criterion in torch
ops: 2e-2 norm-wise per parameter, the figure of tests/test_gpu_backward.py for two routes of one computation."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import ClipMixer, SoftTargetCriterion, VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402
import mix_ref  # noqa: E402

GRAD_MARGIN, GRAD_FLOOR = 4.0, 1e-6
ROUTE_TOL = 2e-2          # tests/test_gpu_backward.py: two routes of the same computation, norm-wise per parameter
MIX_BOUND = 2.0 ** -22


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def close(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return bool(((got - ref).abs() <= 1e-5 + 1e-5 * ref.abs()).all())


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. clips ------------------------------------------------------------------------------------------------------------------

MIX_SHAPES = [(1, 3, 4, 4), (2, 6, 8, 8), (5, 6, 6, 10), (4, 9, 16, 20), (3, 6, 5, 7), (4, 24, 224, 224)]


def _plans(B, H, W):
    """(name, partner, lam, box) of every plan one shape is mixed by; partner = the batch reversed unless said otherwise."""
    rev = B - 1 - np.arange(B)
    none = np.zeros((B, 4), dtype=np.int32)
    out = []
    for lam in (0.0, 1.0, 0.5, 0.3):
        out.append((f"mixup{lam}", rev, np.full(B, lam, dtype=np.float32), none))
    inner = (1, max(H - 1, 2), min(3, W - 1), max(W - 3, min(3, W - 1) + 1))       # (4, 9, 16, 20): columns 3 .. 17
    for name, box in (("full", (0, H, 0, W)), ("last_pixel", (H - 1, H, W - 1, W)), ("two_borders", (0, H // 2 + 1, 0, W // 2 + 1)),
                      ("inner", inner)):
        out.append((f"cutmix_{name}", rev, np.full(B, 0.4, dtype=np.float32), np.tile(np.array(box, dtype=np.int32), (B, 1))))
    # elem: the members of a pair differ in lam and in kind (the first Mixup, the last CutMix)
    lam = (0.3 + 0.1 * np.arange(B)).astype(np.float32) % 1.0
    box = none.copy()
    box[B - 1] = (H // 3, H, 1 if W > 1 else 0, W - 1 if W > 2 else W)
    if B >= 4:
        box[1] = (0, 1, 0, W)
    out.append(("elem", rev, lam, box))
    return out


@pytest.fixture(scope="module")
def clips():
    made = {}
    for shape in MIX_SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(shape, generator=g) * 2.0 + 0.25
        x.view(-1)[::97] = -0.0                                  # a copy keeps the sign of a zero
        made[shape] = x
    return made


def _check_mix(name, x_host, out, partner, lam, box):
    ref, exact, scale = mix_ref.mix_clips(x_host.numpy(), partner, lam, box)
    got = out.cpu().numpy()
    want_bits = ref.astype(np.float32).view(np.uint32)           # a selection of fp32 values: the cast is exact
    assert np.array_equal(got.view(np.uint32)[exact], want_bits[exact]), name
    if not exact.all():
        err = np.abs(got.astype(np.float64) - ref)[~exact]
        bound = MIX_BOUND * scale[~exact]
        print(f"\n[mix-error] {name}: worst |delta| / (lam |a| + (1 - lam) |b|) = {float((err / np.maximum(scale[~exact], 1e-300)).max()):.3e}"
              f" (bound {MIX_BOUND:.3e})")
        assert (err <= bound).all(), name


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=["x".join(map(str, s)) for s in MIX_SHAPES])
def test_mix_clips_matches_fp64(clips, shape):
    B, planes, H, W = shape
    x_host = clips[shape]
    x = x_host.cuda()
    for name, partner, lam, box in _plans(B, H, W):
        tag = f"{shape} {name}"
        desc = hip.mix_descriptors(dict(partner=partner, lam=lam, box=box), H, W)
        out = hip.mix_clips(x, desc)
        assert torch.equal(x.cpu(), x_host)                       # out of place leaves x alone
        _check_mix(tag, x_host, out, partner, lam, box)
        again = hip.mix_clips(x, desc, out=torch.full_like(x, float("nan")))
        assert torch.equal(bits(again), bits(out)), tag           # the same bits on every run
        inplace = x.clone()
        assert hip.mix_clips(inplace, desc, out=inplace) is inplace
        assert torch.equal(bits(inplace), bits(out)), tag         # in place == out of place, bit for bit
    if B >= 3:
        rot = (np.arange(B) + 1) % B                               # no involution: out of place only
        lam = np.full(B, 0.3, dtype=np.float32)
        box = np.zeros((B, 4), dtype=np.int32)
        box[0] = (0, H, 0, (W + 1) // 2)
        desc = hip.mix_descriptors(dict(partner=rot, lam=lam, box=box), H, W)
        _check_mix(f"{shape} rotation", x_host, hip.mix_clips(x, desc), rot, lam, box)
        keep = x.clone()
        with pytest.raises(hip.GavaError, match="GAVA_EINVAL"):
            hip.mix_clips(keep, desc, out=keep)
        assert torch.equal(bits(keep), bits(x))


def test_mix_clips_narrow_path_for_an_unaligned_base(clips):
    """W % 4 == 0 but the base is 4 bytes off a 16-byte boundary: the element path, the same values."""
    shape = (2, 6, 8, 8)
    B, planes, H, W = shape
    x_host = clips[shape]
    buf = torch.empty(x_host.numel() + 1, device="cuda")
    x = buf[1:].view(shape).copy_(x_host)
    assert x.data_ptr() % 16 == 4
    for name, partner, lam, box in _plans(B, H, W):
        desc = hip.mix_descriptors(dict(partner=partner, lam=lam, box=box), H, W)
        out = hip.mix_clips(x, desc)
        _check_mix(f"unaligned {name}", x_host, out, partner, lam, box)
        assert torch.equal(bits(out), bits(hip.mix_clips(x_host.cuda(), desc))), name       # the vector path's bits


# ---- 2. targets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 5, 400])
def test_mix_targets_matches_fp64(C, eps):
    B = 7
    labels = np.array([0, C - 1, 1, 999, -3, C // 2, 1], dtype=np.int64)             # two out of range: clamped to C - 1 and 0
    partner = B - 1 - np.arange(B)
    lam = np.array([0.0, 1.0, 0.5, 0.3, 0.5, 0.25, 1.0], dtype=np.float32)
    desc = hip.mix_descriptors(dict(partner=partner, lam=lam, box=np.zeros((B, 4), dtype=np.int32)), 8, 8)
    got = hip.mix_targets(torch.from_numpy(labels).cuda(), desc, C, eps)
    ref = mix_ref.mix_targets(labels, partner, lam, C, eps)
    assert got.shape == (B, C) and got.dtype == torch.float32
    g = got.cpu().double().numpy()
    assert (np.abs(g - ref) <= 1e-6 * np.abs(ref)).all()
    if eps == 0.0:
        sure = np.isin(lam, (0.0, 1.0)) | (partner == np.arange(B))
        assert np.array_equal(g[sure], ref[sure])
    assert torch.equal(got, hip.mix_targets(torch.from_numpy(labels).cuda().int(), desc, C, eps))    # any integer type


# ---- 3. criterion --------------------------------------------------------------------------------------------------------------

def torch_soft_criterion(logits, targets, *, weighted, alpha, gamma, beta, scale):
    """The criterion written out in torch ops: what a training loop runs without the kernel (fp32 on the GPU)."""
    ce = torch.nn.functional.cross_entropy(logits, targets, reduction="none")
    if not weighted:
        return ce.mean()
    C = logits.shape[-1]
    p = logits.softmax(-1)
    frac = ((targets.argmax(-1) - p.argmax(-1)).abs() / (C - 1)).float()
    w = ((beta * frac.unsqueeze(-1) + alpha * (1 - p) ** gamma) * targets).sum(-1) * scale
    return (ce * w).mean()


def _golden_sets():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_loss_ref.npz"))
    out = []
    for s in range(int(gold["n_sets"])):
        weighted, alpha, gamma, beta, scale = [float(v) for v in gold[f"params_{s}"]]
        out.append((f"golden{s}", gold[f"logits_{s}"].astype(np.float32), gold[f"targets_{s}"].astype(np.float32),
                    dict(weighted=bool(weighted), alpha=alpha, gamma=gamma, beta=beta, scale=scale)))
    return out


def _synthetic_sets():
    out = []
    eps = 0.1
    for B, C in ((1, 3), (5, 4), (67, 400), (3, 1000), (257, 5)):     # one row per wave; partial last workgroups; C past 64 lanes
        rng = np.random.default_rng(B * 1000 + C)
        z = (rng.standard_normal((B, C)) * 2.5).astype(np.float32)
        t = np.full((B, C), eps / C)
        for i in range(B):
            ya, yb = rng.integers(0, C, 2)
            lam = rng.uniform(0.05, 0.45) if rng.random() < 0.5 else rng.uniform(0.55, 0.95)
            t[i, ya] += lam * (1 - eps)
            t[i, yb] += (1 - lam) * (1 - eps)
            kind = i % 6
            if kind == 0:                                          # one-hot
                t[i] = 0.0
                t[i, ya] = 1.0
            elif kind == 1:                                        # tau = 1.7
                t[i] *= 1.7
            elif kind == 2:                                        # all-zero targets
                t[i] = 0.0
            elif kind == 4:                                        # lam = 0.5 of two labels: two equal largest targets
                a, b = (ya, yb) if ya != yb else (ya, (ya + 1) % C)
                t[i] = eps / C
                t[i, a] = t[i, b] = eps / C + 0.45
            elif kind == 5:                                        # a confident row
                z[i] = rng.standard_normal(C).astype(np.float32) * 0.1
                z[i, ya] = z[i].max() + 30.0
        t = t.astype(np.float32)
        for i in range(B):                                         # keep the top two at least 1e-2 apart ...
            o = np.argsort(z[i])
            if z[i, o[-1]] - z[i, o[-2]] < 1e-2:
                z[i, o[-1]] += 0.05
            o = np.argsort(t[i])
            if i % 6 not in (2, 4) and t[i, o[-1]] - t[i, o[-2]] < 1e-2:
                t[i, o[-1]] += 0.05
            if i % 6 == 3:                                         # ... but for the deliberate exact tie: the lower class wins
                z[i, C - 1] = z[i, 0] = z[i].max() + 1.0
        out.append((f"synth{B}x{C}", z, t, dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)))
    out.append(("synth67x400_plain", out[2][1], out[2][2], dict(weighted=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0)))
    return out


CRITERION_SETS = _golden_sets() + _synthetic_sets()


def _top_gap(a):
    top = np.sort(a.astype(np.float64), axis=1)
    return top[:, -1] - top[:, -2]


@pytest.mark.parametrize("tag,z,t,kw", CRITERION_SETS, ids=[s[0] for s in CRITERION_SETS])
def test_soft_criterion_matches_fp64(tag, z, t, kw):
    B, C = z.shape
    if tag.startswith("synth"):
        gz, gt = _top_gap(z), _top_gap(t)
        assert (((gz >= 1e-3) | (gz == 0)) & ((gt >= 1e-3) | (gt == 0))).all()                        # the test's precondition
        kinds = np.arange(B) % 6
        assert (gz[kinds == 3] == 0).all() and (gt[kinds == 4] == 0).all() and not t[kinds == 2].any()
        assert (gz == 0).sum() == (kinds == 3).sum()
    ref = mix_ref.soft_criterion(z, t, **kw)                       # fp64 on the fp32 inputs the kernel reads
    logits, targets = torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda()
    pad_z, pad_t = torch.zeros(B, C + 5, device="cuda"), torch.full((B, C + 3), 7.0, device="cuda")
    pad_z[:, :C], pad_t[:, :C] = logits, targets
    conf = torch.zeros(C, C, dtype=torch.int32, device="cuda")
    out = hip.soft_criterion(pad_z[:, :C], pad_t[:, :C], conf=conf, **kw)                             # row strides of their own
    out2 = hip.soft_criterion(logits, targets, conf=conf, **kw)
    assert torch.equal(out["top1"].cpu().long(), torch.from_numpy(ref["top1"]))
    assert torch.equal(out["target1"].cpu().long(), torch.from_numpy(ref["target1"]))
    assert int(out["hits"]) == ref["hits"]
    assert torch.equal(conf.cpu().long(), 2 * torch.from_numpy(ref["conf"]))                          # two calls: the matrix accumulates
    for key in ("loss", "per_sample", "weight"):
        assert close(out[key], ref[key]), (tag, key)
        assert torch.equal(out[key], out2[key]), (tag, key)
    g1 = torch.ones((), device="cuda")
    d1 = hip.soft_criterion_backward(logits, targets, out2["saved"], g1, **kw)
    d8 = hip.soft_criterion_backward(pad_z[:, :C], pad_t[:, :C], out["saved"], torch.full((), 0.125, device="cuda"), **kw)
    assert torch.equal(d8, d1 * 0.125)
    zero = ~t.any(axis=1)
    if zero.any():                                                 # an all-zero target row: no loss, no gradient, exactly
        rows = torch.from_numpy(zero).cuda()
        assert bool((out["per_sample"][rows] == 0).all()) and bool((d1[rows] == 0).all())
    lt = logits.clone().requires_grad_()
    torch_soft_criterion(lt, targets, **kw).backward()
    e_new, e_old = rel(d1, ref["dlogits"]), rel(lt.grad, ref["dlogits"])
    print(f"\n[soft-criterion-error] {tag} dlogits: kernels {e_new:.3e} torch-fp32 {e_old:.3e}")
    assert e_new <= max(GRAD_MARGIN * e_old, GRAD_FLOOR), (tag, e_new, e_old)


@pytest.mark.parametrize("B,C,weighted", [(5, 4, True), (67, 400, True), (67, 400, False)])
def test_soft_criterion_on_one_hot_targets_meets_the_label_criterion(B, C, weighted):
    rng = np.random.default_rng(B + C)
    z = torch.from_numpy((rng.standard_normal((B, C)) * 2.5).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, B)).cuda()
    kw = dict(weighted=weighted, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)
    hard = hip.train_criterion(z, y, **kw)
    soft = hip.soft_criterion(z, torch.nn.functional.one_hot(y, C).float(), **kw)
    for key in ("loss", "per_sample", "weight"):
        assert close(soft[key], hard[key]), key
    assert torch.equal(soft["top1"], hard["top1"]) and torch.equal(soft["hits"], hard["hits"])
    assert torch.equal(soft["target1"].long(), y)
    dh = hip.train_criterion_backward(z, hard["labels"], hard["saved"], torch.ones((), device="cuda"))
    ds = hip.soft_criterion_backward(z, torch.nn.functional.one_hot(y, C).float(), soft["saved"], torch.ones((), device="cuda"), **kw)
    assert rel(ds, dh) <= 1e-5


def test_same_bits_on_every_run():
    tag, z, t, kw = [s for s in CRITERION_SETS if s[0] == "synth67x400"][0]
    logits, targets = torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda()
    runs = []
    for _ in range(2):
        out = hip.soft_criterion(logits, targets, conf=torch.zeros(400, 400, dtype=torch.int32, device="cuda"), **kw)
        out["dlogits"] = hip.soft_criterion_backward(logits, targets, out["saved"], torch.full((), 0.5, device="cuda"), **kw)
        runs.append(out)
    for key in ("loss", "per_sample", "weight", "top1", "target1", "hits", "conf", "saved", "dlogits"):
        assert torch.equal(runs[0][key], runs[1][key]), key


# ---- 4. objects ----------------------------------------------------------------------------------------------------------------

def test_soft_target_criterion_object_under_autograd_and_gradscaler():
    g = torch.Generator().manual_seed(1)
    z = torch.randn(6, 5, generator=g).cuda()
    t = torch.softmax(torch.randn(6, 5, generator=g) * 2, -1).cuda()
    kw = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)
    ref = mix_ref.soft_criterion(z.cpu().numpy(), t.cpu().numpy(), **kw)
    crit = SoftTargetCriterion(focal_ordinal=True, beta=0.2, track_confusion=True)
    lt = (z * 1.0).requires_grad_()
    mid = lt * 1.0                                     # a non-leaf input, as a model's logits are
    tt = t.clone().requires_grad_()                    # no gradient flows to the targets
    loss = crit(mid, tt)
    scaler = torch.amp.GradScaler("cuda", init_scale=512.0)
    scaler.scale(loss / 2).backward()
    assert close(loss.detach(), ref["loss"])
    assert rel(lt.grad / 256.0, ref["dlogits"]) <= 1e-5
    assert tt.grad is None
    assert set(crit.last) == {"per_sample", "weight", "top1", "target1", "hits", "conf"} and all(v.is_cuda for v in crit.last.values())
    assert int(crit.last["hits"]) == ref["hits"] and torch.equal(crit.last["conf"].cpu().long(), torch.from_numpy(ref["conf"]))
    assert torch.equal(crit.last["target1"].cpu().long(), torch.from_numpy(ref["target1"]))
    plain = SoftTargetCriterion()
    assert close(plain(z, t), torch.nn.functional.cross_entropy(z.double(), t.double()))
    assert plain.last["conf"] is None
    with pytest.raises(hip.GavaError, match="TrainCriterion"):
        crit(z, torch.tensor([0, 4, 2, 2, 1, 3], device="cuda"))


def test_clip_mixer_object():
    B, T, S, C = 4, 2, 8, 5
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 3, T, S, S, generator=g).cuda()
    y = torch.tensor([0, 4, 2, 1], device="cuda")
    plan = dict(partner=np.array([3, 2, 1, 0], dtype=np.int32), lam=np.array([0.3, 0.75, 0.75, 0.5], dtype=np.float32),
                box=np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 7, 2, 5]], dtype=np.int32))
    mixer = ClipMixer(C, label_smoothing=0.1, seed=0)
    xm, t = mixer(x, y, plan=plan)
    desc = hip.mix_descriptors(plan, S, S)
    assert xm is not x and xm.shape == x.shape and torch.equal(bits(xm), bits(hip.mix_clips(x, desc)))
    assert torch.equal(t, hip.mix_targets(y, desc, C, 0.1)) and t.shape == (B, C)
    keep = x.clone()
    xi, ti = mixer(keep, y, plan=plan, inplace=True)
    assert xi is keep and torch.equal(bits(keep), bits(xm)) and torch.equal(ti, t)
    # a drawn plan: the result is the op calls on mixer.last_plan
    xd, td = ClipMixer(C, mode="elem", seed=5)(x, y)
    drawn = ClipMixer(C, mode="elem", seed=5).draw(B, S, S)
    d2 = hip.mix_descriptors(drawn, S, S)
    assert torch.equal(bits(xd), bits(hip.mix_clips(x, d2))) and torch.equal(td, hip.mix_targets(y, d2, C, 0.1))
    # nothing mixed: x itself, the targets only smoothed
    for off in (ClipMixer(C, prob=0.0, label_smoothing=0.1), ClipMixer(C, mixup_alpha=0.0, cutmix_alpha=0.0, label_smoothing=0.1)):
        x0, t0 = off(x, y)
        assert x0 is x
        want = torch.full((B, C), 0.1 / C, dtype=torch.float64)
        want[torch.arange(B), y.cpu()] += 0.9
        assert bool(((t0.cpu().double() - want).abs() <= 1e-6 * want).all())
    with pytest.raises(hip.GavaError, match="requires grad"):
        mixer(x.clone().requires_grad_(), y)
    with pytest.raises(hip.GavaError, match="device"):
        mixer(x.cpu(), y.cpu())
    with pytest.raises(hip.GavaError, match="fp32"):
        mixer(x.half(), y)
    with pytest.raises(hip.GavaError, match="integer"):
        mixer(x, y.float())
    with pytest.raises(hip.GavaError, match="contiguous"):
        mixer(x.transpose(3, 4), y, inplace=True)
    xt, _ = mixer(x.transpose(3, 4), y, plan=plan)                  # out of place takes any layout
    assert torch.equal(bits(xt), bits(hip.mix_clips(x.transpose(3, 4).contiguous(), desc)))


# ---- 5. one training step ------------------------------------------------------------------------------------------------------

def _torch_mix(x, y, plan, C, eps):
    """The mix and its targets in torch ops: what a training loop runs without the kernels."""
    partner = torch.from_numpy(np.asarray(plan["partner"])).long().to(x.device)
    out = x.clone()
    for i in range(x.shape[0]):
        j = int(plan["partner"][i])
        y0, y1, x0, x1 = (int(v) for v in plan["box"][i])
        lam = float(plan["lam"][i])
        if j == i:
            continue
        if y1 > y0 and x1 > x0:
            out[i, ..., y0:y1, x0:x1] = x[j, ..., y0:y1, x0:x1]
        else:
            out[i] = x[i] * lam + x[j] * (1 - lam)
    s = torch.full((x.shape[0], C), eps / C, device=x.device)
    s[torch.arange(x.shape[0]), y] += 1 - eps
    lam = torch.from_numpy(np.asarray(plan["lam"])).float().to(x.device)[:, None]
    return out, lam * s + (1 - lam) * s[partner]


def test_tiny_training_step_with_mixer_and_soft_criterion():
    B, C = 4, 3
    S = TINY.input_size
    x = torch.from_numpy(synth.synth_clip(B, TINY.num_frames, S)).cuda()
    y = torch.tensor([2, 0, 1, 0], device="cuda")
    plan = dict(partner=np.array([3, 2, 1, 0], dtype=np.int32), lam=np.array([0.3, 0.6, 0.6, 0.55], dtype=np.float32),
                box=np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [S // 4, S - 3, 5, S // 2 + 2]], dtype=np.int32))
    kw = dict(weighted=True, alpha=0.25, gamma=2.0, beta=0.2, scale=1.0)
    model = VitaCLIP(**model_kwargs(TINY, CLASSES_3))
    model.load_state_dict(synth_torch_state(TINY, 3), strict=True)
    model = model.cuda().train()
    grads = {}
    for route in ("hip", "torch"):
        model.zero_grad(set_to_none=True)
        if route == "hip":
            mixer, crit = ClipMixer(C, label_smoothing=0.1), SoftTargetCriterion(focal_ordinal=True, beta=0.2)
            xm, t = mixer(x, y, plan=plan)
            loss = crit(model(xm)[0], t)
            assert crit.last["hits"].is_cuda
        else:
            xm, t = _torch_mix(x, y, plan, C, 0.1)
            loss = torch_soft_criterion(model(xm)[0], t, **kw)
        loss.backward()
        grads[route] = (loss.detach().clone(), {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()})
    (loss_h, gh), (loss_t, gt) = grads["hip"], grads["torch"]
    print(f"\n[mix-step] loss: kernels {float(loss_h):.7f} torch ops {float(loss_t):.7f}")
    assert abs(float(loss_h) - float(loss_t)) <= ROUTE_TOL * abs(float(loss_t))      # the towers run in 16 bits on inputs an ulp apart
    n, worst = 0, ("", 0.0)
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert gh[name] is None and gt[name] is None, name      # frozen parameters stay None
            continue
        assert gh[name] is not None and bool(torch.isfinite(gh[name]).all()), name      # every trainable parameter has a gradient
        assert gt[name] is not None, name
        if float(gt[name].norm()) < 1e-12:
            assert float(gh[name].norm()) < 1e-6, name
            continue
        n += 1
        if name.endswith("k_proj.bias"):
            # softmax is invariant to a constant added to every key: this gradient is exactly zero in exact arithmetic and both
            # routes return rounding noise, so the difference is measured against the scale of its sibling, d q_proj.bias
            # (tests/test_gpu_backward.py does the same against the oracle)
            scale = gt[name.replace("k_proj", "q_proj")].norm()
            e = float((gh[name] - gt[name]).norm() / scale)
            assert float(gt[name].norm()) <= 0.2 * float(scale), name
            assert e <= ROUTE_TOL, (name, e)
            continue
        e = rel(gh[name], gt[name])
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e <= ROUTE_TOL, (name, e)
    print(f"\n[mix-step] {n} parameters, worst norm-wise difference of the two routes {worst[1]:.3e} ({worst[0]})")
    assert n > 20
