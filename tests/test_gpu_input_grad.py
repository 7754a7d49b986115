"""GPU: the gradient with respect to the input clip - gava_unpatchify op by op, then x.grad and VitaCLIP.saliency end to end.

Op level.  The fold is a permutation: GRAD and ABSMAX (|.| and max are exact) must equal the torch restatement
(tests/input_grad_ref.py, pinned to autograd by tests/test_input_grad_host.py) bit for bit.  GRAD_X_INPUT is three fp32 roundings of a
three-term sum and L2 three plus the square root's: 4 * 2^-24 * sum_c |g_c x_c| and 4 * 2^-24 * value against fp64.  The patch
dgrad GEMM in front of the fold carries the accumulation bound tests/test_gpu_train_ops.py applies to EPI_F32 dgrad GEMMs.

Model level.  The reference is the fixture the REFERENCE produced (tests/golden/tiny_input_grads.npz) or the fp32 oracle under
autograd; the bound is the project's frozen gradient criterion, 4e-2 norm-wise (bf16 gradient operands through every block
against fp32), over the whole dx and per clip.  Every case prints an [input-grad-error] line; a record of one run is
profiles/input_grad_errors.txt."""
import ctypes
import dataclasses
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gava_clip_amd import VitaCLIP, hip, synth  # noqa: E402
from gava_clip_amd.config import TINY, VIT_B16_T8  # noqa: E402
from oracle.vita_oracle import Oracle  # noqa: E402  (checker only)
from helpers import CLASSES_3, model_kwargs, synth_torch_state  # noqa: E402
import input_grad_ref as ref  # noqa: E402

BF = hip.PREC_BF16
F64 = torch.float64
U = 2.0 ** -24
ACC = 2 ** -18          # fp32 accumulation of a dgrad GEMM, relative to |A|.|W|^T (tests/test_gpu_train_ops.py)
GRAD_TOL = 4e-2         # the frozen norm-wise criterion of the backward's gradients (tests/test_gpu_backward.py)
MODES = (hip.UNPATCH_GRAD, hip.UNPATCH_ABSMAX, hip.UNPATCH_L2, hip.UNPATCH_GRAD_X_INPUT)
#        B, T, size, P, ld, frame_rows, row_offset
CASES = [(2, 3, 64, 16, 768, 17, 1),      # the model's form: CLS row skipped, no padding columns
         (1, 2, 28, 14, 640, 5, 1),       # P = 14: 588 columns in rows of 640, 8-byte accesses
         (2, 1, 32, 16, 776, 4, 0)]       # the dense form, 8 padding columns


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def note(tag, **values):
    print(f"\n[input-grad-error] {tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in values.items()))


def _inputs(B, T, size, P, ld, frame_rows, row_offset, seed=0):
    """dpatch with NaN in every row and column the kernel must not read, and a clip; random values, so every plane is distinct."""
    g = torch.Generator().manual_seed(1000 * seed + size + P)
    n = (size // P) ** 2
    dp = torch.full((B * T, frame_rows, ld), float("nan"))
    dp[:, row_offset:row_offset + n, :3 * P * P] = torch.randn(B * T, n, 3 * P * P, generator=g)
    return dp, torch.randn(B, 3, T, size, size, generator=g)


def _run(dp, x, mode, B, T, size, P, ld, frame_rows, row_offset):
    shape = (B, 3, T, size, size) if mode == hip.UNPATCH_GRAD else (B, T, size, size)
    out = torch.full(shape, float("nan"), device="cuda")
    hip.unpatchify(dp, out, B=B, T=T, size=size, patch=P, mode=mode, frame_rows=frame_rows, row_offset=row_offset,
                   x=x if mode == hip.UNPATCH_GRAD_X_INPUT else None)
    return out


def _check_maps(tag, g32, x32, absmax, l2, gxi):
    """The three maps of a device gradient g32 [B, 3, T, S, S] against the restatement: absmax exact, the other two within the
    op-level bounds of fp64."""
    assert torch.equal(absmax, ref.reduce_map(g32, ref.ABSMAX)), tag
    g64, x64 = g32.to(F64), x32.to(F64)
    want = ref.reduce_map(g64, ref.L2)
    r_l2 = float(((l2.to(F64) - want).abs() / (4 * U * want)).max())
    want = ref.reduce_map(g64, ref.GRAD_X_INPUT, x64)
    r_gxi = float(((gxi.to(F64) - want).abs() / (4 * U * (g64 * x64).abs().sum(1))).max())
    print(f"\n[input-grad-error] {tag}: l2 {r_l2:.3f} of its bound, grad_x_input {r_gxi:.3f} of its bound")
    assert r_l2 <= 1 and r_gxi <= 1, (tag, r_l2, r_gxi)


@pytest.mark.parametrize("case", CASES)
def test_unpatchify_matches_the_restatement(case):
    B, T, size, P, ld, frame_rows, row_offset = case
    dp, x = _inputs(*case)
    dpd, xd = dp.cuda(), x.cuda()
    outs = [_run(dpd, xd, mode, *case) for mode in MODES]
    again = [_run(dpd, xd, mode, *case) for mode in MODES]
    for a, b in zip(outs, again):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)            # nothing skipped read, nothing left unwritten, repeatable
    want = ref.unpatchify(dp, B, T, size, P, frame_rows, row_offset, ref.GRAD)
    assert torch.equal(outs[0].cpu(), want)
    _check_maps(f"op {case}", outs[0], xd, *outs[1:])
    # the three-dimensional view of the same buffer is the same call
    assert torch.equal(_run(dpd.view(B * T * frame_rows, ld), xd, hip.UNPATCH_ABSMAX, *case), outs[1])


def test_unpatchify_more_frames_than_one_grid_dimension_holds():
    """B*T just past 65535 (the z extent the patchify launch is cut at), one 16 x 16 patch per frame."""
    B, T, size, P, ld = 32770, 2, 16, 16, 768
    dp = torch.randn(B * T, 1, ld, generator=torch.Generator().manual_seed(9)).cuda()
    got = _run(dp, None, hip.UNPATCH_GRAD, B, T, size, P, ld, 1, 0)
    assert torch.equal(got, ref.unpatchify(dp, B, T, size, P, 1, 0, ref.GRAD))
    amax = _run(dp, None, hip.UNPATCH_ABSMAX, B, T, size, P, ld, 1, 0)
    assert torch.equal(amax, ref.reduce_map(got, ref.ABSMAX))
    assert torch.equal(amax[-1, -1], dp[-1, 0].view(3, 16, 16).abs().amax(0))


def test_unpatchify_refusals_leave_the_output_untouched():
    B, T, size, P, ld, frame_rows, row_offset = CASES[1]
    dp, x = _inputs(*CASES[1])
    dpd, xd = dp.cuda(), x.cuda()
    out = torch.full((B, 3, T, size, size), 7.0, device="cuda")      # large enough for every mode
    lib = hip.load()

    def call(**kw):
        a = hip.UnpatchifyArgs()
        a.dpatch, a.ld, a.out, a.x = dpd.data_ptr(), ld, out.data_ptr(), None
        a.B, a.T, a.size, a.patch, a.mode, a.frame_rows, a.row_offset = B, T, size, P, hip.UNPATCH_ABSMAX, frame_rows, row_offset
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gava_unpatchify(ctypes.byref(a), hip.stream_ptr())

    bad = [dict(dpatch=None), dict(out=None), dict(dpatch=dpd.data_ptr() + 4), dict(out=out.data_ptr() + 8),
           dict(mode=hip.UNPATCH_GRAD_X_INPUT, x=xd.data_ptr() + 4), dict(size=30), dict(ld=587), dict(frame_rows=4), dict(row_offset=2),
           dict(row_offset=-1), dict(mode=4), dict(mode=-1), dict(mode=hip.UNPATCH_GRAD_X_INPUT), dict(x=xd.data_ptr()),
           dict(mode=hip.UNPATCH_GRAD, x=xd.data_ptr()), dict(mode=hip.UNPATCH_L2, x=xd.data_ptr()),
           dict(B=0), dict(T=0), dict(size=0), dict(patch=0), dict(B=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and call(mode=hip.UNPATCH_GRAD_X_INPUT, x=xd.data_ptr()) == 0      # the same call without the fault goes through
    with pytest.raises(hip.GavaError, match="fp32"):
        hip.unpatchify(dpd.half(), out[:, 0], B=B, T=T, size=size, patch=P, mode=hip.UNPATCH_ABSMAX, frame_rows=frame_rows, row_offset=row_offset)


@pytest.mark.parametrize("D", [128, 768])
def test_patch_dgrad_and_fold_match_fp64(D):
    """_input_backward's two launches on their own: d rows (bf16) x the patch weight in dgrad orientation, then the fold with each
    frame's CLS row skipped - against fp64 on the same bf16-rounded operands."""
    B, T, size, P = 1, 2, 64, 16
    n1, cols = (size // P) ** 2 + 1, 3 * P * P
    g = torch.Generator().manual_seed(D)
    d16 = torch.randn(B * T * n1, D, generator=g).bfloat16()
    w16 = (torch.randn(cols, D, generator=g) / D ** 0.5).bfloat16()          # conv weight [D][3 P^2], transposed
    dpatch = torch.full((B * T * n1, cols), float("nan"), device="cuda")
    hip.gemm(d16.cuda(), w16.cuda(), None, dpatch, epilogue=hip.EPI_F32, prec=BF)
    got = _run(dpatch, None, hip.UNPATCH_GRAD, B, T, size, P, cols, n1, 1).cpu()
    A64, W64 = d16.to(F64), w16.to(F64)
    want = ref.fold(A64 @ W64.t(), B, T, size, P, n1, 1)
    bound = ref.fold(ACC * (A64.abs() @ W64.abs().t()), B, T, size, P, n1, 1) + 2 ** -23 * want.abs()
    worst = float(((got.to(F64) - want).abs() / bound).max())
    print(f"\n[input-grad-error] patch dgrad + fold D={D}: {worst:.3f} of its bound")
    assert worst <= 1


# ---- model level ---------------------------------------------------------------------------------------------------------------

def _model(cfg=TINY, keep=True, train=True):
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3), strict=True)
    m = m.cuda()
    m = m.train() if train else m.eval()
    if not keep:
        m.keep_activation_bytes = 0
    return m


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _check_dx(tag, got, want):
    assert got is not None and got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous(), tag
    assert bool(torch.isfinite(got).all()), tag
    whole, clips = rel(got.cpu(), want), [rel(got[b].cpu(), want[b]) for b in range(want.shape[0])]
    note(tag, whole=whole, **{f"clip{b}": e for b, e in enumerate(clips)})
    assert whole <= GRAD_TOL and max(clips) <= GRAD_TOL, (tag, whole, clips)


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_input_grads.npz"))
    return {k: torch.from_numpy(g[k]) for k in g.files}


@pytest.fixture(scope="module")
def tiny_x():
    return torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).cuda()


@pytest.mark.parametrize("keep", [True, False])
def test_input_gradient_matches_reference_tiny(gold, tiny_x, keep):
    m = _model(keep=keep)
    x = tiny_x.clone().requires_grad_()
    logits = m(x)[0]
    assert (logits.detach().cpu() - gold["logits"]).abs().max() <= 1e-3 * gold["logits"].abs().max()
    (logits * gold["w_logits"].cuda()).sum().backward()
    _check_dx(f"TINY B=2 {'kept' if keep else 'recompute'} vs reference", x.grad, gold["dx"])
    assert m.visual.time_embed.grad is not None and m.prompt_learner.ctx.grad is not None      # the parameters got theirs as well


def _oracle_dx(cfg, x, wlog, tokens):
    p = {k: v.clone().float() for k, v in synth_torch_state(cfg, 3).items()}
    o = Oracle(cfg, p, tokens)
    xr = x.clone().float().requires_grad_()
    vf, _ = o.vision(xr)
    tf = o.text(o.prompts())
    logits = p["logit_scale"].exp() * (vf / vf.norm(dim=-1, keepdim=True)) @ (tf / tf.norm(dim=-1, keepdim=True)).t()
    (logits * wlog).sum().backward()
    return logits.detach(), xr.grad


@pytest.mark.parametrize("name,B", [("tiny_p14", 2), ("vit_b16", 1)])
def test_input_gradient_with_twice_the_frames_matches_oracle_autograd(name, B):
    """T_in = 2 * num_frames: the blocks regroup the frames by the model's num_frames, the embedding (and so the fold) is per input
    frame.  P = 14 at 56 px (588 patch columns in GEMM rows of 640) and ViT-B/16 at full size."""
    cfg = dataclasses.replace(TINY, input_size=56, patch_size=14) if name == "tiny_p14" else VIT_B16_T8
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    m = _model(cfg)
    x = torch.from_numpy(synth.synth_clip(B, 2 * cfg.num_frames, cfg.input_size, seed=13))
    wlog = torch.randn(B, 3, generator=torch.Generator().manual_seed(6))
    ref_logits, ref_dx = _oracle_dx(cfg, x, wlog, torch.cat(m.tokenized_prompts).cpu())
    xg = x.cuda().requires_grad_()
    logits = m(xg)[0]
    assert (logits.detach().cpu() - ref_logits).abs().max() <= 1e-3 * ref_logits.abs().max()
    (logits * wlog.cuda()).sum().backward()
    _check_dx(f"{name} B={B} T_in={2 * cfg.num_frames} vs oracle", xg.grad, ref_dx)


@pytest.mark.parametrize("keep", [True, False])
def test_asking_for_the_input_gradient_moves_nothing_else(tiny_x, keep):
    m = _model(keep=keep)
    w = torch.randn(2, 3, generator=torch.Generator().manual_seed(3)).cuda()

    def run(want_dx):
        _clear(m)
        x = tiny_x.clone().requires_grad_(want_dx)
        logits = m(x)[0]
        (logits * w).sum().backward()
        return logits.detach(), x.grad, {n: p.grad for n, p in m.named_parameters() if p.grad is not None}

    l0, dx0, g0 = run(False)
    l1, dx1, g1 = run(True)
    l2, dx2, _ = run(True)
    assert dx0 is None and dx1 is not None
    assert torch.equal(l0, l1) and torch.equal(l1, l2) and torch.equal(dx1, dx2)
    assert set(g0) == set(g1) and "visual.time_embed" in g0
    for n in g0:
        if ".summary_ln." in n:       # fp32 atomics: compared as the repeat test of tests/test_gpu_backward.py does
            assert rel(g1[n], g0[n]) <= 1e-5, n
        else:
            assert torch.equal(g1[n], g0[n]), n


def test_eval_mode_with_everything_frozen(gold, tiny_x):
    """How evaluation/evaluate.py and analysis_segment.py leave the model: eval(), no parameter trainable."""
    m = _model(train=False)
    for p in m.parameters():
        p.requires_grad_(False)
    x = tiny_x.clone().requires_grad_()
    logits = m(x)[0]
    assert logits.grad_fn is not None
    (logits * gold["w_logits"].cuda()).sum().backward()
    _check_dx("TINY B=2 eval(), all frozen, vs reference", x.grad, gold["dx"])
    assert all(p.grad is None for p in m.parameters())
    plain = m(tiny_x)[0]                                    # grad enabled, nothing asks for one: the inference path
    with torch.no_grad():
        inference = m(tiny_x)[0]
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, inference)
    assert (logits.detach() - inference).abs().max() <= 2e-3 * inference.abs().max()


@pytest.mark.parametrize("train", [True, False])
def test_saliency(tiny_x, train):
    m = _model(train=train)
    # reduce=None is x.grad of the plain route for the same targets
    xg = tiny_x.clone().requires_grad_()
    logits = m(xg)[0]
    target = logits.detach().argmax(1)
    logits.gather(1, target.view(-1, 1)).sum().backward()
    _clear(m)
    full, lg, tg = m.saliency(tiny_x, target=target, reduce=None)
    assert torch.equal(full, xg.grad) and torch.equal(lg, logits.detach()) and tg is target
    assert not lg.requires_grad and not full.requires_grad and tiny_x.grad is None and not tiny_x.requires_grad
    maps = {r: m.saliency(tiny_x, target=target, reduce=r)[0] for r in ("absmax", "l2", "grad_x_input")}
    assert all(v.shape == (2, TINY.num_frames, TINY.input_size, TINY.input_size) for v in maps.values())
    _check_maps(f"saliency maps train={train}", full, tiny_x, maps["absmax"], maps["l2"], maps["grad_x_input"])
    # target=None is the top-1 of this forward; an int is that class for every clip
    with torch.no_grad():                   # the call enables grad for itself
        auto, lg2, tg2 = m.saliency(tiny_x)
    assert torch.equal(tg2, lg2.argmax(1)) and tg2.dtype == torch.int64 and torch.equal(tg2, target) and torch.equal(auto, maps["absmax"])
    one, _, t1 = m.saliency(tiny_x, target=1, reduce=None)
    xg = tiny_x.clone().requires_grad_()
    m(xg)[0][:, 1].sum().backward()
    assert torch.equal(one, xg.grad) and t1.tolist() == [1, 1]
    _clear(m)
    # no parameter gradient, nothing kept
    del full, lg, tg, auto, lg2, tg2, one, t1, maps, xg, logits
    assert all(p.grad is None for p in m.parameters())
    # (the level is taken after a saliency call: the plain route above leaves model.text_features attached to its graph - 2 KB of
    # saved tensors that the next forward of either kind releases - which is not this call's to account for)
    m.saliency(tiny_x)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = m.saliency(tiny_x)
    assert all(p.grad is None for p in m.parameters())
    del out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


def test_saliency_adds_no_host_synchronisation(tiny_x):
    m = _model()
    target = torch.tensor([0, 2], device="cuda")

    def plain():
        _clear(m)
        m(tiny_x)[0].gather(1, target.view(-1, 1)).sum().backward()

    def count(fn):
        fn()                                        # warm-up: packs, workspaces, the side stream
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return len([w for w in caught if "synchroniz" in str(w.message).lower()])

    n_plain, n_sal, n_top1 = count(plain), count(lambda: m.saliency(tiny_x, target=target)), count(lambda: m.saliency(tiny_x))
    print(f"\n[input-grad-error] host synchronisations: forward + backward {n_plain}, saliency(target) {n_sal}, saliency(top-1) {n_top1}")
    assert n_sal <= n_plain and n_top1 <= n_plain


def test_refusals(tiny_x, tmp_path, monkeypatch):
    m = _model()
    with pytest.raises(hip.GavaError, match="fp32"):
        m(tiny_x.half().requires_grad_())
    with pytest.raises(hip.GavaError, match="HIP device"):
        m.saliency(tiny_x.cpu())
    for target in (3, -1):
        with pytest.raises(hip.GavaError, match="outside the 3 classes"):
            m.saliency(tiny_x, target=target)
    with pytest.raises(hip.GavaError, match="int64"):
        m.saliency(tiny_x, target=torch.tensor([0, 1], device="cuda", dtype=torch.int32))
    with pytest.raises(hip.GavaError, match="reduce"):
        m.saliency(tiny_x, reduce="sum")
    assert m(tiny_x.half())[0].requires_grad                  # an fp16 clip that asks for nothing trains as before
    # a per-descriptor head: a ragged number of prompts per class
    synth.synth_descriptor_files(str(tmp_path), "updrs", (2, 3, 1))
    monkeypatch.chdir(tmp_path)
    d = VitaCLIP(**{**model_kwargs(TINY, CLASSES_3), "text_prompt_init": "cntn_split_uni_disc", "knowledge_version": ["v1", "v2", "v3"],
                    "use_descriptor": True}).cuda().eval()
    with pytest.raises(hip.GavaError, match="per-descriptor"):
        d.saliency(tiny_x)
