"""loss.backward() through VitaCLIP.forward_frames: training from decoded uint8 videos, for the branch the reference trains with
(ClipPreprocessor, video_dataset/dataset.py:117-139) and for the random-sample branch (TrainClipPreprocessor, :93-114).

Every comparison is against the two-step route the parent commit offers, `model(pre.batch(videos))`, on the same videos and
the same draws.  Which patch-embedding kernel each route takes (csrc/forward.hip patch_operand, csrc/gemm.hip
gemm_patch_on_persistent):
  * uint8 source: always two passes - gava_patchify writes the 16-bit patch matrix, the GEMM reads it as an ordinary A operand;
  * fp32 clips: the same two passes when the persistent 256 x 256 kernel gets >= 512 tiles (D % 256 == 0 and
    ceil(B*T*n / 256) * D/256 >= 512: 28 clips at ViT-B/16, 8 frames), else the im2col-free GEMM with the in-loop fp32 loader.
Both routes feed the GEMM the same 16-bit operands (one rounding, one clip_pixel1 body); where they take the same kernel
everything downstream sees the same bits and logits and gradients are compared with torch.equal.  Two exceptions, by the
backward's own construction: summary_ln.weight / summary_ln.bias are reduced over rows with fp32 atomics
(csrc/backward.hip, dgamma / dbeta), whose order is not fixed from run to run even on one route - those, and every
comparison across different patch GEMMs (fp32 accumulation in another tile order), use the frozen constants of
tests/helpers.py: the mixed criterion on the logits, LOGITS_RTOL norm-wise on a gradient."""
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_preprocess_ref as ref
from helpers import CLASSES_3, LOGITS_RTOL, mixed_violation, model_kwargs, synth_torch_state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ATOMIC = ("summary_ln.weight", "summary_ln.bias")
SHAPES = [(11, 90, 130), (6, 120, 80), (9, 64, 64), (14, 70, 200), (20, 96, 96)]   # landscape, portrait, square; short and long


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _videos(B, seed=500):
    return [ref.video(*SHAPES[i % len(SHAPES)], seed + i).cuda() for i in range(B)]


def _pre(kind, cfg):
    from gava_clip_amd.preprocess import ClipPreprocessor, TrainClipPreprocessor
    cls = dict(eval=ClipPreprocessor, random=TrainClipPreprocessor)[kind]
    return cls(num_frames=cfg.num_frames, sampling_rate=2, spatial_size=cfg.input_size)


_MODELS = {}


def _model(cfg, name, **extra):
    """one model per config for the module (the ViT-B/16 synthetic weights take a while to build)"""
    from gava_clip_amd import VitaCLIP, synth
    if name not in _MODELS:
        _MODELS.clear()
        m = VitaCLIP(**model_kwargs(cfg, CLASSES_3), **extra)
        sd = synth_torch_state(cfg, 3)
        if extra:
            sd.update({k: torch.from_numpy(v) for k, v in synth.synth_aux_state(cfg, 3).items()})
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        _MODELS[name] = (m, m.keep_activation_bytes)
    m, keep_default = _MODELS[name]
    m.keep_activation_bytes = keep_default
    return m.train()


def _step(m, run, weights):
    """one forward + backward -> (outputs, {parameter: gradient})"""
    m.zero_grad(set_to_none=True)
    outs = [o for o in run() if o is not None]
    assert len(outs) == len(weights)
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _compare(got, want, same_kernel, what):
    (lg, gg), (lw, gw) = got, want
    assert set(gg) == set(gw) and len(gg) > 20
    worst = 0.0
    for a, b in zip(lg, lw):
        v = mixed_violation(a.cpu().numpy(), b.cpu().numpy())
        worst = max(worst, v)
        print(f"{what}: output {tuple(a.shape)} bitwise {torch.equal(a, b)} mixed violation {v:.3e}")
        assert torch.equal(a, b) if same_kernel else v <= 1.0, what
    n_exact, rel_worst = 0, 0.0
    for n in sorted(gg):
        a, b = gg[n], gw[n]
        assert torch.isfinite(a).all() and float(b.norm()) > 0, n
        if same_kernel and not n.endswith(ATOMIC):
            assert torch.equal(a, b), (what, n)
            n_exact += 1
        else:
            rel = float((a - b).norm() / b.norm())
            rel_worst = max(rel_worst, rel)
            assert rel <= LOGITS_RTOL, (what, n, rel)
    print(f"{what}: {len(gg)} gradients, {n_exact} bitwise equal, worst norm-wise difference of the others {rel_worst:.3e}")


def _both_routes(m, pre, vids, weights, seed, **kw):
    def frames():
        _seed(seed)
        return m.forward_frames(vids, pre, **kw)

    def two_step():
        _seed(seed)
        return m(pre.batch(vids), **kw)
    return _step(m, frames, weights), _step(m, two_step, weights)


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
@pytest.mark.parametrize("kind", ["eval", "random"])
def test_tiny_gradients_equal_the_two_step_route(kind, keep):
    """TINY (D = 128: never the persistent kernel), 3 videos of different sizes.  The two routes take different patch GEMMs
    (patch matrix + 128 x 128 tile GEMM vs the im2col-free 128 x 128 tile GEMM): frozen constants."""
    from gava_clip_amd.config import TINY
    m = _model(TINY, "tiny")
    if not keep:
        m.keep_activation_bytes = 0
    vids = _videos(3)
    w = [torch.randn(3, 3, generator=torch.Generator().manual_seed(7)).cuda()]
    got, want = _both_routes(m, _pre(kind, TINY), vids, w, seed=11)
    _compare(got, want, False, f"tiny/{kind}/{'kept' if keep else 'recompute'}")


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
def test_tiny_auxiliary_heads_train_through_frames(keep):
    """video_nte / memory on the tiny aux config (add_nte + use_support_memory): all three outputs and every gradient, the
    torch-side heads' included."""
    from gava_clip_amd import synth
    from gava_clip_amd.config import TINY
    m = _model(TINY, "tiny_aux", add_nte=True, use_support_memory=True, detach_features=False, num_classes=3)
    if not keep:
        m.keep_activation_bytes = 0
    B = 2
    vids = _videos(B)
    nte, mem = synth.synth_aux_inputs(B, TINY.embed_dim)
    kw = dict(memory=torch.from_numpy(mem).cuda(), video_nte=torch.from_numpy(nte).cuda())
    g = torch.Generator().manual_seed(8)
    w = [torch.randn(s, generator=g).cuda() for s in ((B, 3), (B, 3), (B, B))]      # logits, logits_mt, logits_vm
    for kind in ("eval", "random"):
        got, want = _both_routes(m, _pre(kind, TINY), vids, w, seed=12, **kw)
        assert len(got[0]) == 3
        _compare(got, want, False, f"tiny_aux/{kind}/{'kept' if keep else 'recompute'}")


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
@pytest.mark.parametrize("kind", ["eval", "random"])
@pytest.mark.parametrize("B", [2, 28])
def test_vit_b16_gradients_equal_the_two_step_route(B, kind, keep):
    """ViT-B/16, 8 frames, 3 classes (config c1's shapes).  B = 28: 224 frames x 196 patches = 172 row tiles x 3 column tiles
    = 516 >= 512, so the fp32 clips take the two-pass patch embedding too - gava_patchify + the persistent 256 x 256 GEMM on
    both routes: bit for bit.  B = 2 (c1's own batch): the fp32 clips take the im2col-free 128 x 256 tile GEMM, the uint8
    source the patch matrix + 128 x 128 tile GEMM: frozen constants."""
    from gava_clip_amd.config import VIT_B16_T8
    cfg = VIT_B16_T8
    n = (cfg.input_size // cfg.patch_size) ** 2
    same_kernel = cfg.feature_dim % 256 == 0 and -(-B * cfg.num_frames * n // 256) * (cfg.feature_dim // 256) >= 512
    assert same_kernel == (B == 28)
    m = _model(cfg, "b16")
    if not keep:
        m.keep_activation_bytes = 0
    vids = _videos(B)
    w = [torch.randn(B, 3, generator=torch.Generator().manual_seed(9)).cuda()]
    got, want = _both_routes(m, _pre(kind, cfg), vids, w, seed=13)
    _compare(got, want, same_kernel, f"b16/B{B}/{kind}/{'kept' if keep else 'recompute'}")


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "recompute"])
def test_videos_may_be_released_before_backward(keep):
    """The backward never re-reads the input (forward_frames' docstring): drop every reference to the videos after the
    forward, let other tensors take their memory, then backward() - the gradients of the run that kept them alive."""
    from gava_clip_amd.config import TINY
    m = _model(TINY, "tiny")
    if not keep:
        m.keep_activation_bytes = 0
    pre = _pre("random", TINY)
    w = torch.randn(3, 3, generator=torch.Generator().manual_seed(7)).cuda()

    def run(release):
        m.zero_grad(set_to_none=True)
        vids = _videos(3)
        sizes = [v.shape for v in vids]
        _seed(21)
        logits = m.forward_frames(vids, pre)[0]
        loss = (logits * w).sum()
        junk = None
        if release:
            del vids
            junk = [torch.full(tuple(s), 255, dtype=torch.uint8, device="cuda") for s in sizes]   # reuses the freed blocks
        loss.backward()
        torch.cuda.synchronize()
        del junk
        return logits.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    (la, ga), (lb, gb) = run(True), run(False)
    assert torch.equal(la, lb) and set(ga) == set(gb) and len(ga) > 20
    for n in ga:
        if n.endswith(ATOMIC):
            assert float((ga[n] - gb[n]).norm() / gb[n].norm()) <= LOGITS_RTOL, n
        else:
            assert torch.equal(ga[n], gb[n]), n


def test_eval_mode_still_needs_no_grad():
    """Training goes through train() mode; a model in eval() mode with grad enabled is still refused (the evaluation path with
    a forgotten torch.no_grad()), and under no_grad both preprocessors give forward()'s logits."""
    from gava_clip_amd import hip
    from gava_clip_amd.config import TINY
    m = _model(TINY, "tiny").eval()
    vids = _videos(2)
    for kind in ("eval", "random"):
        pre = _pre(kind, TINY)
        with pytest.raises(hip.GavaError):
            m.forward_frames(vids, pre)
        with torch.no_grad():
            _seed(3)
            a = m.forward_frames(vids, pre)[0]
            _seed(3)
            b = m(pre.batch(vids))[0]
        assert torch.equal(a, b)
    m.train()


def test_ddp_gradients_through_frames_equal_single_process(tmp_path):
    """2 gloo ranks sharing cuda:0 under DistributedDataParallel, each with its own decoded videos: averaged gradients ==
    single-process gradients through forward_frames on all videos, to the bound tests/test_distributed.py holds forward() to
    (2e-2 norm-wise: the backward's own accuracy, partial sums over another number of frames per process)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker_frames.py"), "ddp_frames_gpu", str(r), "2", str(port),
                               str(tmp_path)], env=env) for r in range(2)]
    try:
        codes = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:          # only the exact children this test started
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0]
    for r in range(2):
        worst, n = np.load(tmp_path / f"ddpframes{r}.npy")
        print(f"rank {r}: {int(n)} gradients, worst norm-wise difference {worst:.3e}")
        assert n > 20 and worst <= 2e-2, (worst, n)
