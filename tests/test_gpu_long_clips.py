"""VitaCLIP at shapes past the 320-key class of the single-pass attention kernels (key-streaming kernels): long clips and
high-resolution inputs, forward / forward_frames / one training step against the reference's fixtures
(tools/gen_golden.py --long), and full-width ViT-L/14 at T = 64 and ViT-B/16 at T = 128 against the fp32 oracle."""
import os

import numpy as np
import pytest
import torch

from gava_clip_amd import VitaCLIP, synth
from gava_clip_amd.config import TINY_T320, TINY_320PX, VIT_L14_T64, VIT_B16_T128
from gava_clip_amd.preprocess import ClipPreprocessor
from helpers import CLASSES_3, model_kwargs, synth_torch_state, rel_to_max, mixed_violation

pytestmark = pytest.mark.gpu

LONG = {"tiny_t320": TINY_T320, "tiny_320px": TINY_320PX}


def _model(cfg, train=False):
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(synth_torch_state(cfg, 3, 0), strict=True)
    m = m.cuda()
    return m.train() if train else m.eval()


@pytest.mark.parametrize("name", sorted(LONG))
def test_long_shape_forward_matches_reference(golden_dir, name):
    cfg = LONG[name]
    assert cfg.attn_keys() > 320
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    m = _model(cfg)
    x = torch.from_numpy(synth.synth_clip(2, cfg.num_frames, cfg.input_size, seed=int(g["xseed"]))).cuda()
    with torch.no_grad():
        logits, lmt, lvm = m(x)
    assert lmt is None and lvm is None
    lg = logits.float().cpu().numpy()
    e_rel, viol = rel_to_max(lg, g["logits"]), mixed_violation(lg, g["logits"])
    ev = rel_to_max(m.last["video_features"].cpu().numpy(), g["video_features"])
    et = rel_to_max(m.text_features.cpu().numpy(), g["text_features"])
    es = rel_to_max(m.last["summary"].cpu().numpy(), g["summary"])
    print(f"\n[{name}] logits rel-to-max {e_rel:.2e} mixed {viol:.3f} video {ev:.2e} text {et:.2e} summary {es:.2e}")
    assert e_rel < 1e-3 and viol <= 1.0 and ev < 1e-3 and et < 1e-3
    assert es < 3e-3


@pytest.mark.parametrize("name", sorted(LONG))
def test_long_shape_forward_frames_equals_forward(name):
    """The decoded-video path at the long shapes: bit for bit the forward of the preprocessed batch."""
    cfg = LONG[name]
    m = _model(cfg)
    gen = torch.Generator().manual_seed(7)
    n_frames = cfg.num_frames + 9
    vids = [torch.randint(0, 256, (n_frames, cfg.input_size + 6, cfg.input_size + 26, 3), dtype=torch.uint8, generator=gen).cuda(),
            torch.randint(0, 256, (n_frames - 5, cfg.input_size, cfg.input_size, 3), dtype=torch.uint8, generator=gen).cuda()]
    pre = ClipPreprocessor(num_frames=cfg.num_frames, sampling_rate=1, spatial_size=cfg.input_size,
                           mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225))
    with torch.no_grad():
        a, b = m.forward_frames(vids, pre)[0], m(pre.batch(vids))[0]
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(LONG))
def test_long_shape_gradients_match_reference(golden_dir, name):
    """loss.backward() through the streaming attention backward: every trainable parameter's gradient against the
    reference under torch autograd, norm-wise within 4e-2 (the bound of the existing gradient fixtures)."""
    cfg = LONG[name]
    gold = np.load(os.path.join(golden_dir, name + "_grads.npz"))
    m = _model(cfg, train=True)
    x = torch.from_numpy(synth.synth_clip(2, cfg.num_frames, cfg.input_size, seed=1234)).cuda()
    logits, lmt, lvm = m(x)
    assert lmt is None and lvm is None
    assert (logits.detach().cpu() - torch.from_numpy(gold["logits"])).abs().max() <= 1e-3 * np.abs(gold["logits"]).max()
    (logits * torch.from_numpy(gold["w_logits"]).cuda()).sum().backward()
    got = dict(m.named_parameters())
    names = [k.split(".", 1)[1] for k in gold.files if k.startswith("grad.")]
    assert len(names) > 20
    worst = {}
    for pname in names:
        g, ref = got[pname].grad, torch.from_numpy(gold["grad." + pname])
        assert g is not None and g.shape == ref.shape, pname
        if pname.endswith("k_proj.bias") and "summary" in pname:   # exactly zero in exact arithmetic (softmax shift)
            q_n = torch.from_numpy(gold["grad." + pname.replace("k_proj", "q_proj")]).norm()
            assert float(g.norm()) <= 0.2 * float(q_n) and float(ref.norm()) <= 1e-4 * float(q_n)
            continue
        worst[pname] = float((g.float().cpu() - ref).norm() / ref.norm())
    top = max(worst, key=worst.get)
    print(f"\n[{name}] worst gradient {top}: {worst[top]:.2e}")
    assert worst[top] < 4e-2, (top, worst[top])


@pytest.mark.parametrize("cfg", [VIT_L14_T64, VIT_B16_T128], ids=["vit_l14_t64", "vit_b16_t128"])
def test_full_width_long_clips_against_oracle(cfg):
    """Full-width backbones past 320 keys: two clips finite, clip 0 against the fp32 oracle (fixture criteria)."""
    from oracle.vita_oracle import Oracle
    sd = synth_torch_state(cfg, 3, 0)
    m = VitaCLIP(**model_kwargs(cfg, CLASSES_3))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(synth.synth_clip(2, cfg.num_frames, cfg.input_size, seed=11))
    with torch.no_grad():
        lg = m(x.cuda())[0].float().cpu().numpy()
    assert np.isfinite(lg).all()
    torch.set_num_threads(16)
    with torch.no_grad():
        want = Oracle(cfg, sd, torch.cat(m.tokenized_prompts).cpu()).forward(x[:1])["logits"].numpy()
    e_rel, viol = rel_to_max(lg[:1], want), mixed_violation(lg[:1], want)
    print(f"\n[{cfg.num_frames} frames, D = {cfg.feature_dim}] clip 0 vs oracle: rel-to-max {e_rel:.2e} mixed {viol:.3f}")
    assert e_rel < 1e-3 and viol <= 1.0
