"""CPU: the host side of the gradient with respect to the input clip (gava_unpatchify, hip.unpatchify, VitaCLIP.saliency).

The torch restatement of the fold (tests/input_grad_ref.py) is pinned to autograd in fp64: for a Conv2d(3, D, P, stride=P) the fold
of dE @ W.view(D, -1) is x.grad, to 1e-12 relative (the same products, summed in another order).  The oracle under autograd is
pinned to the REFERENCE's d logits / d x (tests/golden/tiny_input_grads.npz, tools/gen_golden_input_grad.py) with the figures that pin
its parameter gradients (tests/test_oracle_golden.py): logits 2e-5, gradient 2e-4.  Plus the C ABI's surface (names, the struct
mirror, the argument checks that return before any launch) and the Python refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gava_clip_amd import synth
from gava_clip_amd.config import TINY
from oracle.vita_oracle import Oracle
from helpers import REPO, synth_torch_state, rel_to_max
import input_grad_ref as ref

NAMES = ("gava_unpatchify", "gava_input_grad_struct_sizes")


@pytest.mark.parametrize("B,T,size,P", [(2, 3, 64, 16), (1, 2, 28, 14)])
def test_restated_fold_is_the_conv_input_gradient(B, T, size, P):
    D, n = 24, (size // P) ** 2
    gen = torch.Generator().manual_seed(size + P)
    conv = torch.nn.Conv2d(3, D, P, stride=P).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen, dtype=torch.float64))
    x = torch.randn(B, 3, T, size, size, generator=gen, dtype=torch.float64, requires_grad=True)
    # ImagePatchEmbed2D (VitaCLIP_vision_encoder_utils.py:31-53): the conv over every frame, patch rows in (b, t, py, px) order
    frames = x.permute(0, 2, 1, 3, 4).reshape(B * T, 3, size, size)
    E = conv(frames).flatten(2).transpose(1, 2)                       # [B*T, n, D]
    dE = torch.randn(B * T, n, D, generator=gen, dtype=torch.float64)
    (E * dE).sum().backward()
    dpatch = dE.reshape(B * T * n, D) @ conv.weight.detach().view(D, -1)
    got = ref.fold(dpatch, B, T, size, P, n, 0)
    assert got.shape == x.shape
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    # the model's form: a CLS row in front of every frame's patch rows and padding columns behind them, both skipped
    padded = torch.full((B * T, n + 1, 3 * P * P + 9), float("nan"), dtype=torch.float64)
    padded[:, 1:, :3 * P * P] = dpatch.view(B * T, n, -1)
    assert torch.equal(ref.fold(padded, B, T, size, P, n + 1, 1), got)


def test_restated_maps():
    g = torch.tensor([[3.0, -4.0], [0.5, 2.0], [-12.0, 1.0]]).view(1, 3, 1, 1, 2)
    x = torch.tensor([[1.0, 2.0], [-2.0, 0.5], [0.25, 4.0]]).view(1, 3, 1, 1, 2)
    assert ref.reduce_map(g, ref.ABSMAX).flatten().tolist() == [12.0, 4.0]
    assert torch.allclose(ref.reduce_map(g, ref.L2).flatten(), torch.tensor([153.25 ** 0.5, 21.0 ** 0.5]))
    assert ref.reduce_map(g, ref.GRAD_X_INPUT, x).flatten().tolist() == [3.0 - 1.0 - 3.0, -8.0 + 1.0 + 4.0]


def test_oracle_input_gradient_matches_reference_tiny(golden_dir):
    """The oracle under torch autograd with x.requires_grad_() against the REFERENCE's own x.grad: pins the checker of the HIP route."""
    g = np.load(os.path.join(golden_dir, "tiny_input_grads.npz"))
    assert os.path.getsize(os.path.join(golden_dir, "tiny_input_grads.npz")) < 1 << 20
    p = {k: v.clone().float() for k, v in synth_torch_state(TINY, 3).items()}
    o = Oracle(TINY, p, torch.from_numpy(np.load(os.path.join(golden_dir, "tiny.npz"))["tokens"]))
    x = torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).requires_grad_()
    vf, _ = o.vision(x)
    tf = o.text(o.prompts())
    logits = p["logit_scale"].exp() * (vf / vf.norm(dim=-1, keepdim=True)) @ (tf / tf.norm(dim=-1, keepdim=True)).t()
    assert rel_to_max(logits.detach().numpy(), g["logits"]) <= 2e-5
    (logits * torch.from_numpy(g["w_logits"])).sum().backward()
    assert x.grad.shape == g["dx"].shape
    err = float(np.linalg.norm((x.grad.numpy() - g["dx"]).astype(np.float64)) / np.linalg.norm(g["dx"].astype(np.float64)))
    assert err <= 2e-4, err


def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    from gava_clip_amd.build import SOURCES
    assert "input_grad.hip" in SOURCES
    for name, value in (("GRAD", 0), ("ABSMAX", 1), ("L2", 2), ("GRAD_X_INPUT", 3)):
        assert re.search(rf"#define GAVA_UNPATCH_{name} {value}\b", header) and getattr(hip, "UNPATCH_" + name) == value == getattr(ref, name)


def test_struct_matches_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirror == what the library reports (gava_input_grad_struct_sizes)."""
    import __graft_entry__ as ge
    ge.build()
    from gava_clip_amd import hip
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){printf("%zu\\n", sizeof(gava_unpatchify_args));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    size = int(subprocess.check_output([str(tmp_path / "s")]).decode())
    lib = hip.load()
    got = (ctypes.c_size_t * 1)()
    assert lib.gava_input_grad_struct_sizes(got, 1) == 1
    assert ctypes.sizeof(hip.UnpatchifyArgs) == size == got[0]
    assert lib.gava_input_grad_struct_sizes(None, 0) == 1          # a zero capacity writes nothing


ONE = 64      # a non-null, 16-byte aligned stand-in for a device pointer: every call below returns before it is used


def _args(hip, **kw):
    """A valid call of the model's form (ViT-L/14 at 28 px: 588 columns in rows of 640, the CLS row skipped)."""
    a = hip.UnpatchifyArgs()
    a.dpatch, a.ld, a.out = ONE, 640, ONE
    a.B, a.T, a.size, a.patch, a.mode, a.frame_rows, a.row_offset = 2, 3, 28, 14, hip.UNPATCH_ABSMAX, 5, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_unpatchify_refuses_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    call = lambda **kw: lib.gava_unpatchify(ctypes.byref(_args(hip, **kw)), None)
    assert lib.gava_unpatchify(None, None) == -1
    assert call(dpatch=None) == -1 and call(out=None) == -1                                    # null pointers
    assert call(dpatch=ONE + 4) == -1 and call(out=ONE + 8) == -1                              # misaligned pointers
    assert call(mode=hip.UNPATCH_GRAD_X_INPUT, x=ONE + 4) == -1
    assert call(size=30) == -1                                                                 # size % P != 0
    assert call(ld=587) == -1                                                                  # ld < 3 P^2
    assert call(frame_rows=4) == -1 and call(row_offset=2) == -1 and call(row_offset=-1) == -1   # row_offset + n > frame_rows
    assert call(mode=4) == -1 and call(mode=-1) == -1                                          # unknown mode
    assert call(mode=hip.UNPATCH_GRAD_X_INPUT) == -1                                           # x missing in its mode
    for mode in (hip.UNPATCH_GRAD, hip.UNPATCH_ABSMAX, hip.UNPATCH_L2):
        assert call(mode=mode, x=ONE) == -1, mode                                              # x given in another mode
    for field in ("B", "T", "size", "patch"):                                                  # B * T * n == 0
        assert call(**{field: 0}) == -1 and call(**{field: -1}) == -1, field
    assert call(B=65536, T=32768) == -1                                                        # B * T past 2^31 - 1


def test_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    kw = dict(B=2, T=3, size=28, patch=14, mode=hip.UNPATCH_ABSMAX, frame_rows=5, row_offset=1)
    dp, out, clip = f(30, 640), f(2, 3, 28, 28), f(2, 3, 3, 28, 28)
    with pytest.raises(E, match="HIP device"):
        hip.unpatchify(dp, out, **kw)                                              # CPU tensors: everything else about them is right
    with pytest.raises(E, match="HIP device"):
        hip.unpatchify(dp, clip, **{**kw, "mode": hip.UNPATCH_GRAD})
    with pytest.raises(E, match="fp32"):
        hip.unpatchify(dp.double(), out, **kw)
    with pytest.raises(E, match="fp32"):
        hip.unpatchify(dp, out.half(), **kw)
    with pytest.raises(E, match="contiguous"):
        hip.unpatchify(f(640, 30).t(), out, **kw)
    with pytest.raises(E, match="contiguous"):
        hip.unpatchify(dp, f(2, 3, 28, 56)[..., ::2], **kw)
    with pytest.raises(E, match="frames of"):
        hip.unpatchify(f(29, 640), out, **kw)                                      # not B*T*frame_rows rows
    with pytest.raises(E, match="frames of"):
        hip.unpatchify(f(5, 6, 640), out, **kw)                                    # 3-D, but not [B*T, frame_rows, ld]
    with pytest.raises(E, match="patch columns"):
        hip.unpatchify(f(30, 584), out, **kw)
    with pytest.raises(E, match="of a frame of"):
        hip.unpatchify(f(24, 640), out, **{**kw, "frame_rows": 4})
    with pytest.raises(E, match="this mode writes"):
        hip.unpatchify(dp, clip, **kw)                                             # the gradient's shape for a map mode
    with pytest.raises(E, match="this mode writes"):
        hip.unpatchify(dp, out, **{**kw, "mode": hip.UNPATCH_GRAD})
    with pytest.raises(E, match="UNPATCH_GRAD_X_INPUT"):
        hip.unpatchify(dp, out, **{**kw, "mode": hip.UNPATCH_GRAD_X_INPUT})        # x missing
    with pytest.raises(E, match="UNPATCH_GRAD_X_INPUT"):
        hip.unpatchify(dp, out, x=clip, **kw)                                      # x given to another mode
    with pytest.raises(E, match="x is"):
        hip.unpatchify(dp, out, x=f(2, 3, 3, 28, 14), **{**kw, "mode": hip.UNPATCH_GRAD_X_INPUT})
    with pytest.raises(E, match="unknown mode"):
        hip.unpatchify(dp, out, **{**kw, "mode": 7})
    with pytest.raises(E, match="size=30"):
        hip.unpatchify(dp, out, **{**kw, "size": 30})


def test_saliency_refusals_without_a_device():
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.hip import GavaError
    from helpers import CLASSES_3, model_kwargs
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3)).eval()
    x = torch.zeros(1, 3, TINY.num_frames, TINY.input_size, TINY.input_size)
    with pytest.raises(GavaError, match="HIP device"):
        m.saliency(x)
    with pytest.raises(GavaError, match="reduce"):
        m.saliency(x, reduce="max")
