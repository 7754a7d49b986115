"""Shapes past the 320-key class of the single-pass attention kernels (long clips, 336/384 px inputs): the vision
drivers accept them (the key-streaming kernels take their attention), and the attention backward's scratch covers them.
Host only: no GPU needed."""
import ctypes as C

import pytest

from gava_clip_amd import hip
from gava_clip_amd.config import TINY_T320, TINY_320PX, VitaConfig

# (input size, patch, frames T, width, heads, layers): keys per frame = (size / patch)^2 + 1 + G + T + 1
LONG_SHAPES = {
    "vit_l14_t64": (224, 14, 64, 1024, 16, 24),     # 330 keys, 257 queries
    "vit_l14_t70": (224, 14, 70, 1024, 16, 24),     # 336 keys (the UPDRS training recipe's 70 frames)
    "vit_b16_t128": (224, 16, 128, 768, 12, 12),    # 334 keys, 197 queries
    "vit_l14_336px": (336, 14, 8, 1024, 16, 24),    # 594 keys, 577 queries
    "vit_b16_384px": (384, 16, 8, 768, 12, 12),     # 594 keys, 577 queries
}


def _model(size, P, T, D, H, layers, B=2, G=8):
    m = hip.VisionModel()
    m.B, m.T_in, m.T_model, m.size, m.P, m.D, m.H, m.layers = B, T, T, size, P, D, H, layers
    m.F, m.E, m.G, m.prec = 4 * D, 768 if D == 1024 else 512, G, hip.PREC_F16
    layer = (hip.VisionLayer * layers)()
    m.layer = C.cast(layer, C.POINTER(hip.VisionLayer))
    return m, layer


@pytest.mark.parametrize("name", sorted(LONG_SHAPES))
def test_vision_workspace_covers_long_shapes(name):
    size, P, T, D, H, layers = LONG_SHAPES[name]
    m, _keep = _model(size, P, T, D, H, layers)
    lib = hip.load()
    nbytes = lib.gava_vision_workspace_bytes(C.byref(m))
    assert nbytes > 0, name
    # the workspace grows with the rows: one more clip needs more
    m.B = 3
    assert lib.gava_vision_workspace_bytes(C.byref(m)) > nbytes


@pytest.mark.parametrize("cfg", [TINY_T320, TINY_320PX], ids=["tiny_t320", "tiny_320px"])
def test_tiny_long_fixture_shapes_are_accepted(cfg: VitaConfig):
    assert cfg.attn_keys() > 320
    m, _keep = _model(cfg.input_size, cfg.patch_size, cfg.num_frames, cfg.feature_dim, cfg.num_heads, cfg.num_layers,
                      G=cfg.num_global_prompts)
    m.E = cfg.embed_dim
    assert hip.load().gava_vision_workspace_bytes(C.byref(m)) > 0


@pytest.mark.parametrize("batch,heads,n_q", [(16, 16, 577), (128, 12, 197), (4, 2, 401), (2, 2, 320), (7, 3, 1001)])
def test_attention_backward_workspace_covers_long_query_sets(batch, heads, n_q):
    """The streaming dQ kernel writes, per (frame, head), two floats (log2-sum-exp, delta) for each query row < n_q at row
    stride q_pad = query tiles rounded up to pairs; the dK/dV kernels read the same rows."""
    lib = hip.load()
    lib.gava_attention_backward_workspace_bytes.restype = C.c_size_t
    q_pad = ((n_q + 15) // 16 + 1) // 2 * 32
    need = batch * heads * q_pad * 2 * 4
    assert q_pad >= n_q
    assert lib.gava_attention_backward_workspace_bytes(batch, heads, n_q) >= need
