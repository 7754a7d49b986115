"""`loss.backward()` of the trainable subset through the HIP kernels.

The reference trains `prompt_learner.ctx` (CoOp context vectors), the vision prompts and `logit_scale` with every
transformer weight frozen (VitaCLIP_model.py:230-239; training/train.py:441-490 calls `loss.backward()`).  The
gradient therefore only has to flow THROUGH the frozen GEMMs.  Gradient operands are bf16 (fp32 exponent range, so no
loss scaling inside the library; the reference's fp16 autocast needs its GradScaler), accumulation fp32.

Both towers are stacks of one residual block and share its two stages and the layout of its packed weights:
    _block_weights     bf16 copies of the frozen weights in both orientations (forward for the recompute, transposed for dgrad)
    _block_recompute   a block's activations from its saved fp32 input: the six forward launches
    _block_backward    MLP' and attention' (dgrad GEMMs, fused QuickGELU', LayerNorm', gava_attention_backward); LN1' is the caller's
Text (`TextTowerFn`; `gava_text_forward_train` keeps the fp32 input of every block), `text_backward`:
    d text features -> text_projection^T -> ln_final' (EOT rows) -> 12 x (recompute, backward, LN1') -> d ctx
Vision (`VisionTowerFn`; the forward keeps the blocks' activations or, above `keep_activation_bytes`, their fp32 inputs).
Trainable (VitaCLIP_model.py:230-234: names containing summary / local / global / time_embed): visual.global_prompts
(layers,G,D), visual.time_embed (T,D) and per block local_prompts (1,T,D), summary_ln.{weight,bias},
summary_attn_layer.{q,k,v,out}_proj.{weight,bias}.  `vision_backward` runs VitaCLIP_vision_encoder.py:102-132 and
VitaCLIP_vision_encoder_utils.py:155-203 in reverse as a list of stages, on scratch that lives for the one call:
    _head_backward       mean over T, proj^T, ln_post' on the CLS rows
    per block: _prompt_recompute   cls_proj, summary_ln, summary attention, the prompt rows SIDE every frame attends to
               _main_activations   SIDE's K/V and the main rows' qkv / X1 / pre: what the forward kept, or _block_recompute
               _block_backward     on all B*T*197 rows, or _cls_only_backward for a kept last block
               _prompt_backward    d SIDE -> d global / local prompts and, through the summary path, the gradients of
                                   summary_ln / summary_attn_layer (wgrad = gava_gemm on transposed operands) and the CLS rows' share
               LN1' of the main rows
    _embedding_backward  ln_pre', sum over tokens = d time_embed
    _input_backward      only when d x is asked for: patch projection^T (dgrad GEMM), then the fold of the patch rows back into
                         the clip (gava_unpatchify) - the gradient itself, or a saliency map of it without the gradient in memory;
                         with a path request (VitaCLIP.integrated_gradients / smooth_grad) the fold also reduces the m copies of
                         every clip to one map (gava_unpatchify_path)
    _relevance_step      only with a relevance request (VitaCLIP.relevance_maps): per block, right after its d mix exists, one step of
                         the gradient-weighted attention relevance chain (gava_attention_relevance); the backward ends after block 0's
The second half of the module is the step's tail: similarity head and criterion on the device.
"""
import ctypes as C
from types import SimpleNamespace

import torch

from . import hip

BWD = hip.PREC_BF16


def f32(p):
    return p.detach().float().contiguous()


def new(dev, *shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device=dev)


def split3(t):
    """[rows][3W] -> its q, k, v column blocks."""
    W = t.shape[1] // 3
    return t[:, :W], t[:, W:2 * W], t[:, 2 * W:]


def _bf16(t):
    return hip.convert_h16(f32(t), BWD)


def _both(w):
    """Weight [out][in] -> (bf16 copy for the recompute, bf16 copy of its transpose for dgrad)."""
    return _bf16(w), _bf16(w.detach().t())


def _block_weights(w_qkv, b_qkv, out_proj, fc1, fc2):
    """The pack entries every transformer block has, under the same names in both towers."""
    P = dict(b_qkv=f32(b_qkv), b_out=f32(out_proj.bias), b_fc1=f32(fc1.bias), w_fc2_t=_bf16(fc2.weight.detach().t()))
    P["w_qkv"], P["w_qkv_t"] = _both(w_qkv)
    P["w_out"], P["w_out_t"] = _both(out_proj.weight)
    P["w_fc1"], P["w_fc1_t"] = _both(fc1.weight)
    return P


def _block_scratch(dev, R, W, F, recompute=False):
    """Scratch of the block stages for R rows of width W, allocated once per backward call."""
    s = SimpleNamespace(dx16=new(dev, R, W), dhid=new(dev, R, F), dmix=new(dev, R, W), dqkv=new(dev, R, 3 * W),
                        dxn=new(dev, R, W, dtype=torch.float32))
    if recompute:
        s.xn, s.qkv, s.mix, s.pre, s.X1 = new(dev, R, W), new(dev, R, 3 * W), new(dev, R, W), new(dev, R, F), new(dev, R, W, dtype=torch.float32)
    return s


def _block_recompute(P, ln, X0, s, **attn):
    """Recompute a block from its fp32 input X0 with the forward kernels (bf16 operands): fills s.qkv, s.X1 (the stream
    after the attention branch) and s.pre (the fc1 pre-activation).  ln = (ln1 weight, ln1 bias, ln2 weight, ln2 bias);
    `attn` are the tower's keyword arguments of hip.attention."""
    W = X0.shape[1]
    hip.layernorm(X0, ln[0], ln[1], out16=s.xn, prec=BWD)
    hip.gemm(s.xn, P["w_qkv"], P["b_qkv"], s.qkv, epilogue=hip.EPI_H16, prec=BWD, scale_cols=W, scale=0.125)
    hip.attention(*split3(s.qkv), s.mix, prec=BWD, **attn)
    hip.gemm(s.mix, P["w_out"], P["b_out"], s.X1, epilogue=hip.EPI_F32, prec=BWD, resid=X0)
    hip.layernorm(s.X1, ln[2], ln[3], out16=s.xn, prec=BWD)
    hip.gemm(s.xn, P["w_fc1"], P["b_fc1"], s.pre, epilogue=hip.EPI_H16, prec=BWD)


def _mlp_backward(P, ln2_g, dX, s, X1, pre, act):
    """MLP branch x2 = x1 + fc2(gelu(fc1(ln_2 x1))) (VitaCLIP_text_encoder.py:73-77,86; vision_encoder_utils.py:109-115,199):
    dX (fp32; s.dx16 = its bf16 copy, written by the LayerNorm' that produced it) takes the branch's share, then out_proj^T
    -> s.dmix.  `act`: storage type of the kept activations (None: the gradients' bf16)."""
    hip.gemm(s.dx16, P["w_fc2_t"], None, s.dhid, epilogue=hip.EPI_H16_QGELU_BWD, prec=BWD, aux=pre, aux_prec=act)   # fc2^T, gelu' fused
    hip.gemm(s.dhid, P["w_fc1_t"], None, s.dxn, epilogue=hip.EPI_F32, prec=BWD)
    hip.layernorm_backward(X1, ln2_g, s.dxn, dX, accumulate=True, dx16=s.dx16)
    hip.gemm(s.dx16, P["w_out_t"], None, s.dmix, epilogue=hip.EPI_H16, prec=BWD)


def _block_backward(P, ln2_g, dX, s, X1, pre, qkv, act, rel=None, **attn):
    """MLP' and attention' of a block on all its rows; s.dxn is left holding the input of LN1' for the caller.  Attention
    branch: x1 = x0 + out_proj(attn(in_proj(ln_1 x0))) (VitaCLIP_text_encoder.py:81-85; vision_encoder_utils.py:61-81,190-191);
    `attn` are the tower's keyword arguments of hip.attention_backward.  rel (vision, relevance request only): called with the
    block's queries and s.dmix as soon as that exists; a true result (-> True) ends the block there."""
    _mlp_backward(P, ln2_g, dX, s, X1, pre, act)
    if rel is not None and rel(split3(qkv)[0], s.dmix):
        return True
    hip.attention_backward(*split3(qkv), s.dmix, *split3(s.dqkv), prec=BWD, q_scale=0.125, act_prec=act, **attn)
    hip.gemm(s.dqkv, P["w_qkv_t"], None, s.dxn, epilogue=hip.EPI_F32, prec=BWD)


# ---- text tower: gradient of the context vectors ------------------------------------------------

def pack_text_backward(model):
    """bf16 copies of the frozen text weights in both orientations (forward for the recompute, transposed for dgrad)."""
    t = model.textual
    layers = [dict(_block_weights(blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj, blk.mlp.c_fc, blk.mlp.c_proj),
                   ln=(f32(blk.ln_1.weight), f32(blk.ln_1.bias), f32(blk.ln_2.weight), f32(blk.ln_2.bias)))
              for blk in t.transformer.resblocks]
    return dict(layers=layers, lnf_g=f32(t.ln_final.weight),
                # out = x @ text_projection (W,E): dx = dout @ text_projection^T = gemm(A = dout, W = text_projection)
                w_tproj=_bf16(t.text_projection))


def text_forward_train(model, ctx_param):
    """-> (text features (C,E) fp32, saved block inputs fp32 [layers+1, C*L, W])."""
    lib = hip.load()
    pk, sh = model._pack(), model._shape
    tok = pk["tokens"]
    n = tok.shape[0]
    m = hip.TextModel()
    m.n_prompts, m.L, m.W, m.H, m.layers = n, model.text_rows_per_prompt, sh["W"], sh["TH"], sh["TL"]
    m.E, m.n_ctx, m.prec = sh["E"], sh["n_ctx"], model.prec
    m.split = int(model.text_split_precision)
    for k, val in pk["txt"].items():
        setattr(m, k, val)
    m.layer = C.cast(pk["txt_layers"], C.POINTER(hip.TextLayer))
    nbytes = lib.gava_text_workspace_bytes(C.byref(m))
    if nbytes == 0:
        raise hip.GavaError(f"unsupported text shape: {sh}")
    ws = model._workspace("text", nbytes, tok.device)
    ctx = ctx_param.detach().float().contiguous()
    out = torch.empty(n, sh["E"], dtype=torch.float32, device=tok.device)
    saved = torch.empty(sh["TL"] + 1, n * model.text_rows_per_prompt, sh["W"], dtype=torch.float32, device=tok.device)
    hip.check(lib.gava_text_forward_train(C.byref(m), hip.ptr(tok), hip.ptr(ctx), hip.ptr(pk["eot"]), hip.ptr(out),
                                          hip.ptr(saved), hip.ptr(ws), ws.numel(), hip.stream_ptr()),
              "gava_text_forward_train")
    return out, saved


def text_backward(model, saved, dtext):
    """d(text features) (C,E) -> d ctx (C, n_ctx, W), through the frozen text tower."""
    sh = model._shape
    pk, bw = model._pack(), model._backward_pack("text")
    n, L, W, H, n_ctx = pk["tokens"].shape[0], model.text_rows_per_prompt, sh["W"], sh["TH"], sh["n_ctx"]
    R, dev, eot = n * L, dtext.device, pk["eot"]
    dX = torch.zeros(R, W, dtype=torch.float32, device=dev)
    # text_projection^T and ln_final' on the EOT rows (VitaCLIP_text_encoder.py:164-170)
    dEOT = new(dev, n, W, dtype=torch.float32)
    hip.gemm(hip.convert_h16(dtext.float(), BWD), bw["w_tproj"], None, dEOT, epilogue=hip.EPI_F32, prec=BWD)
    hip.layernorm_backward(saved[sh["TL"]], bw["lnf_g"], dEOT, dX, x_row_index=eot, dx_row_index=eot, rows=n)
    s = _block_scratch(dev, R, W, 4 * W, recompute=True)
    hip.convert_h16(dX, BWD, out=s.dx16)
    for i in reversed(range(sh["TL"])):
        P, X0 = bw["layers"][i], saved[i]
        _block_recompute(P, P["ln"], X0, s, batch=n, heads=H, n_q=L, n_kmain=L, causal=True)
        _block_backward(P, P["ln"][2], dX, s, s.X1, s.pre, s.qkv, None, batch=n, heads=H, n=L, causal=True)
        hip.layernorm_backward(X0, P["ln"][0], s.dxn, dX, accumulate=True, dx16=s.dx16)
    # x0 = [SOS | ctx[c] | suffix] + positional_embedding  (VitaCLIP_text_encoder.py:323-332,157): ctx rows 1..n_ctx
    return dX.view(n, L, W)[:, 1:1 + n_ctx].clone()


class TextTowerFn(torch.autograd.Function):
    """text features = f(ctx) with the HIP text tower in both directions."""

    @staticmethod
    def forward(fctx, model, ctx_param):
        out, saved = text_forward_train(model, ctx_param)
        fctx.model = model
        fctx.save_for_backward(saved)
        return out

    @staticmethod
    def backward(fctx, dtext):
        (saved,) = fctx.saved_tensors
        dctx = text_backward(fctx.model, saved, dtext)
        return None, dctx.to(dtext.dtype)


# ---- vision tower: gradients of the Vita-CLIP prompt parameters through the frozen ViT -----------

def _summary_weights(blk):
    """Pack entries of the summary attention's projections: the only trainable weights with bf16 copies."""
    s, P = blk.summary_attn_layer, {}
    P["w_sqkv"], P["w_sqkv_t"] = _both(torch.cat([s.q_proj.weight, s.k_proj.weight, s.v_proj.weight], 0))
    P["w_sout"], P["w_sout_t"] = _both(s.out_proj.weight)
    return P


def pack_vision_backward(model):
    """bf16 copies, in both orientations, of the vision block weights and of the summary path's projections."""
    v = model.visual
    layers = []
    for blk in v.blocks:
        a = blk.attn
        wqkv = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach()
        D = wqkv.shape[1]
        P = _block_weights(wqkv, torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0), a.out_proj, blk.mlp.fc1, blk.mlp.fc2)
        P["w_kv"], P["w_kv_t"] = _both(wqkv[D:])
        P["w_cls"], P["w_cls_t"] = _both(blk.cls_proj.weight)
        P["b_cls"] = f32(blk.cls_proj.bias)
        layers.append({**P, **_summary_weights(blk)})
    # patch rows = patches @ Wp^T, Wp = conv weight as [D][3*P*P]: d patches = d rows @ Wp = gemm(d rows, W = Wp^T), its 3*P*P
    # output columns padded with zero weight rows to the GEMM's granularity of N
    wp_t = v.patch_embed.proj.weight.detach().float().flatten(1).t()
    wp_t = torch.nn.functional.pad(wp_t, (0, 0, 0, -wp_t.shape[0] % 128))
    return dict(layers=layers, proj=_bf16(v.proj),     # cls_x = ln_post(x) @ proj (D,E): dx = d @ proj^T = gemm(d, W=proj)
                w_patch_t=_bf16(wp_t), summary_ver=model._summary_weight_versions())


def refresh_vision_backward(model, bw):
    """After an optimizer step: re-convert the summary-attention projections that changed, and nothing else."""
    cur = model._summary_weight_versions()
    for i, blk in enumerate(model.visual.blocks):
        if cur[i] != bw["summary_ver"][i]:
            bw["layers"][i].update(_summary_weights(blk))
    bw["summary_ver"] = cur


def _pad_k(t, mult=64):
    """[N][K] -> K padded with zero columns to a multiple of `mult` (GEMM reduction-dim granularity)."""
    k = t.shape[1]
    kp = (k + mult - 1) // mult * mult
    return t.contiguous() if kp == k else torch.nn.functional.pad(t, (0, kp - k)).contiguous()


def _wgrad(dy16, x16):
    """dW[o][i] = sum_m dy[m][o] * x[m][i] for an nn.Linear weight [out][in]: gava_gemm on the transposed operands."""
    A, W = _pad_k(dy16.t()), _pad_k(x16.t())
    out = torch.empty(A.shape[0], W.shape[0], dtype=torch.float32, device=dy16.device)
    hip.gemm(A, W, None, out, epilogue=hip.EPI_F32, prec=BWD)
    return out


def kept_bytes(model, B, T):
    sh = model._shape
    n1 = (sh["size"] // sh["P"]) ** 2 + 1
    R, D, F, NL = B * T * n1, sh["D"], sh["F"], sh["layers"]
    return R * D * 4 * (2 * NL + 1) + NL * R * 3 * D * 2 + (NL - 1) * R * F * 2 + NL * (sh["G"] + 2 * B * T) * 2 * D * 2


def alloc_kept(model, B, T, device):
    """Per-block activation buffers for gava_vision_forward_keep (include/gava_hip.h, gava_vision_saved)."""
    sh = model._shape
    n1 = (sh["size"] // sh["P"]) ** 2 + 1
    R, D, F, NL, SR = B * T * n1, sh["D"], sh["F"], sh["layers"], sh["G"] + 2 * B * T
    h16 = hip.h16_dtype(model.prec)
    e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=device)
    BT = B * T
    return dict(e0=e(R, D), x=e(NL + 1, R, D), x1=e(max(NL - 1, 1), R, D), qkv=e(NL, R, 3 * D, dtype=h16),
                pre=e(max(NL - 1, 1), R, F, dtype=h16), sidekv=e(NL, SR, 2 * D, dtype=h16),
                # the last block runs on the CLS rows only (as in inference): its CLS queries / stream / pre-activations
                last_q=e(BT, D, dtype=h16), last_x1=e(BT, D), last_pre=e(BT, F, dtype=h16))


def _vision_dims(model, B_in, T_in, dev):
    """T_in frames per input clip; the blocks regroup the B_in*T_in frames by the MODEL's num_frames regardless
    (vision_encoder_utils.py:160-162): inside the block loop (B, T) are (groups, num_frames), the head and the temporal
    embedding keep the input's (B_in, T_in)."""
    sh, T = model._shape, model.num_frames
    B, n1 = B_in * T_in // T, (sh["size"] // sh["P"]) ** 2 + 1
    return SimpleNamespace(B_in=B_in, T_in=T_in, B=B, T=T, BT=B * T, n1=n1, R=B * T * n1, SR=sh["G"] + 2 * B * T, D=sh["D"],
                           H=sh["H"], F=sh["F"], E=sh["E"], G=sh["G"], NL=sh["layers"], dev=dev)


def _vision_scratch(d, recompute):
    """Every fixed-shape scratch tensor of the block loop, allocated once per backward call (stream order makes the reuse
    from block to block safe).  Nothing in here may end up in the returned gradients: those are fresh tensors."""
    b, f = (lambda *shape: new(d.dev, *shape)), (lambda *shape: new(d.dev, *shape, dtype=torch.float32))
    BT, D, SR = d.BT, d.D, d.SR
    s = _block_scratch(d.dev, d.R, D, d.F, recompute)
    if recompute:
        s.SIDEn, s.SIDEKV = b(SR, D), b(SR, 2 * D)
    # prompt path forward (cls_proj, summary_ln, summary attention), then backward; part: per-frame partials of d K/V of the prompt rows
    s.CP, s.CPn, s.SQKV, s.SMIX, s.SUMM = f(BT, D), b(BT, D), b(BT, 3 * D), b(BT, D), f(BT, D)
    s.part, s.dSIDEn, s.dSIDE = f(BT * (d.G + d.T + 1), 2 * D), f(SR, D), f(SR, D)
    s.dSMIX, s.dSQKV, s.dCPn, s.dCLS = b(BT, D), b(BT, 3 * D), f(BT, D), f(BT, D)
    return s


def _block_params(blk):
    """This step's values of the block's LayerNorm affines and summary-attention biases (trainable ones among them, so
    they are read per call, not packed)."""
    a = blk.summary_attn_layer
    return SimpleNamespace(ln=(f32(blk.norm1.weight), f32(blk.norm1.bias), f32(blk.norm2.weight), f32(blk.norm2.bias)),
                           sln_g=f32(blk.summary_ln.weight), sln_b=f32(blk.summary_ln.bias),
                           b_sqkv=f32(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0)), b_sout=f32(a.out_proj.bias))


def _head_backward(model, bw, d, x_final, dcls_x):
    """cls_x = mean_t(ln_post(x_cls) @ proj) (VitaCLIP_vision_encoder.py:126-128), in reverse: mean over T, proj^T, ln_post'
    on the CLS rows.  -> dX [R, D] fp32, zero off the CLS rows."""
    cls_idx = (torch.arange(d.BT, device=d.dev, dtype=torch.int32) * d.n1).contiguous()
    dproj = (dcls_x.float() / d.T_in).unsqueeze(1).expand(d.B_in, d.T_in, d.E).reshape(d.BT, d.E).contiguous()
    dclspost = new(d.dev, d.BT, d.D, dtype=torch.float32)
    hip.gemm(hip.convert_h16(dproj, BWD), bw["proj"], None, dclspost, epilogue=hip.EPI_F32, prec=BWD)
    dX = torch.zeros(d.R, d.D, dtype=torch.float32, device=d.dev)
    hip.layernorm_backward(x_final, f32(model.visual.ln_post.weight), dclspost, dX, x_row_index=cls_idx, dx_row_index=cls_idx, rows=d.BT)
    return dX


def _prompt_recompute(P, prm, gp, lp, X0, d, s):
    """Recompute the prompt ("side") path of a block (vision_encoder_utils.py:164-190): cls_proj of the CLS rows (s.CP),
    summary_ln (s.CPn), the T-token summary attention (s.SQKV, s.SMIX) with its out_proj + residual (s.SUMM).
    gp (G, D) / lp (T, D): the block's global / local prompts.  -> SIDE [SR, D] fp32, the rows every frame attends to
    besides its own: [global prompts | local prompts + CP | summary tokens]."""
    BT, D = d.BT, d.D
    cls16 = hip.convert_h16(X0.view(BT, d.n1, D)[:, 0], BWD)
    hip.gemm(cls16, P["w_cls"], P["b_cls"], s.CP, epilogue=hip.EPI_F32, prec=BWD)
    hip.layernorm(s.CP, prm.sln_g, prm.sln_b, out16=s.CPn, prec=BWD)
    hip.gemm(s.CPn, P["w_sqkv"], prm.b_sqkv, s.SQKV, epilogue=hip.EPI_H16, prec=BWD, scale_cols=D, scale=0.125)
    hip.attention(*split3(s.SQKV), s.SMIX, batch=d.B, heads=d.H, n_q=d.T, n_kmain=d.T, prec=BWD)
    hip.gemm(s.SMIX, P["w_sout"], prm.b_sout, s.SUMM, epilogue=hip.EPI_F32, prec=BWD, resid=s.CP)
    return torch.cat([gp, (s.CP.view(d.B, d.T, D) + lp).view(BT, D), s.SUMM], 0).contiguous()


def _main_activations(kept, i, cls_only, P, prm, X0, SIDE, d, s):
    """-> (SIDEKV, qkv, X1, pre) of block i: the prompt rows' K/V, the main rows' q/k/v, the stream after the attention
    branch and the fc1 pre-activation.  From what the forward kept (in its operand type; for a CLS-only last block X1 and
    pre are the CLS rows' only), or recomputed from the block input X0 and SIDE with the forward kernels (bf16)."""
    if kept is not None:
        X1, pre = (kept["last_x1"], kept["last_pre"]) if cls_only else (kept["x1"][i], kept["pre"][i])
        return kept["sidekv"][i], kept["qkv"][i], X1, pre
    D = d.D
    hip.layernorm(SIDE, prm.ln[0], prm.ln[1], out16=s.SIDEn, prec=BWD)
    hip.gemm(s.SIDEn, P["w_kv"], P["b_qkv"][D:], s.SIDEKV, epilogue=hip.EPI_H16, prec=BWD)
    _block_recompute(P, prm.ln, X0, s, batch=d.BT, heads=d.H, n_q=d.n1, n_kmain=d.n1,
                     side_k=s.SIDEKV[:, :D], side_v=s.SIDEKV[:, D:], n_g=d.G, T=d.T, has_summary=True)
    return s.SIDEKV, s.qkv, s.X1, s.pre


def _cls_only_backward(P, ln2_g, dX, s, last_q, qkv, X1c, pre_c, act, rel=None, **attn):
    """The main-row backward of a kept last block: only the CLS rows carry a gradient (VitaCLIP_vision_encoder.py:126) -
    MLP', out_proj' and the query side of attention' on B*T rows (last_q, X1c, pre_c: the CLS rows' queries, stream and
    pre-activation); keys / values (and through them every row of the block input) in full.  Leaves s.dxn like
    `_block_backward`, and takes `rel` like it (the queries and d mix are then the CLS rows' own buffers)."""
    BT, D = last_q.shape
    n1 = dX.shape[0] // BT
    c = _block_scratch(dX.device, BT, D, pre_c.shape[1])
    dXc = dX.view(BT, n1, D)[:, 0].contiguous()
    hip.convert_h16(dXc, BWD, out=c.dx16)
    _mlp_backward(P, ln2_g, dXc, c, X1c, pre_c, act)
    if rel is not None and rel(last_q, c.dmix):
        return True
    dq_c = new(dX.device, BT, D)
    hip.attention_backward(last_q, *split3(qkv)[1:], c.dmix, dq_c, *split3(s.dqkv)[1:], prec=BWD, q_scale=0.125, act_prec=act,
                           n_q=1, q_batch_rows=1, **attn)
    hip.gemm(s.dqkv[:, D:], P["w_kv_t"], None, s.dxn, epilogue=hip.EPI_F32, prec=BWD)          # [dK dV] . [Wk; Wv]
    dxn_cls = s.dxn.view(BT, n1 * D)[:, :D]                                                     # CLS rows, stride n1*D
    hip.gemm(dq_c, P["w_qkv_t"][:, :D], None, dxn_cls, epilogue=hip.EPI_F32, prec=BWD, resid=dxn_cls)   # + dQ . Wq
    dX.view(BT, n1, D)[:, 0] = dXc


def _relevance_step(st, d, i, q, qkv, SIDEKV, dmix, act):
    """One step of the relevance chain (VitaCLIP.relevance_maps) at block i, from the last block to the
    first: r <- r + mean_h gava_attention_relevance(w = r) on this block's q / k / v, the prompt rows' keys and d mix, the
    gradient with respect to the attention output that the backward has just formed.  In the last block only the CLS rows
    of d mix are non-zero (only the CLS output is used), so its step is the one-query form r = e_cls + mean_h out, whether
    q and dmix are the CLS rows' own buffers (kept route) or the block's full ones (recompute route).  st: the request's
    state - "r" fp32 [BT, n1]; "capture" (tests only): a list that receives clones of the step's operands.  -> True after
    block 0's step: the chain is complete and nothing further of the backward is needed."""
    D = d.D
    k, v, side_k = qkv[:, D:2 * D], qkv[:, 2 * D:], SIDEKV[:, :D]
    if st.get("capture") is not None:
        c = lambda t: t.clone(memory_format=torch.contiguous_format)
        st["capture"].append(dict(layer=i, q=c(q), k=c(k), v=c(v), side_k=c(side_k), dmix=c(dmix), act=act))
    common = dict(batch=d.BT, heads=d.H, n_kmain=d.n1, prec=BWD, act_prec=act, side_k=side_k, n_g=d.G, T=d.T, has_summary=True)
    if i == d.NL - 1:
        r = hip.attention_relevance(q, k, v, dmix, n_q=1, q_batch_rows=q.shape[0] // d.BT, **common).mean(1)
        r[:, 0] += 1.0
    else:
        r = st["r"] + hip.attention_relevance(q, k, v, dmix, n_q=d.n1, w=st["r"], **common).mean(1)
    st["r"] = r.contiguous()
    return i == 0


def _prompt_backward(P, prm, i, SIDE, dsummary, dX, grads, dgp, d, s):
    """The prompt rows' backward: sum the partials over the frames that share a row (global: all; local: the T frames of
    the clip; summary: its own frame), then K/V projection^T, norm1', split into global / local / summary; summary
    attention' with its weight and bias gradients, summary_ln', and cls_proj' back onto the CLS rows of dX.  dsummary: the
    auxiliary head's gradient of the summary (last block only) or None.  Fills `grads` with block i's entries and dgp[i]."""
    B, T, BT, D, G = d.B, d.T, d.BT, d.D, d.G
    pv = s.part.view(B, T, G + T + 1, 2 * D)      # attention' wrote d K/V of the shared prompt rows as per-frame partials
    dsidekv = torch.cat([pv[:, :, :G].sum(dim=(0, 1)), pv[:, :, G:G + T].sum(dim=1).reshape(BT, 2 * D),
                         pv[:, :, G + T].reshape(BT, 2 * D)], 0).contiguous()
    hip.gemm(hip.convert_h16(dsidekv, BWD), P["w_kv_t"], None, s.dSIDEn, epilogue=hip.EPI_F32, prec=BWD)
    hip.layernorm_backward(SIDE, prm.ln[0], s.dSIDEn, s.dSIDE)
    dgp[i] = s.dSIDE[:G]
    dlocal, dSUMM = s.dSIDE[G:G + BT], s.dSIDE[G + BT:]
    if dsummary is not None:
        # summary = mean over T of the last block's summary tokens (VitaCLIP_vision_encoder.py:129-130)
        dSUMM = dSUMM + (dsummary.float() / T).repeat_interleave(T, dim=0)
    grads[f"blocks.{i}.local_prompts"] = dlocal.view(B, T, D).sum(0).unsqueeze(0)
    dCP = (dlocal + dSUMM).contiguous()                      # local = lp + CP;  SUMM = CP + out_proj(...)
    # ---- summary attention' (T tokens per clip) with parameter gradients
    dSUMM16 = hip.convert_h16(dSUMM, BWD)
    hip.gemm(dSUMM16, P["w_sout_t"], None, s.dSMIX, epilogue=hip.EPI_H16, prec=BWD)
    grads[f"blocks.{i}.summary_attn_layer.out_proj.weight"] = _wgrad(dSUMM16, s.SMIX)
    grads[f"blocks.{i}.summary_attn_layer.out_proj.bias"] = dSUMM.sum(0)
    hip.attention_backward(*split3(s.SQKV), s.dSMIX, *split3(s.dSQKV), batch=B, heads=d.H, n=T, prec=BWD, q_scale=0.125)
    dWs = _wgrad(s.dSQKV, s.CPn)
    dbs = s.dSQKV.float().sum(0)
    for k, nm in enumerate(("q_proj", "k_proj", "v_proj")):
        grads[f"blocks.{i}.summary_attn_layer.{nm}.weight"] = dWs[k * D:(k + 1) * D]
        grads[f"blocks.{i}.summary_attn_layer.{nm}.bias"] = dbs[k * D:(k + 1) * D]
    hip.gemm(s.dSQKV, P["w_sqkv_t"], None, s.dCPn, epilogue=hip.EPI_F32, prec=BWD)
    dg, db = torch.zeros(D, device=d.dev), torch.zeros(D, device=d.dev)
    hip.layernorm_backward(s.CP, prm.sln_g, s.dCPn, dCP, accumulate=True, dgamma=dg, dbeta=db)
    grads[f"blocks.{i}.summary_ln.weight"], grads[f"blocks.{i}.summary_ln.bias"] = dg, db
    # ---- cls_proj' (frozen weight): back onto the CLS rows of the block input
    hip.gemm(hip.convert_h16(dCP, BWD), P["w_cls_t"], None, s.dCLS, epilogue=hip.EPI_F32, prec=BWD)
    dX.view(BT, d.n1, D)[:, 0] += s.dCLS


def _embedding_backward(model, d, e0, dX, dx16=None):
    """ln_pre' (in place on dX; e0 is the embedding output it normalised) and the temporal embedding
    (VitaCLIP_vision_encoder.py:86-100,108-113): time_embed[t] is added to every token of frame t.  -> d time_embed.
    dx16: receives the bf16 copy of the finished dX (the operand of _input_backward's GEMM)."""
    hip.layernorm_backward(e0, f32(model.visual.ln_pre.weight), dX, dX, dx16=dx16)
    dte = dX.view(d.B_in, d.T_in, d.n1, d.D).sum(dim=(0, 2))
    if d.T_in != d.T:   # nearest-resized time_embed (VitaCLIP_vision_encoder.py:91-95): row t of the resized table is row floor(t*T/T_in)
        src = (torch.arange(d.T_in, device=d.dev) * d.T) // d.T_in
        dte = torch.zeros(d.T, d.D, dtype=dte.dtype, device=d.dev).index_add_(0, src, dte)
    return dte


def _input_backward(model, bw, d, dx16, mode, x=None, path=None):
    """d(embedding output) -> d x (VitaCLIP_vision_encoder_utils.py:31-53 in reverse).  dx16 [R, D]: the bf16 copy of dX after
    ln_pre', all B_in*T_in*(n+1) rows in (b, t_in) order.  The embedding is patches @ Wp^T plus terms that do not depend on x
    (conv bias, pos_embed, time_embed, the cls_token rows), so d patches = dX @ Wp - one dgrad GEMM over every row, the CLS
    rows included (1/(n+1) of the work, and no gather) - and gava_unpatchify folds the patch rows back into the clip, skipping
    each frame's CLS row.  mode: hip.UNPATCH_*; GRAD -> fp32 [B_in, 3, T_in, size, size], the map modes -> [B_in, T_in, size,
    size] (x: the fp32 clip, UNPATCH_GRAD_X_INPUT only).  The product lives for this call only.
    path: the path request of VitaCLIP.integrated_gradients / smooth_grad - the B_in clips are m copies each of B_in / m clips,
    mode is hip.PATH_* and the fold reduces the copies with the weights w as it goes (gava_unpatchify_path), into path["out"]:
    one map per ORIGINAL clip, the m gradients are never formed."""
    sh, w = model._shape, bw["w_patch_t"]
    dpatch = new(d.dev, d.R, w.shape[0], dtype=torch.float32)
    hip.gemm(dx16, w, None, dpatch, epilogue=hip.EPI_F32, prec=BWD)
    if path is not None:
        geo = dict(B=d.B_in // path["m"], T=d.T_in, size=sh["size"], patch=sh["P"], frame_rows=d.n1, row_offset=1, w=path["w"], x=x,
                   baseline=path.get("baseline"))
        if path.get("signed") is not None:      # the signed map next to an unsigned one: a second fold of the same rows
            hip.unpatchify_path(dpatch, path["signed"], mode=hip.PATH_ATTR_SUM, **geo)
        return hip.unpatchify_path(dpatch, path["out"], mode=mode, **geo)
    shape = (d.B_in, 3, d.T_in) if mode == hip.UNPATCH_GRAD else (d.B_in, d.T_in)
    out = new(d.dev, *shape, sh["size"], sh["size"], dtype=torch.float32)
    return hip.unpatchify(dpatch, out, B=d.B_in, T=d.T_in, size=sh["size"], patch=sh["P"], mode=mode, frame_rows=d.n1, row_offset=1, x=x)


def vision_backward(model, saved, dcls_x, B, T, dsummary=None, kept=None, input_grad=None):
    """d cls_x (B,E) [+ d summary (B,D), the auxiliary NTE head's input] -> {parameter name: gradient} for the trainable
    vision parameters.  `kept` (alloc_kept, filled by the forward) replaces the per-block recomputation of the main rows:
    activations are then in the forward's operand type (fp16 by default) while gradients stay bf16 - the attention
    backward converts K/V/Q as it stages them, the QuickGELU' epilogue decodes the pre-activation by its own flag.
    input_grad: None, or dict(mode=hip.UNPATCH_*, x=the fp32 clip or None) - the result then also holds "input", the gradient
    with respect to the clip or the saliency map of it (_input_backward); without it not one launch differs.  Or
    dict(relevance=state): every block also runs _relevance_step, the gradient chain between the blocks stays the true one
    (prompt path included), and the call ends after block 0's step - what follows it (attention', the prompt path, LN1', the
    embedding, the input) adds nothing to the chain - with {"relevance": r fp32 [B*T, n1]} as its only result."""
    bw, v = model._backward_pack("vision"), model.visual
    d = _vision_dims(model, B, T, dcls_x.device)
    if kept is not None:      # block inputs x[i] (x[NL]: the last block's output), embedding output, activations' storage type
        xs, e0, act, last_q = kept["x"], kept["e0"], model.prec, kept.get("last_q")
    else:
        xs, e0, act, last_q = saved[1:], saved[0], BWD, None
    NL, D, grads = d.NL, d.D, {}
    dX = _head_backward(model, bw, d, xs[NL], dcls_x)
    s = _vision_scratch(d, recompute=kept is None)
    hip.convert_h16(dX, BWD, out=s.dx16)
    dgp = torch.zeros_like(v.global_prompts, dtype=torch.float32)
    rel_state = input_grad.get("relevance") if input_grad is not None else None
    for i in reversed(range(NL)):
        P, blk, X0 = bw["layers"][i], v.blocks[i], xs[i]
        prm = _block_params(blk)
        cls_only = last_q is not None and i == NL - 1
        SIDE = _prompt_recompute(P, prm, v.global_prompts.detach().float()[i], blk.local_prompts.detach().float()[0], X0, d, s)
        SIDEKV, qkv, X1, pre = _main_activations(kept, i, cls_only, P, prm, X0, SIDE, d, s)
        attn = dict(batch=d.BT, heads=d.H, n=d.n1, side_k=SIDEKV[:, :D], side_v=SIDEKV[:, D:], dside_k=s.part[:, :D],
                    dside_v=s.part[:, D:], n_g=d.G, T=d.T, has_summary=True)
        rel = None
        if rel_state is not None:
            rel = lambda q, dmix, i=i, qkv=qkv, SIDEKV=SIDEKV: _relevance_step(rel_state, d, i, q, qkv, SIDEKV, dmix, act)
        if cls_only:
            done = _cls_only_backward(P, prm.ln[2], dX, s, last_q, qkv, X1, pre, act, rel=rel, **attn)
        else:
            done = _block_backward(P, prm.ln[2], dX, s, X1, pre, qkv, act, rel=rel, **attn)
        if done:
            return {"relevance": rel_state["r"]}
        _prompt_backward(P, prm, i, SIDE, dsummary if i == NL - 1 else None, dX, grads, dgp, d, s)
        # norm1' of the main rows is applied at the end of the block, after the prompt path has added its share to
        # the CLS rows of dX: it also writes the bf16 copy of the finished dX for the next block
        hip.layernorm_backward(X0, prm.ln[0], s.dxn, dX, accumulate=True, dx16=s.dx16)
    grads["global_prompts"] = dgp
    grads["time_embed"] = _embedding_backward(model, d, e0, dX, dx16=s.dx16 if input_grad is not None else None)
    if input_grad is not None:
        grads["input"] = _input_backward(model, bw, d, s.dx16, input_grad["mode"], input_grad.get("x"),
                                         path=input_grad if "m" in input_grad else None)
    return grads


class VisionTowerFn(torch.autograd.Function):
    """cls_x = f(x; prompt parameters) with the HIP vision tower in both directions.  `params` are the trainable vision
    parameters in `VitaCLIP._vision_trainables` order (they enter only so that autograd routes their gradients).
    clips: None, or the uint8 source of VitaCLIP.forward_frames (encode_video's `clips`; x is then the descriptor tensor).
    Either way the backward starts from what the forward kept (the embedding output and the blocks' activations, or in
    recompute mode the fp32 input of every block): the input is read by the forward's patch embedding only, so neither the
    descriptors nor the decoded videos are held for the backward.
    The backward returns d x when an fp32 x asks for it (never on the uint8 route).  request: None, or the dict of
    VitaCLIP.saliency - mode (hip.UNPATCH_*) and x; a map mode's result is left in request["out"] instead of being returned
    (it has not x's shape), so that the full-size gradient is never formed.  Or the dict of VitaCLIP.relevance_maps,
    dict(relevance=state): the backward then runs the relevance chain beside the gradient, leaves r in request["out"] and
    returns no gradient at all.  Or the path form of VitaCLIP.integrated_gradients / smooth_grad, dict(mode=hip.PATH_*, m, w,
    x, baseline, out, signed): x holds m copies of every clip, the fold reduces them with the weights w (gava_unpatchify_path) into the
    tensor the caller put in request["out"], and no gradient is returned either."""

    @staticmethod
    def forward(fctx, model, x, clips, request, *params):
        sh = model._shape
        B, T = (clips[1], clips[2]) if clips is not None else (x.shape[0], x.shape[2])
        n1 = (sh["size"] // sh["P"]) ** 2 + 1
        fctx.model, fctx.BT, fctx.request = model, (B, T), request
        if kept_bytes(model, B, T) <= model.keep_activation_bytes:
            fctx.kept = alloc_kept(model, B, T, x.device)
            cls_x, summary = model.encode_video(x, kept=fctx.kept, clips=clips)
            fctx.save_for_backward()
        else:
            fctx.kept = None
            saved = torch.empty(sh["layers"] + 2, B * T * n1, sh["D"], dtype=torch.float32, device=x.device)
            cls_x, summary = model.encode_video(x, saved=saved, clips=clips)
            fctx.save_for_backward(saved)
        return cls_x, summary

    @staticmethod
    def backward(fctx, dcls_x, dsummary):
        model, kept = fctx.model, fctx.kept
        saved = fctx.saved_tensors[0] if kept is None else None
        dev = (kept["x"] if kept is not None else saved).device
        if dcls_x is None:
            dcls_x = torch.zeros(fctx.BT[0], model._shape["E"], device=dev)
        req = None
        if fctx.needs_input_grad[1]:      # (never on the uint8 route: its x is the descriptor tensor)
            req = fctx.request if fctx.request is not None else dict(mode=hip.UNPATCH_GRAD)
        g = vision_backward(model, saved, dcls_x.contiguous(), *fctx.BT, dsummary=dsummary, kept=kept, input_grad=req)
        fctx.kept = fctx.request = None      # release the activation buffers with the graph
        dx = g.get("input")
        if "relevance" in g:
            req["out"] = g["relevance"]
        if dx is not None and (req["mode"] != hip.UNPATCH_GRAD or "m" in req):      # a map, or a path request's reduced result
            req["out"], dx = dx, None
        out = []
        for name, p in model._vision_trainables():
            gi = g.get(name)
            out.append(gi.reshape(p.shape).to(p.dtype) if (gi is not None and p.requires_grad) else None)
        return (None, dx, None, None, *out)


# =================================================================================================
# The step's tail: similarity head and criterion on the device (opt-in)
# =================================================================================================
# With VitaCLIP.train_head = "hip" the head between the towers' outputs and the logits is HeadFn (the inference head's kernels
# forward, fp32 MFMA tiles backward) instead of the traced torch ops of VitaCLIP._train_head, and TrainCriterion is the
# criterion of training/train.py:360-362,446-452 (cross-entropy x ordinal-focal weight of training/loss_utils.py:9-46, mean)
# as two launches forward and one backward.  Not covered here: soft (mixup) labels - they have their own route below (ClipMixer,
# SoftTargetCriterion) - and the InfoNCE variants of loss_utils.py, which stay torch code on the caller's side; the auxiliary heads and their terms (the sigmoid memory criterion among them) are further down.

class HeadFn(torch.autograd.Function):
    """(logits [B, C], text_features [C, E]) = head(video [B, E], text [P, E], logit_scale, logit_bias or None, class_offsets):
    gava_train_head / gava_train_head_backward.  Saved for the backward (save_for_backward, so they die with the graph and an
    in-place edit of the logits is caught): the unit rows, their inverse norms, the class means and the logits - (B + P + 2C) x E
    floats, none of the towers' activations.  text_features carries a gradient back (the support-memory head reads it); an
    unused output costs nothing (its gradient stays undefined -> NULL)."""
    SAVED = ("video_norm", "video_inv", "text_norm", "text_inv", "class_mean", "logits", "class_offsets", "logit_scale", "logit_bias")

    @staticmethod
    def forward(fctx, video, text, logit_scale, logit_bias, offsets):
        kept = hip.train_head(video.detach().float(), text.detach().float(), offsets, logit_scale.detach().float(),
                              logit_bias.detach().float() if logit_bias is not None else None)
        fctx.save_for_backward(*[kept[k] for k in HeadFn.SAVED])
        fctx.dims = {k: kept[k] for k in ("B", "C", "P", "E")}
        fctx.set_materialize_grads(False)
        fctx.shapes = (logit_scale.shape, logit_bias.shape if logit_bias is not None else None)
        fctx.dtypes = (video.dtype, text.dtype, logit_scale.dtype)
        return kept["logits"], kept["text_features"]

    @staticmethod
    def backward(fctx, dlogits, dtf):
        kept = dict(zip(HeadFn.SAVED, fctx.saved_tensors), **fctx.dims)
        if dlogits is None:
            dlogits = torch.zeros_like(kept["logits"])
        dvideo, dtext, dls, dlb = hip.train_head_backward(kept, dlogits.float(), dtf.float() if dtf is not None else None)
        ls_shape, lb_shape = fctx.shapes
        return (dvideo.to(fctx.dtypes[0]), dtext.to(fctx.dtypes[1]), dls.reshape(ls_shape).to(fctx.dtypes[2]),
                dlb.reshape(lb_shape) if dlb is not None else None, None)


class _CriterionFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logits, labels, crit):
        out = hip.train_criterion(logits.detach(), labels, weighted=crit.focal_ordinal, alpha=crit.alpha, gamma=crit.gamma,
                                  beta=crit.beta, scale=crit.scale, conf=crit.conf, check_labels=crit.check_labels)
        fctx.save_for_backward(logits.detach(), out["labels"], out["saved"])
        crit.last = {k: out[k] for k in ("per_sample", "weight", "top1", "hits", "conf")}
        return out["loss"]

    @staticmethod
    def backward(fctx, g):
        logits, labels, saved = fctx.saved_tensors
        return hip.train_criterion_backward(logits, labels, saved, g.float().contiguous()), None, None


class TrainCriterion:
    """loss = crit(logits, labels): the criterion of the reference's training loop on the device (gava_train_criterion).
    focal_ordinal=False is torch.nn.CrossEntropyLoss()(logits, labels); True multiplies every sample's cross-entropy by
    scale * (beta * |label - argmax| / (C - 1) + alpha * (1 - p_label)^gamma) before the mean (training/train.py:361-362 uses
    gamma 2, alpha 0.25 and beta 0.2 for UPDRS).  Any device fp32 [B, C] logits with int64 (integer) labels [B]; soft targets
    are refused.  After a call, `last` holds device tensors per_sample, weight, top1 (int32), hits (int32 scalar) and conf:
    nothing is read back - read hits when you print.  conf: pass track_confusion=True to keep an int32 [C, C] matrix
    conf[label, top1] that every call adds to (reset_confusion() clears it).  check_labels=True validates the label range on
    the host (a sync); by default out-of-range labels are clamped on the device."""

    def __init__(self, focal_ordinal=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, track_confusion=False, check_labels=False):
        if focal_ordinal and not gamma >= 1.0:
            raise hip.GavaError("TrainCriterion needs gamma >= 1: the focal factor's derivative is unbounded at p = 1 below that")
        self.focal_ordinal, self.alpha, self.gamma, self.beta, self.scale = bool(focal_ordinal), float(alpha), float(gamma), float(beta), float(scale)
        self.track_confusion, self.check_labels = track_confusion, check_labels
        self.conf, self.last = None, {}

    def reset_confusion(self):
        self.conf = None

    def __call__(self, logits, labels):
        if not (torch.is_tensor(labels) and not labels.is_floating_point() and labels.dim() == 1):
            raise hip.GavaError("TrainCriterion takes integer class labels [B]; soft (mixup) targets are not supported")
        if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
            raise hip.GavaError("TrainCriterion takes device fp32 logits [B, C]")
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        if self.track_confusion and (self.conf is None or self.conf.shape[0] != logits.shape[1] or self.conf.device != logits.device):
            self.conf = torch.zeros(logits.shape[1], logits.shape[1], dtype=torch.int32, device=logits.device)
        return _CriterionFn.apply(logits, labels.to(logits.device), self)


# =================================================================================================
# Mixup / CutMix on the device and the criterion for the soft targets they make (opt-in)
# =================================================================================================
# The reference's loss code takes targets of the logits' shape (training/loss_utils.py:32-44, CrossEntropyLoss with class
# probabilities) and its loop keeps the branch for them (training/train.py:477), but it ships no mixing code.  ClipMixer mixes
# a preprocessed fp32 batch and builds the targets (gava_mix_clips, gava_mix_targets); SoftTargetCriterion is the criterion for
# them (gava_soft_criterion*), under autograd like TrainCriterion.  TrainCriterion and AuxCriterion keep their integer labels.
# Not covered: a gradient through the mix to x, mixing uint8 frames (call pre.batch(videos), then the mixer), the memory batch.

class _SoftCriterionFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logits, targets, crit):
        kw = dict(weighted=crit.focal_ordinal, alpha=crit.alpha, gamma=crit.gamma, beta=crit.beta, scale=crit.scale)
        out = hip.soft_criterion(logits.detach(), targets, conf=crit.conf, **kw)
        fctx.save_for_backward(logits.detach(), targets, out["saved"])
        fctx.kw = kw
        crit.last = {k: out[k] for k in ("per_sample", "weight", "top1", "target1", "hits", "conf")}
        return out["loss"]

    @staticmethod
    def backward(fctx, g):
        logits, targets, saved = fctx.saved_tensors
        return hip.soft_criterion_backward(logits, targets, saved, g.float().contiguous(), **fctx.kw), None, None


class SoftTargetCriterion:
    """loss = crit(logits, targets): the reference's criterion for targets of the logits' shape, on the device
    (gava_soft_criterion).  focal_ordinal=False is torch.nn.CrossEntropyLoss()(logits, targets) with class probabilities;
    True multiplies every sample's cross-entropy by scale * (beta * |argmax targets - argmax logits| / (C - 1) * sum(targets)
    + alpha * sum_c targets_c (1 - p_c)^gamma) before the mean (training/loss_utils.py:32-44 with a y_true of the logits'
    shape).  Device fp32 [B, C] logits and device fp32 [B, C] targets (what ClipMixer returns); integer labels are refused -
    they go to TrainCriterion.  No gradient flows to the targets.  After a call, `last` holds device tensors per_sample,
    weight, top1, target1 (int32: the argmax of the logits and of the targets), hits (int32 scalar, #{top1 == target1}) and
    conf; nothing is read back.  track_confusion=True keeps an int32 [C, C] matrix conf[target1, top1] that every call adds
    to (reset_confusion() clears it)."""

    def __init__(self, focal_ordinal=False, alpha=0.25, gamma=2.0, beta=0.0, scale=1.0, track_confusion=False):
        if focal_ordinal and not gamma >= 1.0:
            raise hip.GavaError("SoftTargetCriterion needs gamma >= 1: the focal factor's derivative is unbounded at p = 1 below that")
        self.focal_ordinal, self.alpha, self.gamma, self.beta, self.scale = bool(focal_ordinal), float(alpha), float(gamma), float(beta), float(scale)
        self.track_confusion = track_confusion
        self.conf, self.last = None, {}

    def reset_confusion(self):
        self.conf = None

    def __call__(self, logits, targets):
        if not (torch.is_tensor(targets) and targets.is_floating_point() and targets.dim() == 2):
            raise hip.GavaError("SoftTargetCriterion takes fp32 targets [B, C] of the logits' shape; integer class labels [B] go to TrainCriterion")
        if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
            raise hip.GavaError("SoftTargetCriterion takes device fp32 logits [B, C]")
        if not (targets.is_cuda and targets.dtype == torch.float32 and targets.shape == logits.shape and targets.device == logits.device):
            raise hip.GavaError("SoftTargetCriterion takes device fp32 targets of the logits' shape, on the logits' device")
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        targets = targets.detach()
        if targets.shape[1] > 1 and targets.stride(1) != 1:
            targets = targets.contiguous()
        if self.track_confusion and (self.conf is None or self.conf.shape[0] != logits.shape[1] or self.conf.device != logits.device):
            self.conf = torch.zeros(logits.shape[1], logits.shape[1], dtype=torch.int32, device=logits.device)
        return _SoftCriterionFn.apply(logits, targets, self)


class ClipMixer:
    """x_mixed, targets = mixer(x, labels): Mixup / CutMix of a preprocessed batch on the device (gava_mix_clips) and the soft
    targets that go with it (gava_mix_targets), for SoftTargetCriterion.  x: device fp32 [B, 3, T, S, S]; labels: device
    integer [B]; -> x's shape, fp32 [B, C].  Clip i is mixed with clip B - 1 - i (the middle clip of an odd batch stays as it
    is).  Mixup: lam x_i + (1 - lam) x_partner; CutMix: a box of the partner pasted through every frame.  mode: "batch" draws
    once for the whole batch, "pair" once per pair, "elem" once per clip.  label_smoothing spreads eps over the classes before
    the targets are mixed; ClipMixer(C, mixup_alpha=0, cutmix_alpha=0, label_smoothing=eps) is label smoothing alone.
    inplace=True overwrites x.  No gradient flows through the mix.  Nothing is read back from the device."""

    MODES = ("batch", "pair", "elem")

    def __init__(self, num_classes, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                 correct_lam=True, seed=None):
        import numpy as np
        if mode not in self.MODES:
            raise hip.GavaError(f"ClipMixer: mode must be one of {self.MODES}")
        if not (int(num_classes) >= 1 and mixup_alpha >= 0 and cutmix_alpha >= 0 and 0 <= prob <= 1 and 0 <= switch_prob <= 1
                and 0 <= label_smoothing <= 1):
            raise hip.GavaError("ClipMixer: num_classes >= 1, alphas >= 0, prob, switch_prob and label_smoothing in [0, 1]")
        self.num_classes, self.mixup_alpha, self.cutmix_alpha = int(num_classes), float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.label_smoothing, self.correct_lam = float(label_smoothing), bool(correct_lam)
        self.rng = np.random.default_rng(seed)
        self.last_plan = None

    def _draw_one(self, H, W):
        """(lam, box) of one mixed-or-not unit."""
        rng = self.rng
        none = (1.0, (0, 0, 0, 0))
        if not (self.mixup_alpha > 0 or self.cutmix_alpha > 0) or rng.random() >= self.prob:
            return none
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            return float(rng.beta(self.mixup_alpha, self.mixup_alpha)), (0, 0, 0, 0)
        lam = float(rng.beta(self.cutmix_alpha, self.cutmix_alpha))
        ratio = (1.0 - lam) ** 0.5
        ch, cw = int(H * ratio), int(W * ratio)
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        if self.correct_lam:
            lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
        if y1 <= y0 or x1 <= x0:                       # nothing is pasted: the clip keeps its pixels and its label
            return none
        return lam, (y0, y1, x0, x1)

    def draw(self, B, H=224, W=None):
        """The host plan of one batch: dict(partner int32 [B], lam float32 [B], box int32 [B, 4] as (y0, y1, x0, x1)), numpy.
        partner[i] = B - 1 - i.  With probability `prob` a batch / pair / clip (by `mode`) is mixed: CutMix with probability
        switch_prob when both alphas are positive (otherwise whichever is), lam ~ Beta(alpha, alpha) of the chosen kind.  The
        CutMix box has its centre uniform in the image and sides H sqrt(1 - lam), W sqrt(1 - lam), clipped to the image; with
        correct_lam, lam becomes 1 - area / (H W) of the clipped box.  Unmixed clips get lam = 1 and an empty box.  Everything
        is drawn from the mixer's own numpy generator (np.random.default_rng(seed)) and from nothing else: the reference ships
        no mixing code, so there is no generator order to stay in step with."""
        import numpy as np
        W = H if W is None else W
        partner = (B - 1 - np.arange(B)).astype(np.int32)
        lam, box = np.ones(B, dtype=np.float32), np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            l, b = self._draw_one(H, W)
            lam[:], box[:] = l, b
        elif self.mode == "pair":
            for i in range((B + 1) // 2):
                l, b = self._draw_one(H, W)
                lam[i] = lam[B - 1 - i] = l
                box[i] = box[B - 1 - i] = b
        else:
            for i in range(B):
                lam[i], box[i] = self._draw_one(H, W)
        return dict(partner=partner, lam=lam, box=box)     # the middle clip of an odd batch is its own partner: untouched

    @torch.no_grad()
    def __call__(self, x, labels, plan=None, inplace=False):
        import numpy as np
        if not (torch.is_tensor(x) and torch.is_tensor(labels)):
            raise hip.GavaError("ClipMixer takes tensors")
        if not (x.is_cuda and labels.is_cuda):
            raise hip.GavaError("ClipMixer takes device tensors: there is no CPU fallback")
        if x.dtype != torch.float32 or x.dim() < 3:
            raise hip.GavaError("ClipMixer takes fp32 clips [B, 3, T, S, S] (preprocessed; uint8 frames go through pre.batch first)")
        if x.requires_grad:
            raise hip.GavaError("ClipMixer: x requires grad, and no gradient flows through the mix")
        if labels.is_floating_point() or labels.dim() != 1 or labels.shape[0] != x.shape[0]:
            raise hip.GavaError("ClipMixer takes integer class labels [B]; it makes the soft targets itself")
        if inplace and not x.is_contiguous():
            raise hip.GavaError("ClipMixer: inplace=True needs a contiguous x")
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        if plan is None:
            plan = self.draw(B, H, W)
        self.last_plan = plan
        desc = hip.mix_descriptors(plan, H, W, device=x.device)
        lam, partner = np.asarray(plan["lam"]).reshape(-1), np.asarray(plan["partner"]).reshape(-1)
        box = np.asarray(plan["box"]).reshape(-1, 4)
        boxed = (box[:, 1] > box[:, 0]) & (box[:, 3] > box[:, 2])
        if partner.shape[0] != B or lam.shape[0] != B or box.shape[0] != B:
            raise hip.GavaError("ClipMixer: the plan is for another batch size")
        mixed = (partner != np.arange(B)) & (boxed | (lam != 1))
        if not mixed.any() and not (((partner >= 0) & (partner < B)).all() and ((lam >= 0) & (lam <= 1)).all()):
            raise hip.GavaError("ClipMixer: the plan's partners must lie in [0, B) and its lam in [0, 1]")      # no launch validates it
        if mixed.any():
            xc = x if x.is_contiguous() else x.contiguous()
            x = hip.mix_clips(xc, desc, out=xc if inplace else None)
        targets = hip.mix_targets(labels.to(x.device), desc, self.num_classes, self.label_smoothing)
        return x, targets


# =================================================================================================
# The auxiliary heads and their loss terms on the device (opt-in)
# =================================================================================================
# With VitaCLIP.aux_heads = "hip" the video<->NTE head and the support-memory<->text head (VitaCLIP_model.py:311-398) are
# NteHeadFn and MemoryHeadFn - gava_nte_head* / gava_memory_head*, a constant number of launches whatever the batch and the
# number of classes - instead of the traced torch ops of VitaCLIP._forward_impl, and AuxCriterion is loss_mt and loss_vm of
# training/train.py:454-475.  Not covered: the InfoNCE / cosine-NCE variants of loss_utils.py (the reference's loop does not
# call them) and soft targets.

class NteHeadFn(torch.autograd.Function):
    """logits_vm [B, B] = nte_head(summary [B, D], sum_proj.weight, sum_proj.bias, video_nte [B, K, E], logit_scale_vm).  Saved
    for the backward: summary, the weight, the unit projected rows, the mean unit NTE rows and six [B] / [B, B] arrays - not
    video_nte.  d summary goes back to the vision tower (VisionTowerFn's second output); a frozen parameter gets None."""
    SAVED = ("summary", "weight", "logit_scale") + hip._NTE_KEPT

    @staticmethod
    def forward(fctx, summary, weight, bias, video_nte, logit_scale):
        kept = hip.nte_head(summary, weight, bias, video_nte, logit_scale)
        fctx.save_for_backward(*[kept[k] for k in NteHeadFn.SAVED])
        fctx.dims = {k: kept[k] for k in ("B", "D", "E", "K")}
        fctx.set_materialize_grads(False)
        fctx.meta = [(t.shape, t.dtype) for t in (summary, weight, bias, logit_scale)]
        return kept["logits_vm"]

    @staticmethod
    def backward(fctx, dlogits):
        if dlogits is None:
            return None, None, None, None, None
        kept = dict(zip(NteHeadFn.SAVED, fctx.saved_tensors), **fctx.dims)
        grads = hip.nte_head_backward(kept, dlogits)
        need = [fctx.needs_input_grad[i] for i in (0, 1, 2, 4)]
        out = [g.reshape(shape).to(dtype) if n else None for g, n, (shape, dtype) in zip(grads, need, fctx.meta)]
        return out[0], out[1], out[2], None, out[3]


class MemoryHeadFn(torch.autograd.Function):
    """logits_mt [M, C] = memory_head(memory [M, S, E], text_features [C, E], logit_scale_mt, logit_bias_mt or None, the device
    pointer table of memory_project's parameters, then tf_project's four parameters and memory_project's 4 C as inputs so that
    autograd routes their gradients).  The per-class gradients are written into four stacked buffers and handed out as views.
    d text_features is computed only when text_features asks for a gradient (detach_features passes a detached tensor)."""
    SAVED = ("text_features", "tf_w1", "tf_b1", "tf_w2", "tf_b2", "mem_params", "logit_scale", "logit_bias") + hip._MEM_KEPT

    @staticmethod
    def forward(fctx, memory, text_features, logit_scale, logit_bias, mem_table, *params):
        kept = hip.memory_head(memory, text_features, params[:4], mem_table, logit_scale, logit_bias)
        fctx.save_for_backward(*[kept[k] for k in MemoryHeadFn.SAVED], *params[4:])      # (the table points into params[4:])
        fctx.dims = {k: kept[k] for k in ("M", "S", "C", "E")}
        fctx.set_materialize_grads(False)
        fctx.meta = [(t.shape, t.dtype) if t is not None else None for t in (text_features, logit_scale, logit_bias)]
        return kept["logits_mt"]

    @staticmethod
    def backward(fctx, dlogits):
        n_par = len(fctx.needs_input_grad) - 5
        if dlogits is None:
            return (None,) * (5 + n_par)
        kept = dict(zip(MemoryHeadFn.SAVED, fctx.saved_tensors), **fctx.dims)
        need = fctx.needs_input_grad
        g = hip.memory_head_backward(kept, dlogits, want_dtext=need[1])
        cast = lambda t, meta: t.reshape(meta[0]).to(meta[1])
        dtf = cast(g["dtext_features"], fctx.meta[0]) if need[1] else None
        dls = cast(g["dlogit_scale"], fctx.meta[1]) if need[2] else None
        dlb = cast(g["dlogit_bias"], fctx.meta[2]) if (fctx.meta[2] is not None and need[3]) else None
        par = [g["dtf_w1"], g["dtf_b1"], g["dtf_w2"], g["dtf_b2"]]
        for c in range(fctx.dims["C"]):
            par += [g["dmem_w1"][c], g["dmem_b1"][c], g["dmem_w2"][c], g["dmem_b2"][c]]
        return (None, dtf, dls, dlb, None, *[p if need[5 + i] else None for i, p in enumerate(par)])


class _SigmoidCriterionFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logits, labels, kw):
        out = hip.sigmoid_criterion(logits.detach(), labels, **kw)
        fctx.save_for_backward(logits.detach(), out["labels"])
        fctx.kw = kw
        return out["loss"]

    @staticmethod
    def backward(fctx, g):
        logits, labels = fctx.saved_tensors
        return hip.sigmoid_criterion_backward(logits, labels, g.float().contiguous(), **fctx.kw), None, None


class _NteDiagFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logits_vm, weight):
        fctx.B, fctx.weight = logits_vm.shape[0], weight
        return hip.nte_diag_loss(logits_vm.detach(), weight)

    @staticmethod
    def backward(fctx, g):
        return hip.nte_diag_loss_backward(fctx.B, g.float().contiguous(), fctx.weight), None


class AuxCriterion:
    """(loss_mt, loss_vm) = crit(logits_mt=None, mt_labels=None, logits_vm=None): the auxiliary loss terms of the reference's
    training loop (training/train.py:454-475) on the device, as scalars under autograd; a term whose logits are None is None.

    loss_mt, sigmoid=False: memory_loss_weight * mean cross-entropy(logits_mt, mt_labels), through gava_train_criterion
    (unweighted).  sigmoid=True: memory_loss_weight * mean(sigmoid_focal_loss(scale=memory_loss_weight)(logits_mt, mt_labels))
    through gava_sigmoid_criterion - the weight enters TWICE, as it does in the reference, which builds the criterion with
    scale=args.memory_loss_weight (train.py:365) and multiplies its result by args.memory_loss_weight again (train.py:459).
    use_focal / alpha / gamma are sigmoid_focal_loss's (loss_utils.py:139-177; the reference's loop passes use_focal=False).
    loss_vm = -vnte_loss_weight * mean of the diagonal of logits_vm (gava_nte_diag_loss).
    Integer labels [M] only: soft targets are refused."""

    def __init__(self, memory_loss_weight=1.0, vnte_loss_weight=1.0, sigmoid=False, alpha=0.25, gamma=2.0, use_focal=False):
        if use_focal and not gamma >= 1.0:
            raise hip.GavaError("AuxCriterion needs gamma >= 1 with use_focal: the focal factor's derivative is unbounded at p = 1 below that")
        self.memory_loss_weight, self.vnte_loss_weight = float(memory_loss_weight), float(vnte_loss_weight)
        self.sigmoid, self.alpha, self.gamma, self.use_focal = bool(sigmoid), float(alpha), float(gamma), bool(use_focal)
        self._ce = TrainCriterion()

    @staticmethod
    def _logits(t, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2):
            raise hip.GavaError(f"AuxCriterion takes device {what} of two dimensions")
        return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()

    def __call__(self, logits_mt=None, mt_labels=None, logits_vm=None):
        loss_mt = loss_vm = None
        if logits_mt is not None:
            if not (torch.is_tensor(mt_labels) and not mt_labels.is_floating_point() and mt_labels.dim() == 1):
                raise hip.GavaError("AuxCriterion takes integer class labels [M]; soft targets are not supported")
            logits_mt = self._logits(logits_mt, "logits_mt")
            if self.sigmoid:
                kw = dict(use_focal=self.use_focal, alpha=self.alpha, gamma=self.gamma, scale=self.memory_loss_weight ** 2)
                loss_mt = _SigmoidCriterionFn.apply(logits_mt, mt_labels, kw)
            else:
                loss_mt = self._ce(logits_mt, mt_labels)
                if self.memory_loss_weight != 1.0:
                    loss_mt = loss_mt * self.memory_loss_weight
        if logits_vm is not None:
            loss_vm = _NteDiagFn.apply(self._logits(logits_vm, "logits_vm"), self.vnte_loss_weight)
        return loss_mt, loss_vm
