"""Drop-in ``VitaCLIP(nn.Module)`` whose forward runs on libgava_hip.so (MI355X / gfx950).

Mirrors the reference boundary /root/reference/training/VitaCLIP_model.py:22-401: same
constructor keywords (:24-74), same ``forward(x, memory=None, video_nte=None, desc_wise=False)``
-> ``(logits, logits_mt, logits_vm)`` (:241-244,401), same ``state_dict`` keys,
same public attributes (``visual``, ``textual``, ``prompt_learner``, ``tokenized_prompts``,
``logit_scale``, ``text_features``), same freezing of parameters (:222-239).

The sub-modules below are parameter containers with the reference's names and initialisers; they
compute nothing in PyTorch.  All arithmetic of the hot path happens in the HIP kernels through
the C ABI (gava_clip_amd/hip.py); PyTorch only owns the device memory.  There is no CPU or eager
fallback: a non-device input or a missing library raises.
"""
import ctypes as C
import math
import os
import weakref
from collections import OrderedDict
from typing import List, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip
from .tokenizer import tokenize, read_class_names, prompt_texts

NUM_COMB = 70  # /root/reference/video_dataset/dataset.py:19


# ---------------------------------------------------------------------------------------------
# parameter containers (names/initialisers: VitaCLIP_vision_encoder*.py, VitaCLIP_text_encoder.py)
# ---------------------------------------------------------------------------------------------
class _Params(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - never called
        raise RuntimeError("gava_clip_amd sub-modules hold parameters only; call VitaCLIP.forward")


class _Encoder(_Params):
    """The two L1 encoders of the reference are callable on their own (`videoEncoder(data)`, evaluation/iwa.py:212,230;
    `text_model(token_features, tokenized_prompts)`, evaluation/zero_shot.py:75-76, utils/prepare_embedding.py): forward()
    hands the call to the HIP host that packs this encoder's weights - the VitaCLIP it belongs to, or a private one when
    the encoder was constructed stand-alone."""

    def _host(self):
        ref = self.__dict__.get("_host_ref")
        host = ref() if ref is not None else None
        if host is not None and getattr(host, "visual", None) is not self and getattr(host, "textual", None) is not self:
            host = None          # a deep copy still pointing at the model it was copied from
        if host is None:
            host = self.__dict__.get("_own_host")
            if host is None:
                host = _StandaloneHost(self)
                self.__dict__["_own_host"] = host
        return host


class Attention(_Params):
    """q/k/v/out projections (VitaCLIP_vision_encoder_utils.py:31-57)."""

    def __init__(self, dim):
        super().__init__()
        self.q_proj = nn.Linear(dim, dim)
        self.k_proj = nn.Linear(dim, dim)
        self.v_proj = nn.Linear(dim, dim)
        self.out_proj = nn.Linear(dim, dim)
        for m in (self.q_proj, self.k_proj, self.v_proj, self.out_proj):
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0.)


class LayerNorm(nn.LayerNorm):
    pass


class TransformerEncoderLayer(_Params):
    """VitaCLIP_vision_encoder_utils.py:83-152 (summary token and local prompts always on)."""

    def __init__(self, dim, num_heads, mlp_factor, num_frames, patch_size):
        super().__init__()
        self.attn = Attention(dim)
        mlp_dim = round(mlp_factor * dim)
        self.mlp = nn.Sequential(OrderedDict([("fc1", nn.Linear(dim, mlp_dim)), ("act", nn.Identity()),
                                              ("dropout", nn.Identity()), ("fc2", nn.Linear(mlp_dim, dim))]))
        self.norm1 = LayerNorm(dim)
        self.norm2 = LayerNorm(dim)
        self.cls_proj = nn.Linear(dim, dim)
        self.num_frames = num_frames
        self.summary_ln = LayerNorm(dim)
        self.summary_attn_layer = Attention(dim)
        self.local_prompts = nn.Parameter(torch.zeros(1, num_frames, dim))
        val = math.sqrt(6. / float(3 * patch_size[0] * patch_size[1] + dim))
        nn.init.uniform_(self.local_prompts.data, -val, val)
        for m in (self.mlp.fc1, self.mlp.fc2):
            nn.init.xavier_uniform_(m.weight)
            nn.init.normal_(m.bias, std=1e-6)


class _PatchEmbed(_Params):
    def __init__(self, patch, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)


class CLIPVisionEncoder(_Encoder):
    """VitaCLIP_vision_encoder.py:19-84 (same constructor keywords); forward(x) -> (cls_x (B,E), summary (B,D)), :102-132."""

    def __init__(self, input_size=(224, 224), num_frames=8, feature_dim=768, patch_size=(16, 16), num_heads=12,
                 num_layers=12, mlp_factor=4.0, act=None, embed_dim=512, use_summary_token=False, use_local_prompts=False,
                 use_global_prompts=False, num_global_prompts=8):
        super().__init__()
        if not (use_summary_token and use_local_prompts and use_global_prompts):
            raise NotImplementedError("only use_summary_token=use_local_prompts=use_global_prompts=True is a working "
                                      "configuration of the reference (VitaCLIP_vision_encoder.py:123-124,129)")
        if isinstance(input_size, int):
            input_size = (input_size, input_size)
        if isinstance(patch_size, int):
            patch_size = (patch_size, patch_size)
        self.feature_dim = feature_dim
        self.num_frames = num_frames
        self._hip_shape = dict(size=input_size[0], P=patch_size[0], D=feature_dim, H=num_heads, layers=num_layers,
                               F=round(mlp_factor * feature_dim), E=embed_dim, G=num_global_prompts)
        self.patch_embed = _PatchEmbed(patch_size[0], feature_dim)
        self.num_patches = int(np.prod([x // y for x, y in zip(input_size, patch_size)])) + 1
        self.cls_token = nn.Parameter(torch.zeros([feature_dim]))
        self.pos_embed = nn.Parameter(torch.zeros([self.num_patches, feature_dim]))
        self.time_embed = nn.Parameter(torch.zeros([num_frames, feature_dim]))
        self.blocks = nn.ModuleList([TransformerEncoderLayer(feature_dim, num_heads, mlp_factor, num_frames, patch_size)
                                     for _ in range(num_layers)])
        self.ln_pre = LayerNorm(feature_dim)
        self.ln_post = LayerNorm(feature_dim)
        self.proj = nn.Parameter(feature_dim ** -0.5 * torch.randn(feature_dim, embed_dim))
        self.use_global_prompts = True
        self.num_global_prompts = num_global_prompts
        self.global_prompts = nn.Parameter(torch.zeros(num_layers, num_global_prompts, feature_dim))
        val = math.sqrt(6. / float(3 * patch_size[0] * patch_size[1] + feature_dim))
        nn.init.uniform_(self.global_prompts.data, -val, val)
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.time_embed, std=0.02)

    def forward(self, x):
        return self._host().encode_video(x)


class _MHAParams(_Params):
    """Parameter layout of nn.MultiheadAttention (packed in_proj), VitaCLIP_text_encoder.py:71."""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.)


class ResidualAttentionBlock(_Params):
    def __init__(self, width):
        super().__init__()
        self.attn = _MHAParams(width)
        self.ln_1 = LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, width * 4)), ("gelu", nn.Identity()),
                                              ("c_proj", nn.Linear(width * 4, width))]))
        self.ln_2 = LayerNorm(width)


class Transformer(_Params):
    def __init__(self, width, layers):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width) for _ in range(layers)])


class CLIPTextEncoder(_Encoder):
    """VitaCLIP_text_encoder.py:120-143.  positional_embedding / text_projection are
    ``torch.empty`` upstream (uninitialised without a checkpoint); here they get the CLIP
    initialisers so that a random-weight model is finite."""

    def __init__(self, embed_dim=512, context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                 transformer_layers=12):
        super().__init__()
        self._hip_shape = dict(W=transformer_width, TH=transformer_heads, TL=transformer_layers, L=context_length,
                               E=embed_dim, n_ctx=0)
        self.context_length = context_length
        self.transformer = Transformer(transformer_width, transformer_layers)
        self.heads = transformer_heads
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        nn.init.normal_(self.positional_embedding, std=0.01)
        nn.init.normal_(self.text_projection, std=transformer_width ** -0.5)

    def forward(self, prompts, tokenized_prompts):
        """(n, L, W) prompt embeddings + (n, L) token ids -> (n, E) (VitaCLIP_text_encoder.py:154-171)."""
        return self._host().encode_prompt_embeddings(prompts, tokenized_prompts)


class ContextualPromptLearner(nn.Module):
    """Knowledge-aware prompts, training/kapt_head.py:24-214, in the configuration that works upstream and that the
    reference's training scripts use (train_scripts/updrs_3cls_train_tulip.sh:31-36): `cntn_split_uni[_disc]`, one
    bias-free two-layer MLP per class (768 -> W/4 -> W, zero-initialised, kapt_head.py:127-133,161) applied to the
    class's KEPLER entity embeddings, one prompt per knowledge version (n_kv).  Reads the same files as upstream,
    relative to the working directory: ./data/ke_<type>/EntityEmb_<kv>.npy, simQdesc_<kv>.txt (kapt_head.py:60,94-112).
    This small module (n_cls * n_kv rows) is evaluated by torch; its output joins the context vectors that enter the
    HIP text tower, and its gradients come back through TextTowerFn."""

    def __init__(self, use_cntn, cntn_split, uni_mlp, use_disc, emb_dim, out_dim, inp_dim=768, n_cls=4, n_tokens=16,
                 cls_type="updrs", knowledge_version=("v0",), use_descriptor=False, token_wise_mlp=False):
        super().__init__()
        if token_wise_mlp:   # upstream: asserts against class_wise_mlp=True (kapt_head.py:63) and reads an unbound idc (:201)
            raise NotImplementedError("KAPT: token_wise_mlp=True does not run in the reference")
        if not (use_cntn and cntn_split and uni_mlp):
            # upstream: without `split` ke_v0_path is read before assignment (kapt_head.py:91), without `uni` a Python
            # list is .expand()-ed (:187-191), without `cntn` a 2-D ctx is concatenated with 3-D prefixes (text_encoder.py:325)
            raise NotImplementedError("KAPT: only text_prompt_init with cntn+split+uni (optionally disc) runs in the reference")
        assert len(knowledge_version) > 0 or use_descriptor, "No knowledge is specified."
        self.type = cls_type.lower().split("_")[0]
        self.n_cls, self.n_tokens = n_cls, n_tokens
        self.use_descriptor = use_descriptor
        self.updrs_ke_dir = f"./data/ke_{self.type}"
        assert os.path.isdir(self.updrs_ke_dir), f"{self.updrs_ke_dir} (KEPLER knowledge files) not found"
        embeds = torch.empty(n_cls, 0, inp_dim)
        cls_disc = [[] for _ in range(n_cls)]
        if use_descriptor:
            # per-class descriptors instead of one description per knowledge version (kapt_head.py:65-88): class c has as
            # many prompts as descriptor_<c>.txt has lines, each with its own entity embedding (descriptor_<c>.npy)
            np.load(os.path.join(self.updrs_ke_dir, "all.npy"), allow_pickle=False)     # read upstream as well (:68)
            embeds = []
            for idc in range(n_cls):
                with open(os.path.join(self.updrs_ke_dir, f"descriptor_{idc}.txt")) as f:
                    cls_disc[idc] = [ln.strip() for ln in f]
                ent = np.load(os.path.join(self.updrs_ke_dir, f"descriptor_{idc}.npy"), allow_pickle=False)
                assert ent.shape[0] == len(cls_disc[idc])
                embeds.append(torch.from_numpy(ent).float())
            knowledge_version = ()
        for kv in knowledge_version:
            ent = np.load(os.path.join(self.updrs_ke_dir, f"EntityEmb_{kv}.npy"), allow_pickle=False)[:n_cls]
            embeds = torch.cat([embeds, torch.from_numpy(ent).float().unsqueeze(1)], dim=1)
            if use_disc:
                with open(os.path.join(self.updrs_ke_dir, f"simQdesc_{kv}.txt")) as f:
                    lines = [ln.strip() for ln in f]
                for idc in range(n_cls):
                    cls_disc[idc].append(lines[idc])
            else:
                for idc in range(n_cls):
                    cls_disc[idc].append("")
        self.projector = nn.ModuleList([nn.Sequential(nn.Linear(inp_dim, emb_dim, bias=False), nn.ReLU(inplace=True),
                                                      nn.Linear(emb_dim, out_dim, bias=False)) for _ in range(n_cls)])
        for m in self.projector.modules():
            if isinstance(m, nn.Linear):
                nn.init.zeros_(m.weight)
        self.cntn_embeds = list(embeds)          # plain attribute like upstream (:166-167): n_cls x (n_kv, inp_dim)
        self.cls_disc = cls_disc

    def forward(self, ctx_prompt):
        """(n_cls, N, W) context parameters -> list of n_cls tensors (n_kv, N, W) (kapt_head.py:177-214)."""
        prompts = []
        for idc in range(self.n_cls):
            e = self.cntn_embeds[idc] = self.cntn_embeds[idc].to(ctx_prompt.device)
            emb = self.projector[idc](e).unsqueeze(1).expand(-1, self.n_tokens, -1)
            prompts.append(ctx_prompt[idc].unsqueeze(0) + emb)
        return prompts


class TextPromptLearner(_Params):
    """VitaCLIP_text_encoder.py:174-332: class-specific context vectors, plain ("X X ... name.") or knowledge-aware."""

    def __init__(self, classnames, text_model, num_prompts, prompts_init="", CSC=False, ctx_pos="end", cls_type="updrs",
                 knowledge_version=("v0",), use_descriptor=False, token_wise_mlp=False):
        super().__init__()
        ctx_init = prompts_init.lower()
        assert ctx_init == "" or set(ctx_init.split("_")).issubset({"split", "uni", "cntn", "disc"}), "Invalid prompt initialization"
        if ctx_pos != "end":
            raise NotImplementedError(f"Unsupported class token position: {ctx_pos}")
        n_cls, n_ctx = len(classnames), num_prompts
        ctx_dim = text_model.ln_final.weight.shape[0]
        self.knowledge_aware_prompt = ctx_init != ""
        names = [name.replace("_", " ") for name in classnames]
        if self.knowledge_aware_prompt:
            flags = set(ctx_init.split("_"))
            self.context_prompt_learner = ContextualPromptLearner(
                use_cntn="cntn" in flags, cntn_split="split" in flags, uni_mlp="uni" in flags, use_disc="disc" in flags,
                emb_dim=ctx_dim // 4, out_dim=ctx_dim, n_cls=n_cls, n_tokens=n_ctx, cls_type=cls_type,
                knowledge_version=list(knowledge_version), use_descriptor=use_descriptor, token_wise_mlp=token_wise_mlp)
            self.ctx = nn.Parameter(torch.zeros(n_cls, n_ctx, ctx_dim))                      # :218-220
            if use_descriptor:                                                               # :253-255
                texts = [[d + " " + names[c] for d in self.context_prompt_learner.cls_disc[c]] for c in range(n_cls)]
            else:
                texts = [[self.context_prompt_learner.cls_disc[c][k] + " " + names[c] for k in range(len(knowledge_version))]
                         for c in range(n_cls)]                                              # :256-258
        else:
            if not CSC:
                # upstream: a generic (n_ctx, dim) ctx is unsqueezed to (n_ctx,1,dim) and cannot be
                # concatenated (text_encoder.py:317,325-332) -> only CSC=True works there either.
                raise NotImplementedError("text_prompt_CSC=False is broken in the reference (SURVEY.md §7.5); use CSC=True")
            ctx = torch.empty(n_cls, n_ctx, ctx_dim)
            nn.init.normal_(ctx, std=0.02)
            self.ctx = nn.Parameter(ctx)
            texts = [[t] for t in prompt_texts(classnames, n_ctx)]
        # list of (n_kv, 77) int tensors, one per class, like upstream (:266-270)
        self.tokenized_prompts = [torch.from_numpy(np.concatenate([tokenize(t, text_model.context_length) for t in ts]))
                                  for ts in texts]
        assert max(int((tp == 49407).nonzero()[:, -1].max()) for tp in self.tokenized_prompts) <= 77, \
            "The tokenized prompt is too long"
        self.n_cls, self.n_ctx = n_cls, n_ctx
        # prompts per class: uniform (n_kv knowledge versions) or ragged (use_descriptor); n_kv is None when ragged
        self.kv_counts = [int(tp.shape[0]) for tp in self.tokenized_prompts]
        self.n_kv = self.kv_counts[0] if len(set(self.kv_counts)) == 1 else None
        self.class_token_position = ctx_pos

    def embedding_token_ids(self):
        """(n_cls*n_kv, L) token ids in the order their EMBEDDINGS sit in the prompt: [SOS | n_ctx context slots | rest].
        Plain prompts carry "X" placeholders at the context slots, so this is the tokenised text itself (:300);
        knowledge-aware prompts have no placeholders - upstream inserts the context after SOS and drops the last n_ctx
        positions (`embedding[:, 1:-n_ctx]`, :298), i.e. every later token moves n_ctx places to the right.  The EOT
        look-up keeps using the un-shifted ids (:169 with tokenized_prompts) - reproduced as is."""
        tok = torch.cat(self.tokenized_prompts)
        if not self.knowledge_aware_prompt:
            return tok
        eff = tok.clone()
        eff[:, 1 + self.n_ctx:] = tok[:, 1:tok.shape[1] - self.n_ctx]
        return eff

    def full_context(self):
        """(n_cls*n_kv, n_ctx, W) context rows of every prompt (text_encoder.py:310-317)."""
        if self.knowledge_aware_prompt:
            return torch.cat(self.context_prompt_learner(self.ctx), dim=0)
        return self.ctx


class _HipHost:
    """Weight packing and tower launches on libgava_hip.so, shared by VitaCLIP and by stand-alone encoders.  Expects
    `visual` and / or `textual` attributes (parameter containers), `num_frames`, and the nn.Module parameter iterators."""

    # the auxiliary heads' route, refused where it is set (train_head, its sibling, is read on every training forward and is
    # checked there; this one may not be read for many calls - the heads run only when memory / video_nte are passed)
    @property
    def aux_heads(self):
        return self._aux_heads

    @aux_heads.setter
    def aux_heads(self, route):
        if route not in ("torch", "hip"):
            raise hip.GavaError(f"aux_heads must be 'torch' or 'hip', got {route!r}")
        self._aux_heads = route

    def _hip_init(self, shape, operand_dtype=None):
        operand_dtype = operand_dtype or os.environ.get("GAVA_PREC", "fp16")
        self.prec, self.w_lo = self._parse_operand_dtype(operand_dtype)
        # text tower GEMMs in split precision (hi+lo operands, 3 MFMA passes): the text side is <1 % of
        # the work at the headline configs but dominates the logits error at plain 16-bit operands
        self.text_split_precision = os.environ.get("GAVA_TEXT_SPLIT", "1") != "0"
        # with it (inference): q/k/v leave their GEMM in fp32 and the softmax core runs in fp32 - the text features then carry
        # no 16-bit rounding at all (GAVA_TEXT_ATTN_F32=0: the MFMA attention on 16-bit q/k/v, as in rounds 1-2)
        self.text_attention_fp32 = os.environ.get("GAVA_TEXT_ATTN_F32", "1") != "0"
        # eval-time text-feature cache: in eval mode the text tower is input
        # independent; opt-in because a benchmark must not skip work.  Invalidated by any parameter update.
        self.cache_text_features = False
        self.text_on_side_stream = os.environ.get("GAVA_TEXT_STREAM", "1") != "0"
        # inference: LayerNorm folded into the qkv / fc1 GEMMs (two row passes per block less); GAVA_LN_FOLD=0 turns it off
        self.fold_layernorm = os.environ.get("GAVA_LN_FOLD", "1") != "0"
        self.trim_text_rows = os.environ.get("GAVA_TEXT_TRIM", "1") != "0"   # skip the rows behind the last EOT (see _pack)
        # inference, opt-in: the last block's B*T CLS rows (the only ones that reach the outputs) in split precision.
        # Measured at c1 (tools/archive/r2_diag.py): video-feature rms error 2.06e-5 with, 2.10e-5 without - the error of the
        # features is made in the fp16 K/V and in the eleven blocks before, not here - so it is off by default.
        self.split_last_block = os.environ.get("GAVA_LAST_SPLIT", "0") != "0"
        self.text_rows_per_prompt = shape.get("L", 77)
        # training: keep the backward's activations (~21 GB at B = 64, T = 8) instead of recomputing them per block, as
        # long as they fit this budget; beyond it the backward recomputes from the block inputs only
        self.keep_activation_bytes = int(float(os.environ.get("GAVA_KEEP_ACT_GB", "96")) * 2 ** 30)
        # the similarity head under autograd: "torch" = traced torch ops (_train_head), "hip" = training.HeadFn (gava_train_head)
        self.train_head = os.environ.get("GAVA_TRAIN_HEAD", "torch")
        self._head_offsets = (None, None)
        # the auxiliary NTE and support-memory heads: "torch" = traced torch ops, "hip" = training.NteHeadFn / MemoryHeadFn
        self.aux_heads = os.environ.get("GAVA_AUX_HEADS", "torch")
        self._mem_table = (None, None)
        self._text_stream = None
        self._text_cache = None
        self.gather_across_ranks = True     # RCCL all-gather of clip embeddings when world_size > 1
        self.shard_text_across_ranks = True  # eval, world_size > 1: each rank encodes a slice of the prompts (+ all-gather)
        self.debug_taps = False             # keep per-layer CLS rows of the last forward
        self._shape = dict(shape)
        self._packed = None
        self._packed_key = None
        self._bwd_packs = {}
        self._ws = {}
        self.last = {}

    # ---- weight packing -----------------------------------------------------------------------
    @staticmethod
    def _parse_operand_dtype(name):
        """"fp16" | "bf16", optionally "+wlo" / "+wlo8": the weight-lo pass of the vision tower in inference (include/gava_hip.h,
        gava_gemm_args.w_lo; DESIGN.md "Numerics") - the 16-bit rounding of the frozen weights is what misses north_star's 1e-3
        on some models, so every vision GEMM also multiplies by W - h16(W): "+wlo" as a second 16-bit k-loop over the
        re-read activations, "+wlo8" at 8 bits (block-scaled MFMA, twice the rate) for the four full-width GEMMs of a block."""
        base, _, mode = name.partition("+")
        if mode not in ("", "wlo", "wlo8") or base not in hip.PREC_NAMES:
            raise ValueError(f"operand_dtype must be fp16 | bf16 [+wlo | +wlo8], got {name!r}")
        if mode == "wlo8" and hip.PREC_NAMES[base] != hip.PREC_F16:
            raise ValueError("the 8-bit weight-lo pass takes its bf8 activations from fp16 operands: use fp16+wlo8")
        return hip.PREC_NAMES[base], {"": 0, "wlo": 1, "wlo8": 2}[mode]

    def set_operand_dtype(self, name: str):
        self.prec, self.w_lo = self._parse_operand_dtype(name)
        self._packed = None

    _PASS_THROUGH = ("prompt_learner.", "logit_scale", "global_prompts", "local_prompts", "token_embedding",
                     "pos_embed", "time_embed", "positional_embedding", "cls_token", "sum_proj", "tf_project",
                     "memory_project")

    def _pack_key(self):
        """Changes when a packed 16-bit copy goes stale.  fp32 pass-through parameters (prompts, embeddings, LN
        affines, biases: the structs hold pointers into their own storage) only count by address, so an optimizer
        step on the prompt parameters does not re-convert 180 M frozen weights."""
        ver, addr = 0, 0
        for name, p in self.named_parameters():
            addr ^= p.data_ptr()
            if p.dim() >= 2 and not p.requires_grad and not any(k in name for k in self._PASS_THROUGH):
                ver += p._version
        if self.fold_layernorm and hasattr(self, "visual"):   # norm1 / norm2 affines and the qkv / fc1 biases are baked into the folded copies
            for blk in self.visual.blocks:
                for q in (blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias, blk.attn.q_proj.bias,
                          blk.attn.k_proj.bias, blk.attn.v_proj.bias, blk.mlp.fc1.bias):
                    ver += q._version
        ps = next(self.parameters())
        return (self.prec, self.w_lo, self.text_split_precision, self.trim_text_rows, self.fold_layernorm, self.split_last_block,
                ps.device, addr, ver)

    def _summary_weight_versions(self):
        """Versions of the only TRAINABLE weights that have 16-bit copies (summary_attn_layer projections): an optimizer
        step refreshes just those copies in place (same device pointers) instead of re-converting every frozen weight."""
        if not hasattr(self, "visual"):
            return []
        return [tuple(w._version for w in (b.summary_attn_layer.q_proj.weight, b.summary_attn_layer.k_proj.weight,
                                           b.summary_attn_layer.v_proj.weight, b.summary_attn_layer.out_proj.weight,
                                           b.summary_attn_layer.q_proj.bias, b.summary_attn_layer.k_proj.bias,
                                           b.summary_attn_layer.v_proj.bias))
                for b in self.visual.blocks]

    def _refresh_summary_weights(self, packed):
        cur = self._summary_weight_versions()
        if cur == packed["summary_ver"]:
            return
        for i, blk in enumerate(self.visual.blocks):
            if cur[i] != packed["summary_ver"][i]:
                s_ = blk.summary_attn_layer
                packed["w_sqkv"][i].copy_(self._h16(torch.cat([s_.q_proj.weight, s_.k_proj.weight, s_.v_proj.weight], 0)))
                packed["w_sout"][i].copy_(self._h16(s_.out_proj.weight))
                packed["b_sqkv"][i].copy_(torch.cat([s_.q_proj.bias, s_.k_proj.bias, s_.v_proj.bias], 0).detach().float())
                if "w_sqkv_wlo" in packed:
                    packed["w_sqkv_wlo"][i].copy_(self._hl16(torch.cat([s_.q_proj.weight, s_.k_proj.weight, s_.v_proj.weight], 0)))
                    packed["w_sout_wlo"][i].copy_(self._hl16(s_.out_proj.weight))
                    packed["b_sqkv_wlo"][i].copy_(torch.cat([s_.q_proj.bias, s_.k_proj.bias, s_.v_proj.bias], 0).detach().float())
        packed["summary_ver"] = cur

    def _backward_pack(self, tower):
        """The training backward's bf16 weight copies of `tower` ("text" | "vision"; training.pack_*_backward), remade when
        the pack key changes.  The vision side's trainable copies are brought up to date on every use."""
        from . import training
        key = self._pack_key()
        if self._bwd_packs.get(tower, (None,))[0] != key:
            self._bwd_packs[tower] = (key, getattr(training, f"pack_{tower}_backward")(self))
        if tower == "vision":
            training.refresh_vision_backward(self, self._bwd_packs[tower][1])
        return self._bwd_packs[tower][1]

    def _h16(self, t):
        return hip.convert_h16(t.detach().float(), self.prec)

    def _f32(self, t):
        return t.detach().float().contiguous()

    def _pack(self):
        key = self._pack_key()
        if self._packed is not None and self._packed_key == key:
            self._refresh_summary_weights(self._packed)
            return self._packed
        sh = self._shape
        keep = []  # tensors referenced by raw pointers in the structs
        w_sqkv_t, w_sout_t, b_sqkv_t = [], [], []

        def K(t):
            keep.append(t)
            return C.c_void_p(t.data_ptr())

        packed = dict(keep=keep, summary_ver=self._summary_weight_versions())
        if hasattr(self, "visual"):
            self._pack_vision(packed, K, w_sqkv_t, w_sout_t, b_sqkv_t)
        if hasattr(self, "textual"):
            self._pack_text(packed, K)
        self._packed, self._packed_key = packed, key
        return packed

    def _hl16(self, t):
        """[N][K] fp32 -> [N][2K] h16 = [W_hi | W_lo], W_lo = h16(W - W_hi): the weight side of gava_gemm_args.w_lo = 1."""
        t = t.detach().float().contiguous()
        hi = hip.convert_h16(t, self.prec)
        return torch.cat([hi, hip.convert_h16(t - hi.float(), self.prec)], dim=1).contiguous()

    def _pack_vision(self, packed, K, w_sqkv_t, w_sout_t, b_sqkv_t):
        self._pack_vision_set(packed, K, w_sqkv_t, w_sout_t, b_sqkv_t, 0)
        if self.w_lo:
            # inference with the weight-lo pass: a second set of structs whose 16-bit weights are [W_hi | W_lo]; the training
            # drivers keep using the plain set (fp32 pass-through tensors are shared by address: K() dedups nothing, they are views)
            self._pack_vision_set(packed, K, [], [], [], self.w_lo)

    def _pack_vision_set(self, packed, K, w_sqkv_t, w_sout_t, b_sqkv_t, w_lo):
        sh, v = self._shape, self.visual
        h16 = self._hl16 if w_lo else self._h16
        Kp = (3 * sh["P"] ** 2 + 63) // 64 * 64
        wpatch = v.patch_embed.proj.weight.detach().float().reshape(sh["D"], -1)
        if Kp != wpatch.shape[1]:
            wpatch = F.pad(wpatch, (0, Kp - wpatch.shape[1]))
        vis = dict(w_patch=K(h16(wpatch)), b_patch=K(self._f32(v.patch_embed.proj.bias)),
                   cls_token=K(self._f32(v.cls_token)), pos_embed=K(self._f32(v.pos_embed)),
                   lnpre_g=K(self._f32(v.ln_pre.weight)), lnpre_b=K(self._f32(v.ln_pre.bias)),
                   lnpost_g=K(self._f32(v.ln_post.weight)), lnpost_b=K(self._f32(v.ln_post.bias)),
                   w_proj=K(hip.split_pack_weight(v.proj.detach().float().t(), self.prec)))
        layers = (hip.VisionLayer * sh["layers"])()
        layers8 = (hip.VisionLayer8 * sh["layers"])() if (w_lo == 2 and self.fold_layernorm) else None
        for i, blk in enumerate(v.blocks):
            a, s = blk.attn, blk.summary_attn_layer
            L = layers[i]
            if layers8 is not None:
                _, w8, e8, _s = hip.pack_w8(blk.mlp.fc2.weight, self.prec)
                layers8[i].w_fc28, layers8[i].fc2_exp = K(w8), e8
            L.w_qkv = K(h16(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0)))
            L.b_qkv = K(self._f32(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0)))
            L.w_out, L.b_out = K(h16(a.out_proj.weight)), K(self._f32(a.out_proj.bias))
            L.w_fc1, L.b_fc1 = K(h16(blk.mlp.fc1.weight)), K(self._f32(blk.mlp.fc1.bias))
            L.w_fc2, L.b_fc2 = K(h16(blk.mlp.fc2.weight)), K(self._f32(blk.mlp.fc2.bias))
            L.ln1_g, L.ln1_b = K(self._f32(blk.norm1.weight)), K(self._f32(blk.norm1.bias))
            L.ln2_g, L.ln2_b = K(self._f32(blk.norm2.weight)), K(self._f32(blk.norm2.bias))
            if self.fold_layernorm:
                # LayerNorm folded into the consumer GEMM (inference driver): W' = h16(gamma * W),
                # s = row sums of the ROUNDED W', t = W beta + b in fp32
                wq = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().float()
                bq = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().float()
                for tag, w0, b0, nrm in (("qkv", wq, bq, blk.norm1), ("fc1", blk.mlp.fc1.weight.detach().float(),
                                                                     blk.mlp.fc1.bias.detach().float(), blk.norm2)):
                    gam, bet = nrm.weight.detach().float(), nrm.bias.detach().float()
                    wf = h16(w0 * gam)
                    if layers8 is not None:      # the 8-bit lo operand of the folded weight (gava_vision_layer8)
                        _, w8, e8, s8 = hip.pack_w8(w0 * gam, self.prec)
                        setattr(layers8[i], f"w_{tag}_fold8", K(w8))
                        setattr(layers8[i], f"{tag}_fold_s8", K(s8))
                        setattr(layers8[i], f"{tag}_fold_exp", e8)
                    setattr(L, f"w_{tag}_fold", K(wf))
                    # ([W_hi | W_lo]: the row sum over both halves = the sum of the weight the kernel multiplies by)
                    setattr(L, f"{tag}_fold_s", K(wf.float().sum(1).contiguous()))
                    setattr(L, f"{tag}_fold_t", K((w0.double() @ bet.double() + b0.double()).float().contiguous()))
            if self.split_last_block and i == len(v.blocks) - 1:
                L.w_q_split = K(hip.split_pack_weight(a.q_proj.weight, self.prec))
                L.w_out_split = K(hip.split_pack_weight(a.out_proj.weight, self.prec))
                L.w_fc1_split = K(hip.split_pack_weight(blk.mlp.fc1.weight, self.prec))
                L.w_fc2_split = K(hip.split_pack_weight(blk.mlp.fc2.weight, self.prec))
            L.w_cls, L.b_cls = K(h16(blk.cls_proj.weight)), K(self._f32(blk.cls_proj.bias))
            L.sln_g, L.sln_b = K(self._f32(blk.summary_ln.weight)), K(self._f32(blk.summary_ln.bias))
            w_sqkv_t.append(h16(torch.cat([s.q_proj.weight, s.k_proj.weight, s.v_proj.weight], 0)))
            w_sout_t.append(h16(s.out_proj.weight))
            L.w_sqkv, L.w_sout = K(w_sqkv_t[-1]), K(w_sout_t[-1])
            b_sqkv_t.append(self._f32(torch.cat([s.q_proj.bias, s.k_proj.bias, s.v_proj.bias], 0)))
            L.b_sqkv = K(b_sqkv_t[-1])
            L.b_sout = K(self._f32(s.out_proj.bias))
            L.local_prompts = K(self._f32(blk.local_prompts[0]))
            L.global_prompts = K(self._f32(v.global_prompts[i]))
        if w_lo:
            packed.update(vis_wlo=vis, vis_layers_wlo=layers, w_sqkv_wlo=w_sqkv_t, w_sout_wlo=w_sout_t, b_sqkv_wlo=b_sqkv_t,
                          vis_layers8=layers8)
        else:
            packed.update(vis=vis, vis_layers=layers, w_sqkv=w_sqkv_t, w_sout=w_sout_t, b_sqkv=b_sqkv_t)

    def _pack_text(self, packed, K):
        sh = self._shape
        if True:
            t = self.textual
            tlayers = (hip.TextLayer * sh["TL"])()
            tw = (lambda w: hip.split_pack_weight(w, self.prec)) if self.text_split_precision else self._h16
            for i, blk in enumerate(t.transformer.resblocks):
                L = tlayers[i]
                L.w_qkv, L.b_qkv = K(tw(blk.attn.in_proj_weight)), K(self._f32(blk.attn.in_proj_bias))
                L.w_out, L.b_out = K(tw(blk.attn.out_proj.weight)), K(self._f32(blk.attn.out_proj.bias))
                L.w_fc, L.b_fc = K(tw(blk.mlp.c_fc.weight)), K(self._f32(blk.mlp.c_fc.bias))
                L.w_proj, L.b_proj = K(tw(blk.mlp.c_proj.weight)), K(self._f32(blk.mlp.c_proj.bias))
                L.ln1_g, L.ln1_b = K(self._f32(blk.ln_1.weight)), K(self._f32(blk.ln_1.bias))
                L.ln2_g, L.ln2_b = K(self._f32(blk.ln_2.weight)), K(self._f32(blk.ln_2.bias))
            packed.update(txt=dict(token_embedding=K(self._f32(t.token_embedding.weight)),
                                   positional_embedding=K(self._f32(t.positional_embedding)),
                                   lnf_g=K(self._f32(t.ln_final.weight)), lnf_b=K(self._f32(t.ln_final.bias)),
                                   w_tproj=K(tw(t.text_projection.detach().float().t().contiguous()))),
                          txt_layers=tlayers)
            if not getattr(self, "use_text_prompt_learning", False):
                return          # a bare text tower (direct calls only): no prompt learner, no token table
            dev = t.token_embedding.weight.device
            tok0 = torch.cat(self.tokenized_prompts).to(device=dev)
            eot_col = (tok0 == t.vocab_size - 1).nonzero()[:, -1]
            assert eot_col.numel() == tok0.shape[0], "every prompt must contain exactly one EOT token"
            # Causal attention: the EOT row - the only one the text features read (text_encoder.py:169) - depends on the
            # rows up to itself only, and LayerNorm / MLP are row-wise.  Rows behind the last EOT of any prompt are
            # dead work (the reference pads every prompt to 77): the tower runs on the first L_eff positions, results
            # identical.  ("X X .. name." prompts: ~15-20 of 77.)
            L_eff = min(sh["L"], max(int(eot_col.max()) + 1, 1 + sh["n_ctx"]))
            self.text_rows_per_prompt = L_eff if self.trim_text_rows else sh["L"]
            L_eff = self.text_rows_per_prompt
            eot = (torch.arange(tok0.shape[0], device=dev) * L_eff + eot_col).to(torch.int32).contiguous()
            tok = self.prompt_learner.embedding_token_ids()[:, :L_eff].to(device=dev, dtype=torch.int32).contiguous()
            packed.update(tokens=tok, eot=eot)

    def _workspace(self, tag, nbytes, device):
        ws = self._ws.get(tag)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._ws[tag] = ws
        return ws

    # ---- encoders -----------------------------------------------------------------------------
    def encode_video(self, x, saved=None, kept=None, clips=None):
        """CLIPVisionEncoder.forward on the HIP path -> (cls_x (B,E), summary (B,D)), fp32.
        saved: optional fp32 [layers+2, B*T*(n+1), D] that receives what the backward recomputes from;
        kept: optional dict of per-block activation buffers (training.alloc_kept) filled by gava_vision_forward_keep;
        clips: instead of x, the decoded uint8 videos as (descriptor tensor, B, T, normalisation table, device) - the patch embedding
        then reads the frames themselves (hip.clip_descriptors)."""
        if clips is None and not x.is_cuda:
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        lib = hip.load()
        pk, sh = self._pack(), self._shape
        if clips is not None:
            desc, B, T, lut, dev = clips
            x = desc            # only its device is used below
        else:
            B, Cc, T, Hh, Ww = x.shape
            assert Cc == 3 and Hh == sh["size"] and Ww == sh["size"], "input must be (B,3,T,size,size)"
            x = x.detach().float().contiguous()
        if B == 0:   # an empty batch is not an error upstream (every op of the reference accepts zero clips): empty features
            self.last["summary"] = torch.zeros(0, sh["D"], device=x.device)
            return torch.zeros(0, sh["E"], device=x.device), self.last["summary"]
        te = self.visual.time_embed.detach().float()
        if T != te.size(0):  # VitaCLIP_vision_encoder.py:91-95
            te = F.interpolate(te.unsqueeze(0).transpose(1, 2), size=(T), mode='nearest').transpose(1, 2).squeeze(0)
        te = te.contiguous()
        m = hip.VisionModel()
        m.B, m.T_in, m.T_model = B, T, self.num_frames
        for k in ("size", "P", "D", "H", "layers", "F", "E", "G"):
            setattr(m, k, sh[k])
        m.prec = self.prec
        wl = self.w_lo if (saved is None and kept is None) else 0      # the weight-lo pass is an inference mode
        for k, val in pk["vis_wlo" if wl else "vis"].items():
            setattr(m, k, val)
        m.time_embed = C.c_void_p(te.data_ptr())
        m.layer = C.cast(pk["vis_layers_wlo" if wl else "vis_layers"], C.POINTER(hip.VisionLayer))
        m.w_lo = wl
        if wl == 2 and pk.get("vis_layers8") is not None:
            m.layer8 = C.cast(pk["vis_layers8"], C.c_void_p)
        elif wl == 2:
            m.w_lo = 1            # no folded weights packed (fold_layernorm off): every lo product stays 16-bit
        if clips is not None:
            m.clips, m.clip_lut = hip.ptr(desc), hip.ptr(lut)
        nbytes = lib.gava_vision_workspace_bytes(C.byref(m))
        # (measurement / tests) does the inference driver keep the residual stream of this batch as a 16-bit pair?
        self.last["pair_stream"] = bool(saved is None and kept is None and lib.gava_vision_pair_stream(C.byref(m)))
        if nbytes == 0:
            raise hip.GavaError(f"unsupported vision shape: B={B} T={T} num_frames={self.num_frames} {sh}")
        ws = self._workspace("vision", nbytes, x.device)
        cls_x = torch.empty(B, sh["E"], dtype=torch.float32, device=x.device)
        summary = torch.empty(B * T // self.num_frames, sh["D"], dtype=torch.float32, device=x.device)
        dbg = torch.empty(sh["layers"], B * T, sh["D"], dtype=torch.float32, device=x.device) if self.debug_taps else None
        # the drivers key their side stream by the CURRENT device: make it the input's
        with torch.cuda.device(x.device):
            if kept is not None:
                sv = hip.VisionSaved(hip.ptr(kept["e0"]), hip.ptr(kept["x"]), hip.ptr(kept["x1"]), hip.ptr(kept["qkv"]),
                                     hip.ptr(kept["pre"]), hip.ptr(kept["sidekv"]), hip.ptr(kept.get("last_q")),
                                     hip.ptr(kept.get("last_x1")), hip.ptr(kept.get("last_pre")))
                hip.check(lib.gava_vision_forward_keep(C.byref(m), None if clips is not None else hip.ptr(x), hip.ptr(cls_x), hip.ptr(summary), C.byref(sv),
                                                       hip.ptr(ws), ws.numel(), hip.stream_ptr(x.device)), "gava_vision_forward_keep")
            else:
                hip.check(lib.gava_vision_forward_train(C.byref(m), None if clips is not None else hip.ptr(x), hip.ptr(cls_x), hip.ptr(summary), hip.ptr(dbg),
                                                        hip.ptr(saved), hip.ptr(ws), ws.numel(), hip.stream_ptr(x.device)),
                          "gava_vision_forward")
        self.last["cls_rows"] = dbg
        return cls_x, summary

    def _overlapping_stream(self, device):
        """A new stream that really runs BESIDE the current one.  HIP multiplexes streams onto a few hardware queues in creation
        order; a stream that shares the current stream's queue is served in order with it, and the text tower then runs serially
        in front of the vision tower (23.0 instead of 20.7 ms per c2 forward, profiles/r04_text_cost.txt) - which queue a new stream
        gets depends on how many the process has created before (data loaders, DDP).  So the candidate is tried once: a ~1 ms spin
        on the current stream, a one-element fill on the candidate; a candidate whose fill is not done long before the spin ends is
        set aside (kept alive, so that the next one gets another queue) and the next is tried, four at most."""
        if torch.cuda.is_current_stream_capturing():
            return torch.cuda.Stream(device=device)
        main = torch.cuda.current_stream(device)
        tried = []
        with torch.cuda.device(device):
            for _ in range(4):
                cand = torch.cuda.Stream(device=device)
                tried.append(cand)
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                with torch.cuda.stream(cand):
                    torch.zeros(1, device=device)                # first use of the stream (its queue is set up here), untimed
                torch.cuda.synchronize(device)
                e0.record(main)
                torch.cuda._sleep(2_000_000)
                e1.record(main)
                with torch.cuda.stream(cand):
                    torch.zeros(1, device=device)
                    e2.record(cand)
                torch.cuda.synchronize(device)
                if e2.elapsed_time(e1) > 0.3 * e0.elapsed_time(e1):     # the fill was done while the spin still had most of its time to go
                    break
        self._queue_sharing_streams = tried[:-1]
        self.last["text_stream_candidates"] = len(tried)
        return tried[-1]

    def _text_shard(self, n):
        """(lo, hi, rows per rank, world) when the prompts are sharded over the ranks, else None (SURVEY.md 8f row 2:
        every rank would otherwise run the whole text tower redundantly - 2.4 TF per forward at 400 classes)."""
        import torch.distributed as dist
        if not (self.shard_text_across_ranks and self.gather_across_ranks and not torch.is_grad_enabled()
                and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return None
        world, rank = dist.get_world_size(), dist.get_rank()
        if n < 2 * world:
            return None
        per = (n + world - 1) // world
        return min(n, rank * per), min(n, (rank + 1) * per), per, world

    def encode_text(self):
        """prompt_learner() + textual(...) for all classes in one batch -> (C, E) fp32.  With several ranks (eval) each
        rank encodes a contiguous slice of the prompts and the rows are all-gathered: prompts are independent, so the
        result is the same as every rank encoding all of them."""
        pk, sh = self._pack(), self._shape
        n = pk["tokens"].shape[0]
        shard = self._text_shard(n)
        if shard is None:
            return self._encode_text_rows(0, n)
        lo, hi, per, world = shard
        part = torch.zeros(per, sh["E"], dtype=torch.float32, device=pk["tokens"].device)
        if hi > lo:
            part[:hi - lo] = self._encode_text_rows(lo, hi)
        # rank r holds prompts [r*per, (r+1)*per): the rank-major concatenation is already in prompt order, padding last
        return self._gather(part)[:n].contiguous()

    def _text_model(self, n, L, n_ctx):
        pk, sh = self._pack(), self._shape
        m = hip.TextModel()
        m.n_prompts, m.L, m.W, m.H, m.layers = n, L, sh["W"], sh["TH"], sh["TL"]
        m.E, m.n_ctx, m.prec = sh["E"], n_ctx, self.prec
        m.split = int(self.text_split_precision)
        m.attn_f32 = int(self.text_split_precision and self.text_attention_fp32)
        for k, val in pk["txt"].items():
            setattr(m, k, val)
        m.layer = C.cast(pk["txt_layers"], C.POINTER(hip.TextLayer))
        return m

    def _run_text(self, m, tok, ctx, eot, device):
        lib = hip.load()
        nbytes = lib.gava_text_workspace_bytes(C.byref(m))
        if nbytes == 0:
            raise hip.GavaError(f"unsupported text shape: n={m.n_prompts} L={m.L} {self._shape}")
        ws = self._workspace("text", nbytes, device)
        out = torch.empty(m.n_prompts, self._shape["E"], dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            hip.check(lib.gava_text_forward(C.byref(m), hip.ptr(tok), hip.ptr(ctx), hip.ptr(eot), hip.ptr(out),
                                            hip.ptr(ws), ws.numel(), hip.stream_ptr(device)), "gava_text_forward")
        return out

    def _encode_text_rows(self, lo, hi):
        """The text tower on prompts [lo, hi)."""
        pk, sh = self._pack(), self._shape
        L = self.text_rows_per_prompt
        tok = pk["tokens"][lo:hi].contiguous()
        ctx = self.prompt_learner.full_context().detach().float()[lo:hi].contiguous()
        eot = (pk["eot"][lo:hi] - lo * L).to(torch.int32).contiguous()      # flat row index n*L + column, rebased to the slice
        return self._run_text(self._text_model(tok.shape[0], L, sh["n_ctx"]), tok, ctx, eot, tok.device)

    def encode_prompt_embeddings(self, prompts, tokenized_prompts):
        """CLIPTextEncoder.forward(prompts, tokenized_prompts) (VitaCLIP_text_encoder.py:154-171) on ready-made prompt
        embeddings (n, L, W) - the call of evaluation/zero_shot.py:75-76 and utils/prepare_embedding.py - through the
        HIP text tower's direct mode (no token table, no context splice).  Inference only: training goes through
        VitaCLIP.forward, whose TextTowerFn owns the backward."""
        if not prompts.is_cuda:
            raise hip.GavaError("CLIPTextEncoder (gava_clip_amd) runs on the HIP device only; there is no CPU fallback")
        if torch.is_grad_enabled() and prompts.requires_grad:
            raise hip.GavaError("CLIPTextEncoder.forward called stand-alone has no backward: train through VitaCLIP.forward")
        self._pack()
        tok = tokenized_prompts.to(prompts.device)
        n, L, W = prompts.shape
        assert tuple(tok.shape) == (n, L) and W == self._shape["W"] and L <= self._shape["L"]
        hit = (tok == self.textual.vocab_size - 1).nonzero()
        assert hit.shape[0] == n, "every prompt must contain exactly one EOT token"      # text_encoder.py:169
        eot_col = hit[:, -1]
        L_eff = int(eot_col.max()) + 1 if self.trim_text_rows else L        # rows behind the last EOT are dead work (causal)
        x = prompts.detach().float()[:, :L_eff].contiguous()
        eot = (torch.arange(n, device=tok.device) * L_eff + eot_col).to(torch.int32).contiguous()
        return self._run_text(self._text_model(n, L_eff, 0), None, x, eot, prompts.device)


class _StandaloneHost(_HipHost):
    """Host of an encoder that was constructed on its own (evaluation/zero_shot.py:42-52 builds a bare CLIPTextEncoder,
    evaluation/iwa.py a bare CLIPVisionEncoder): packs that encoder's weights and launches its tower."""

    def __init__(self, enc):
        self._enc = weakref.ref(enc)
        self.use_text_prompt_learning = False
        if isinstance(enc, CLIPVisionEncoder):
            self.num_frames = enc.num_frames
        self._hip_init(enc._hip_shape)

    def __getattr__(self, name):      # `visual` / `textual` resolve to the encoder without keeping it alive (no cycle)
        if name in ("visual", "textual"):
            enc = self.__dict__["_enc"]()
            if enc is not None and isinstance(enc, CLIPVisionEncoder if name == "visual" else CLIPTextEncoder):
                return enc
        raise AttributeError(name)

    def named_parameters(self):
        return self._enc().named_parameters()

    def parameters(self):
        return self._enc().parameters()


# ---------------------------------------------------------------------------------------------
class AttentionMaps:
    """What VitaCLIP.attention_maps returns: fp32 device tensors, B clips of T frames as given.
      mode, layer          what was asked for (layer: the block's index from 0; None for "rollout")
      patches [B, T, g, g] the CLS token's attention (or rollout) on the frame's patches, g = S / P
      cls     [B, T]       ... on the CLS token itself
      logits  [B, C]       the inference head on this forward's features
    and for mode "cls" (None for "rollout"; with heads=None every map carries a head axis after T):
      global_prompts [B, T, G], local_prompts [B, T, num_frames] (frame t's CLS on the local prompt of frame t' of its
      num_frames group), summary [B, T]; the five groups of a frame sum to 1."""
    __slots__ = ("mode", "layer", "patches", "cls", "logits", "global_prompts", "local_prompts", "summary")

    def __init__(self, mode, layer, patches, cls, logits, global_prompts=None, local_prompts=None, summary=None):
        self.mode, self.layer, self.patches, self.cls, self.logits = mode, layer, patches, cls, logits
        self.global_prompts, self.local_prompts, self.summary = global_prompts, local_prompts, summary

    def __repr__(self):
        shapes = ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__[2:] if getattr(self, k) is not None)
        return f"AttentionMaps(mode={self.mode!r}, layer={self.layer!r}, {shapes})"


class RelevanceMaps:
    """What VitaCLIP.relevance_maps returns: fp32 device tensors, B clips of T frames as given.
      patches [B, T, g, g] the relevance of the frame's patches for the target class, g = S / P; >= 0, not normalised
      cls     [B, T]       ... of the CLS token itself; >= 1
      logits  [B, C]       the raw logits of the forward that was differentiated
      target  [B]          int64: the class each clip was asked about"""
    __slots__ = ("patches", "cls", "logits", "target")

    def __init__(self, patches, cls, logits, target):
        self.patches, self.cls, self.logits, self.target = patches, cls, logits, target

    def __repr__(self):
        return "RelevanceMaps(" + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__) + ")"


class PerturbationCurves:
    """What VitaCLIP.perturbation_curves returns, B clips and S1 steps:
      mode                 "deletion" or "insertion"
      fractions [S1]       fp32 HOST tensor: the share of a ranking's units perturbed at each step (the curves' abscissae)
      logit     [B, S1]    fp32: the target's raw logit on the perturbed clip
      prob      [B, S1]    fp32: its softmax probability
      top1      [B, S1]    int32: the perturbed clip's top-1 class (lowest class on ties)
      auc_logit, auc_prob [B]  fp32: the areas under the two curves (trapezoids over fractions)
      target    [B]        int64: the class each clip was asked about
      ranks     [B, n]     int32: the ranking the perturbation followed, per unit in the scores' own order (0 = first)
    everything but fractions on the device."""
    __slots__ = ("mode", "fractions", "logit", "prob", "top1", "auc_logit", "auc_prob", "target", "ranks")

    def __init__(self, mode, fractions, logit, prob, top1, auc_logit, auc_prob, target, ranks):
        self.mode, self.fractions, self.logit, self.prob, self.top1 = mode, fractions, logit, prob, top1
        self.auc_logit, self.auc_prob, self.target, self.ranks = auc_logit, auc_prob, target, ranks

    def __repr__(self):
        return f"PerturbationCurves(mode={self.mode!r}, " + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__[1:]) + ")"


class PathAttribution:
    """What VitaCLIP.integrated_gradients returns, B clips of T frames as given; device tensors unless said otherwise:
      maps     fp32 [B, T, S, S] (reduce "sum", "abs", "absmax", "l2") or [B, 3, T, S, S] (reduce=None)
      logits   [B, C]      the raw logits of x itself (the path's last step)
      target   [B]         int64: the class each clip was asked about
      sum_attr [B]         fp32: the clip's summed attribution (None with multiply=False)
      delta    [B]         fp32: the completeness residual sum_attr - (f(x) - f(x0)) for the target's logit (None with
                           multiply=False); what is left is the quadrature's error and the bf16 gradient operands'
      alpha, w [m]         fp32 HOST tensors: the path's points and their weights, zero-weight endpoints included"""
    __slots__ = ("maps", "logits", "target", "sum_attr", "delta", "alpha", "w")

    def __init__(self, maps, logits, target, sum_attr, delta, alpha, w):
        self.maps, self.logits, self.target, self.sum_attr, self.delta, self.alpha, self.w = maps, logits, target, sum_attr, delta, alpha, w

    def __repr__(self):
        return "PathAttribution(" + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__ if getattr(self, k) is not None) + ")"


class Faithfulness(dict):
    """What VitaCLIP.faithfulness returns: {method: {"deletion": PerturbationCurves, "insertion": PerturbationCurves}}, the
    methods in the order asked for and the control "random" last.  table() is the text a user reads: per method the mean
    areas over the clips (a faithful map has a LOW deletion area and a HIGH insertion area; "random" is the floor to beat).
    table() copies the areas to the host, so it waits for the device; building the object does not."""

    def table(self):
        rows = [f"{'method':<12}{'del auc_prob':>14}{'ins auc_prob':>14}{'del auc_logit':>15}{'ins auc_logit':>15}"]
        for name, c in self.items():
            d, i = c["deletion"], c["insertion"]
            rows.append(f"{name:<12}{float(d.auc_prob.mean()):>14.4f}{float(i.auc_prob.mean()):>14.4f}"
                        f"{float(d.auc_logit.mean()):>15.4f}{float(i.auc_logit.mean()):>15.4f}")
        return "\n".join(rows)


class VitaCLIP(nn.Module, _HipHost):

    def __init__(
        self,
        backbone_path: str = '',
        input_size: Tuple[int, int] = (224, 224),
        num_frames: int = 16,
        use_fp16: bool = False,
        cls_type: str = 'updrs',
        num_classes: int = 4,
        feature_dim: int = 768,
        patch_size: Tuple[int, int] = (16, 16),
        num_heads: int = 12,
        num_layers: int = 12,
        mlp_factor: float = 4.0,
        embed_dim: int = 512,
        use_summary_token: bool = False,
        use_local_prompts: bool = False,
        use_global_prompts: bool = False,
        num_global_prompts: int = 8,
        use_text_prompt_learning: bool = False,
        text_context_length: int = 77,
        text_vocab_size: int = 49408,
        text_transformer_width: int = 512,
        text_transformer_heads: int = 8,
        text_transformer_layers: int = 12,
        text_num_prompts: int = 8,
        text_prompt_pos: str = 'end',
        text_prompt_init: str = '',
        text_prompt_CSC: bool = False,
        text_prompt_classes_path: str = '',
        knowledge_version: List[str] = ['v0'],
        use_descriptor: bool = False,
        token_wise_mlp: bool = False,
        zeroshot_evaluation: bool = False,
        zeroshot_text_features_path: str = '',
        use_support_memory: bool = False,
        detach_features: bool = False,
        memory_batch_size: int = 64,
        add_nte: bool = False,
        use_sigmoid_loss: bool = False,
        *,
        operand_dtype: str = None,
    ):
        super().__init__()
        if not (use_summary_token and use_local_prompts and use_global_prompts):
            # upstream's non-global-prompt branch assigns the block's tuple to x and leaves
            # `summary` undefined (VitaCLIP_vision_encoder.py:123-124,129): it cannot run.
            raise NotImplementedError("only use_summary_token=use_local_prompts=use_global_prompts=True is a "
                                      "working configuration of the reference (SURVEY.md §7.5)")
        if isinstance(input_size, int):
            input_size = (input_size, input_size)
        if isinstance(patch_size, int):
            patch_size = (patch_size, patch_size)
        self.fp16 = use_fp16
        self.num_frames = num_frames
        self.num_classes = num_classes
        self.text_context_length = text_context_length
        self.text_transformer_width = text_transformer_width
        self.use_summary_token = use_summary_token
        self.use_sigmoid_loss = use_sigmoid_loss
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.logit_bias = None
        self.zeroshot_evaluation = zeroshot_evaluation
        if self.zeroshot_evaluation:
            self.text_features = torch.load(zeroshot_text_features_path, map_location='cpu',
                                            weights_only=True)['text_features']
        self.visual = CLIPVisionEncoder(input_size=input_size, num_frames=num_frames, feature_dim=feature_dim,
                                        patch_size=patch_size, num_heads=num_heads, num_layers=num_layers,
                                        mlp_factor=mlp_factor, embed_dim=embed_dim, use_summary_token=True,
                                        use_local_prompts=True, use_global_prompts=True,
                                        num_global_prompts=num_global_prompts)
        self.use_text_prompt_learning = use_text_prompt_learning
        if self.use_text_prompt_learning:
            self.textual = CLIPTextEncoder(embed_dim, text_context_length, text_vocab_size, text_transformer_width,
                                           text_transformer_heads, text_transformer_layers)
        if backbone_path:
            ckpt = torch.load(backbone_path, map_location='cpu', weights_only=True)
            self.load_state_dict(ckpt, strict=False)

        self.use_support_memory = use_support_memory
        self.memoty_batch_size = memory_batch_size
        self.detach_features = detach_features
        self.add_nte = add_nte
        if self.add_nte:
            self.sum_proj = nn.Linear(feature_dim, embed_dim)
            self.logit_scale_vm = nn.Parameter(torch.ones([]) * (np.log(10.) if use_sigmoid_loss else 100.))
        if self.use_support_memory:
            def _mlp():
                return nn.Sequential(nn.Linear(embed_dim, embed_dim // 4), nn.Tanh(), nn.Linear(embed_dim // 4, embed_dim // 8))
            self.tf_project = _mlp()
            self.memory_project = nn.ModuleList([_mlp() for _ in range(num_classes)])
            if use_sigmoid_loss:
                self.logit_scale_mt = nn.Parameter(torch.ones([]) * np.log(10.))
                self.logit_bias_mt = nn.Parameter(torch.ones([]) * -10.)
            else:
                self.logit_scale_mt = nn.Parameter(torch.ones([]) * 100.)
                self.logit_bias_mt = None
        if use_sigmoid_loss:
            self.logit_scale = nn.Parameter(torch.ones([]) * np.log(np.log(10.)))
            self.logit_bias = nn.Parameter(torch.ones([]) * -10.)

        if self.use_text_prompt_learning:
            classes = read_class_names(text_prompt_classes_path)
            self.prompt_learner = TextPromptLearner(classnames=classes, text_model=self.textual,
                                                    num_prompts=text_num_prompts, prompts_init=text_prompt_init,
                                                    CSC=text_prompt_CSC, ctx_pos=text_prompt_pos, cls_type=cls_type,
                                                    knowledge_version=knowledge_version, use_descriptor=use_descriptor,
                                                    token_wise_mlp=token_wise_mlp)
            self.tokenized_prompts = self.prompt_learner.tokenized_prompts

        # freeze (VitaCLIP_model.py:222-239)
        for name, param in self.visual.named_parameters():
            if not ('summary' in name or 'local' in name or 'global' in name or 'time_embed' in name):
                param.requires_grad = False
        if hasattr(self, "textual"):
            for param in self.textual.named_parameters():
                param[1].requires_grad = False

        # ---- HIP-path state (not part of the reference surface)
        self._hip_init(dict(size=input_size[0], P=patch_size[0], D=feature_dim, H=num_heads, layers=num_layers,
                            F=round(mlp_factor * feature_dim), E=embed_dim, G=num_global_prompts,
                            W=text_transformer_width, TH=text_transformer_heads, TL=text_transformer_layers,
                            L=text_context_length, n_ctx=text_num_prompts), operand_dtype)
        self._attach_encoders()

    def _attach_encoders(self):
        """The L1 encoders stay callable on their own (evaluation/iwa.py:212, zero_shot.py:75): they run on this host."""
        self.visual.__dict__["_host_ref"] = weakref.ref(self)
        if hasattr(self, "textual"):
            self.textual.__dict__["_host_ref"] = weakref.ref(self)

    def _gather(self, feats):
        """RCCL all-gather over xGMI of the per-clip embeddings (north_star): each rank
        holds whole clips, every rank ends with the embeddings (and logits) of the global batch.
        Contract: with an initialised process group of world size N and grad disabled, forward() returns
        logits of shape (N*B, C), rank-major; `local_logits()` gives a rank its own B rows - what the reference's
        evaluate() loops index with their local labels (training/train.py:661-670).  Under autograd nothing is gathered
        (every rank keeps its own clips, as the reference's DDP does)."""
        import torch.distributed as dist
        if not (self.gather_across_ranks and dist.is_available() and dist.is_initialized()
                and dist.get_world_size() > 1):
            return feats
        feats = feats.contiguous()
        # all_gather_into_tensor needs the same number of rows on every rank: checked once per row count (a 1-int
        # all-gather), so that a ragged last batch fails with a message instead of corrupting the gathered matrix
        checked = self.__dict__.setdefault("_gather_checked", set())
        if feats.shape[0] not in checked:
            mine = torch.tensor([feats.shape[0]], dtype=torch.int64, device=feats.device if dist.get_backend() != "gloo" else "cpu")
            rows = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
            dist.all_gather(rows, mine)
            if any(int(r) != feats.shape[0] for r in rows):
                raise hip.GavaError(f"gather_across_ranks needs the same batch size on every rank, got {[int(r) for r in rows]}; "
                                    "pad the last batch or set model.gather_across_ranks = False")
            checked.add(feats.shape[0])
        if dist.get_backend() == "gloo" and feats.is_cuda:
            # CPU rendezvous (tests on a single-GPU box): stage through the host
            out = torch.empty(dist.get_world_size() * feats.shape[0], feats.shape[1], dtype=feats.dtype)
            dist.all_gather_into_tensor(out, feats.cpu())
            return out.to(feats.device)
        out = torch.empty(dist.get_world_size() * feats.shape[0], feats.shape[1], dtype=feats.dtype, device=feats.device)
        dist.all_gather_into_tensor(out, feats)
        return out

    def local_logits(self, logits):
        """Rows of this rank in the gathered logits (identity when nothing was gathered)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return logits
        b = logits.shape[0] // dist.get_world_size()
        return logits if logits.shape[0] == self.last.get("local_batch", -1) else logits[dist.get_rank() * b:(dist.get_rank() + 1) * b]

    def _class_mean_matrix(self, device):
        """(n_prompts, n_cls) matrix with 1/count_c in the rows of class c's prompts: flat logits @ A = per-class means."""
        counts = self.prompt_learner.kv_counts
        A = torch.zeros(sum(counts), len(counts), dtype=torch.float32, device=device)
        r = 0
        for c, k in enumerate(counts):
            A[r:r + k, c] = 1.0 / k
            r += k
        return A

    def _vision_trainables(self):
        """Ordered (name, parameter) list of the vision-side parameters the reference leaves trainable."""
        return [(n, p) for n, p in self.visual.named_parameters()
                if ("summary" in n or "local" in n or "global" in n or "time_embed" in n)]

    def _memory_head_hip(self, memory, text_features):
        """The support-memory head as one autograd node (training.MemoryHeadFn; aux_heads = "hip").  memory_project's
        parameters reach the kernels through a device table of their pointers, rebuilt only when a pointer changes."""
        from .training import MemoryHeadFn
        params = list(self.tf_project.parameters()) + [q for mp in self.memory_project for q in mp.parameters()]
        if not torch.is_tensor(memory) or not memory.is_cuda:
            raise hip.GavaError("memory must be a tensor on the HIP device: the auxiliary heads have no CPU fallback")
        key = (tuple(q.data_ptr() for q in params[4:]), memory.device)
        if self._mem_table[0] != key:
            self._mem_table = (key, hip.pointer_table(params[4:], memory.device))
        return MemoryHeadFn.apply(memory, text_features, self.logit_scale_mt, self.logit_bias_mt, self._mem_table[1], *params)

    def _train_head(self, video, text, summary, desc_wise):
        """Similarity head under autograd (VitaCLIP_model.py:248,255,287-293,308-309): 2*B*C*E flop on (B,E)/(C,E)
        tensors, traced by torch so that d logits reaches the text tower's backward and logit_scale."""
        assert not desc_wise
        vf = video / video.norm(dim=-1, keepdim=True)
        tf = text / text.norm(dim=-1, keepdim=True)
        logits = self.logit_scale.exp() * vf @ tf.t()
        n_kv = self.prompt_learner.n_kv if self.use_text_prompt_learning else 1
        if n_kv is None:                               # ragged (use_descriptor): per-class means by an averaging matrix
            A = self._class_mean_matrix(tf.device)
            logits, tf = logits @ A, A.t() @ tf
        elif n_kv > 1:                                 # VitaCLIP_model.py:288-290
            logits = logits.view(logits.shape[0], -1, n_kv).mean(-1)
            tf = tf.view(-1, n_kv, tf.shape[-1]).mean(1)
        if self.logit_bias is not None:
            logits = logits + self.logit_bias
        self.text_features = tf / tf.norm(dim=-1, keepdim=True)
        self.last.update(video_features=vf.detach(), summary=summary.detach())
        return logits

    def _train_head_hip(self, video, text, summary, desc_wise):
        """_train_head as one autograd node over the HIP head (training.HeadFn; train_head = "hip"): the same logits,
        text_features and `last` entries, the backward in two launches.  last["head_fn_calls"] counts its uses."""
        from .training import HeadFn
        assert not desc_wise
        counts = self.prompt_learner.kv_counts if self.use_text_prompt_learning else [1] * text.shape[0]
        key = (tuple(counts), video.device)
        if self._head_offsets[0] != key:
            off = [0]
            for k in counts:
                off.append(off[-1] + int(k))
            self._head_offsets = (key, torch.tensor(off, dtype=torch.int32).to(video.device))
        if text.shape[0] != sum(counts):
            raise hip.GavaError(f"{text.shape[0]} prompt features for {sum(counts)} prompts")
        logits, self.text_features = HeadFn.apply(video, text, self.logit_scale, self.logit_bias, self._head_offsets[1])
        self.last.update(video_features=logits.grad_fn.saved_tensors[HeadFn.SAVED.index("video_norm")], summary=summary.detach(),
                         head_fn_calls=self.last.get("head_fn_calls", 0) + 1)
        return logits

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, memory=None, video_nte=None, desc_wise=False):
        if not x.is_cuda:
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        # every launch below names "the current stream": make the input's device the current one (a model on cuda:k
        # called without torch.cuda.set_device(k) would otherwise launch on another device's stream)
        with torch.cuda.device(x.device):
            return self._forward_impl(x, memory, video_nte, desc_wise)

    def forward_frames(self, videos, preprocessor, memory=None, video_nte=None, desc_wise=False):
        """forward() on DECODED videos instead of a preprocessed batch: `videos` is a list of uint8 device tensors
        [n_i, H_i, W_i, 3] (PyAV's to_rgb().to_ndarray() order), `preprocessor` a gava_clip_amd.preprocess.ClipPreprocessor
        (video_dataset/dataset.py:117-139, the branch the reference evaluates AND trains with: its train loader sets
        random_sample=False, dataloader.py:89-102) or a TrainClipPreprocessor (the random-sample branch, :93-114, which
        draws its frames and crop box here, one sample() per video in batch order).  The patch embedding reads the frames
        themselves (frame selection, normalisation, bilinear resize and crop per loaded pixel): same logits, bit for bit,
        as forward(preprocessor.batch(videos)) wherever forward() takes the two-pass patch embedding too (big batches;
        small fp32 batches take the im2col-free GEMM, equal to the rounding of its 16-bit operands), without the fp32 clip
        ever being written to HBM - 4x fewer input bytes.

        Training: on a model in train() mode this runs under autograd like forward() - loss.backward() reaches every
        trainable parameter; the videos themselves get no gradient.  The backward never re-reads the input, in either
        activation mode (kept activations, or GAVA_KEEP_ACT_GB=0: recomputation from the saved fp32 input of every
        block, the first of which is the embedding's output): `videos` may be released as soon as this call returns.
        A model in eval() mode with grad enabled is refused: that is the evaluation path with a forgotten
        torch.no_grad(), which would keep every block's activations alive."""
        if torch.is_grad_enabled() and not self.training:
            raise hip.GavaError("forward_frames on a model in eval() mode is the evaluation data path: call it under "
                                "torch.no_grad(), or put the model in train() mode to train through it")
        pre = preprocessor
        assert pre.spatial_size == self._shape["size"], "the preprocessor's crop size must be the model's input size"
        dev = videos[0].device
        with torch.cuda.device(dev):
            pre.check(videos)
            desc, keep = pre.descriptors([v.contiguous() for v in videos])
            clips = (desc, len(videos), pre.num_frames, pre.lut(dev), dev)
            # (`keep` - the contiguous videos and the frame tables - lives until the patch embedding is enqueued, no longer)
            return self._forward_impl(desc, memory, video_nte, desc_wise, clips=clips)

    def forward_views(self, videos, preprocessor, max_clips=None):
        """Multi-view evaluation: every one of the preprocessor's V = num_spatial_views x num_temporal_views crops of every
        video (video_dataset/dataset.py:135-136,160-199; the views dataloader.py:31-34 asks for and dataset.py:137-139 drops)
        through the towers, and the fused view scores of evaluation/evaluate.py:283 - softmax over the classes per view,
        mean over a video's views.  `videos` as for forward_frames, `preprocessor` a ClipPreprocessor.
        -> (scores fp32 [B, C], logits fp32 [B, V, C], top1 int32 [B] = argmax of scores, lowest class on ties).

        Evaluation only: call it under torch.no_grad() on a model in eval() mode.  The patch embedding reads the uint8
        frames of each crop itself (as forward_frames does); clips go through in chunks of whole videos, by default the
        most videos whose clips x frames fit one launch's grid (65535 frames).  `max_clips` lowers that - one launch's
        workspace grows with its clip count - rounded down to a multiple of V and never below V.  The text features are
        cached for the duration of the call (cache_text_features is restored afterwards), so the text tower runs once, not
        once per chunk.  The call ends with one gava_view_scores launch and never waits for the device.

        Several ranks: each rank passes its own videos (the same number on every rank); the all-gather inside the forward
        returns every rank's clips in rank order, so logits is [B_global, V, C] and scores / top1 cover the global batch,
        rank-major, as forward()'s logits do."""
        from .preprocess import ClipPreprocessor
        if torch.is_grad_enabled() or self.training:
            raise hip.GavaError("forward_views is the evaluation path: call it under torch.no_grad() on a model in eval() mode")
        pre = preprocessor
        if not isinstance(pre, ClipPreprocessor):
            raise hip.GavaError("forward_views takes a ClipPreprocessor (the evaluation branch builds the views; the random-sample "
                                "branch has none)")
        assert pre.spatial_size == self._shape["size"], "the preprocessor's crop size must be the model's input size"
        if not videos:
            raise ValueError("forward_views needs at least one video")
        B, V, T = len(videos), pre.num_views, pre.num_frames
        fit = hip.MAX_GRID_FRAMES // T // V * V
        if fit < V:
            raise hip.GavaError(f"one video's {V} views x {T} frames are past the {hip.MAX_GRID_FRAMES} frames one launch covers")
        step = fit if max_clips is None else min(fit, max(int(max_clips) // V * V, V))
        dev = videos[0].device
        cached = self.cache_text_features
        self.cache_text_features = True
        try:
            with torch.cuda.device(dev):
                pre.check(videos)
                desc, keep, _ = pre.view_descriptors([v.contiguous() for v in videos])
                stride = desc.numel() // (B * V)
                logits = None
                for i in range(0, B * V, step):
                    n = min(step, B * V - i)
                    clips = (desc[i * stride:(i + n) * stride], n, T, pre.lut(dev), dev)
                    lg = self._forward_impl(clips[0], None, None, False, clips=clips)[0]
                    if n == B * V:
                        logits = lg.view(-1, V, lg.shape[-1])
                        break
                    world = lg.shape[0] // n               # ranks whose clips the forward gathered (1 without a process group)
                    if logits is None:
                        logits = torch.empty(world * B, V, lg.shape[-1], dtype=torch.float32, device=dev)
                    logits.view(world, B, V, -1)[:, i // V:(i + n) // V] = lg.view(world, n // V, V, -1)
                self.last["local_batch"] = B
                scores, top1 = hip.view_scores(logits)
        finally:
            self.cache_text_features = cached
        return scores, logits, top1

    _SALIENCY_MODES = {None: hip.UNPATCH_GRAD, "absmax": hip.UNPATCH_ABSMAX, "l2": hip.UNPATCH_L2, "grad_x_input": hip.UNPATCH_GRAD_X_INPUT}

    def saliency(self, x, target=None, reduce="absmax"):
        """Which pixels and frames of the clips moved a class score: the gradient of sum_b logits[b, target_b] (the raw
        logits) with respect to x, through the HIP backward of the frozen vision tower.
        -> (maps, logits [B, C], target int64 [B]); maps is fp32 [B, T, S, S], per pixel over the three channels
             reduce="absmax"        max_c |g_c|
             reduce="l2"            sqrt(sum_c g_c^2)
             reduce="grad_x_input"  sum_c g_c x_c
        or, with reduce=None, the gradient itself, fp32 [B, 3, T, S, S] - the bits x.grad gets from forward(x) followed by
        the same backward.  The map modes fold the patch gradients straight into the map (gava_unpatchify): the full-size
        gradient is never in memory.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it; it need not require grad (decoded uint8 videos:
        preprocess with `preprocessor.batch(videos)` first).  target: None - the top-1 class of this very forward, picked on the
        device -, an int (checked against the number of classes on the host), or an int64 [B] device tensor, which is NOT
        range-checked (a check would wait for the device; an index outside [0, C) is a device-side fault).
        Works on a model in eval() or train() mode, whatever is trainable; no parameter's .grad is touched, no graph and no
        kept activation survives the call, and the call itself never waits for the device.  memory / video_nte / desc_wise
        have no part in it; a ragged (use_descriptor) head is refused.  With an initialised process group every rank works
        on its own clips, as every grad-enabled forward does."""
        if reduce not in self._SALIENCY_MODES:
            raise hip.GavaError(f"saliency: reduce must be one of 'absmax', 'l2', 'grad_x_input' or None, got {reduce!r}")
        if not (torch.is_tensor(x) and x.is_cuda):
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        if not (x.dim() == 5 and x.is_floating_point()):
            raise hip.GavaError(f"saliency takes a floating-point clip batch [B, 3, T, S, S], got {x.dtype} {tuple(x.shape)}")
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError("saliency: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class to differentiate")
        n_cls = self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]
        if target is not None and not torch.is_tensor(target):
            if not 0 <= int(target) < n_cls:
                raise hip.GavaError(f"saliency: target {target} is outside the {n_cls} classes")
        elif target is not None and not (target.is_cuda and target.dtype == torch.int64 and tuple(target.shape) == (x.shape[0],)):
            raise hip.GavaError(f"saliency: a tensor target must be int64 [{x.shape[0]}] on the device")
        mode = self._SALIENCY_MODES[reduce]
        with torch.cuda.device(x.device), torch.enable_grad():
            xg = x.detach().float().contiguous().requires_grad_()       # a leaf of this call's own: x is left alone
            request = dict(mode=mode, x=xg.detach() if mode == hip.UNPATCH_GRAD_X_INPUT else None)
            logits = self._forward_impl(xg, None, None, False, input_request=request)[0]
            if target is None:
                target = logits.detach().argmax(dim=1)
            elif not torch.is_tensor(target):
                target = torch.full((x.shape[0],), int(target), dtype=torch.int64, device=x.device)
            score = logits.gather(1, target.view(-1, 1)).sum()
            (dx,) = torch.autograd.grad(score, [xg], allow_unused=True)      # runs the vision tower's backward, nothing else
        if torch.is_tensor(self.text_features) and self.text_features.requires_grad:
            self.text_features = self.text_features.detach()        # the last reference into this call's graph
        return (dx if mode == hip.UNPATCH_GRAD else request.pop("out")), logits.detach(), target

    _IG_MODES = {(True, "sum"): hip.PATH_ATTR_SUM, (True, "abs"): hip.PATH_ATTR_ABS, (True, None): hip.PATH_ATTR,
                 (False, None): hip.PATH_GRAD, (False, "absmax"): hip.PATH_ABSMAX, (False, "l2"): hip.PATH_L2}
    _SMOOTH_MODES = {None: hip.PATH_GRAD, "absmax": hip.PATH_ABSMAX, "l2": hip.PATH_L2}

    def _path_checks(self, what, x, target, m, max_clips, baseline="zero", noise=False):
        """The refusals integrated_gradients and smooth_grad share, the device's last -> (B, T, clips per chunk)."""
        S = self._shape["size"]
        if not (torch.is_tensor(x) and x.dim() == 5 and x.is_floating_point() and x.shape[1] == 3 and x.shape[3] == x.shape[4] == S
                and x.shape[0] > 0 and x.shape[2] > 0):
            raise hip.GavaError(f"{what} takes a floating-point clip batch [B, 3, T, {S}, {S}], got "
                                f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        B, T = x.shape[0], x.shape[2]
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError(f"{what}: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class to differentiate")
        n_cls = self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]
        if target is not None and not torch.is_tensor(target):
            if not 0 <= int(target) < n_cls:
                raise hip.GavaError(f"{what}: target {target} is outside the {n_cls} classes")
        elif target is not None and not (target.dtype == torch.int64 and tuple(target.shape) == (B,)):
            raise hip.GavaError(f"{what}: a tensor target must be int64 [{B}] on the device")
        if isinstance(max_clips, bool) or not isinstance(max_clips, int) or max_clips < 1:
            raise hip.GavaError(f"{what}: max_clips must be an int >= 1, got {max_clips!r}")
        if m * T > hip.MAX_GRID_FRAMES:
            raise hip.GavaError(f"{what}: one clip's {m} copies x {T} frames are past the {hip.MAX_GRID_FRAMES} frames one launch covers")
        if noise and S % 2:
            raise hip.GavaError(f"{what}: noise is drawn four floats at a time, an odd size {S} is not supported")
        kind = baseline if isinstance(baseline, str) else "tensor"
        if kind not in ("zero", "blur", "tensor") or (kind == "tensor" and not (
                torch.is_tensor(baseline) and baseline.is_floating_point() and (tuple(baseline.shape) == (3,) or baseline.shape == x.shape))):
            raise hip.GavaError(f"{what}: baseline must be 'zero', 'blur', a floating-point tensor [3] or one shaped like x, got "
                                f"{(baseline.dtype, tuple(baseline.shape)) if torch.is_tensor(baseline) else baseline!r}")
        if not x.is_cuda or (torch.is_tensor(target) and not target.is_cuda):
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        return B, T, max(1, min(max_clips, hip.MAX_GRID_FRAMES // T) // m)

    def _path_maps(self, x, make_copies, mode, w, target, ref_step, step, base=None, signed=None):
        """The body integrated_gradients and smooth_grad share: `step` clips at a time, make_copies(i, nb) -> the m = len(w)
        copies of clips [i, i + nb), fp32 [nb, m, 3, T, S, S]; the grad-enabled forward of the nb * m clips; the vision tower's
        backward with the path request, whose fold (gava_unpatchify_path) reduces each clip's m gradients with the weights w
        straight into the chunk's slice of the result.  target: int64 [B] or None - then the top-1 class of each clip's copy
        ref_step, picked on the device.  base: the baseline of the ATTR modes (None, [3] or shaped like x); signed: an fp32
        [B, T, S, S] tensor that also receives the PATH_ATTR_SUM map (a second fold of the same patch gradients).
        -> (maps, logits fp32 [B * m, C], target int64 [B])."""
        B, _, T, S, _ = x.shape
        m = len(w)
        attr = mode >= hip.PATH_ATTR
        shape = (B, 3, T, S, S) if mode in (hip.PATH_GRAD, hip.PATH_ATTR) else (B, T, S, S)
        maps = torch.empty(shape, dtype=torch.float32, device=x.device)
        aligned = lambda t: t if t.data_ptr() % 16 == 0 else t.clone()        # (a slice of clips of an odd size)
        logits, targets = None, []
        for i in range(0, B, step):
            nb = min(step, B - i)
            dst = [maps[i:i + nb]] + ([signed[i:i + nb]] if signed is not None else [])
            out = [d if d.data_ptr() % 16 == 0 else torch.empty_like(d) for d in dst]
            b = base[i:i + nb] if base is not None and base.dim() == 5 else base
            request = dict(mode=mode, m=m, w=w, out=out[0], signed=out[1] if signed is not None else None,
                           x=aligned(x[i:i + nb]) if attr else None,
                           baseline=(aligned(b) if b is not None and b.dim() == 5 else b) if attr else None)
            tg = target[i:i + nb] if target is not None else None
            with torch.enable_grad():
                xg = make_copies(i, nb).view(nb * m, 3, T, S, S).requires_grad_()       # a leaf of this call's own
                lg = self._forward_impl(xg, None, None, False, input_request=request)[0]
                if tg is None:
                    tg = lg.detach().view(nb, m, -1)[:, ref_step].argmax(dim=1)
                score = lg.gather(1, tg.repeat_interleave(m).view(-1, 1)).sum()
                torch.autograd.grad(score, [xg], allow_unused=True)      # runs the vision tower's backward, nothing else
            for d, o in zip(dst, out):
                if o is not d:
                    d.copy_(o)
            request.clear()
            lg = lg.detach()
            if nb == B:
                logits = lg
            else:
                if logits is None:
                    logits = torch.empty(B * m, lg.shape[-1], dtype=torch.float32, device=x.device)
                logits[i * m:(i + nb) * m] = lg
            targets.append(tg)
            del xg, score, lg
        if torch.is_tensor(self.text_features) and self.text_features.requires_grad:
            self.text_features = self.text_features.detach()        # the last reference into this call's graph
        return maps, logits, (target if target is not None else targets[0] if len(targets) == 1 else torch.cat(targets, 0))

    def integrated_gradients(self, x, target=None, baseline="zero", steps=16, rule="trapezoid", reduce="sum", multiply=True,
                             blur_sigma=5.0, max_clips=64):
        """Integrated gradients (Sundararajan et al., "Axiomatic Attribution for Deep Networks") of a class's raw logit along
        the straight path from a baseline x0 to the clip -> PathAttribution (see there for the fields):
          a = (x - x0) * sum_k w_k  d logit_target / d x (x0 + alpha_k (x - x0))
        The one map here with a checkable axiom: a clip's attributions sum to f(x) - f(x0) up to the quadrature's error, and
        .delta is that residual (what Captum calls the convergence delta).
          reduce="sum"  [B, T, S, S]  a_0 + a_1 + a_2, signed: what speaks FOR the class is positive
          reduce="abs"  [B, T, S, S]  |a_0| + |a_1| + |a_2|
          reduce=None   [B, 3, T, S, S]  a itself
        multiply=False returns the path-mean gradient G = sum_k w_k grad_k instead; reduce is then None ([B, 3, T, S, S]),
        "absmax" or "l2" (saliency's map rules on G), and sum_attr / delta are None.
        baseline: as for perturbation_curves - "zero", "blur" (blur_sigma), an fp32 tensor [3] or one shaped like x.
        rule="trapezoid": m = steps >= 2 points alpha_k = k / (m - 1), end weights halved; x0 and x are steps 0 and m - 1, so
        f(x0) and f(x) come with the path.  rule="gausslegendre": the `steps` Gauss-Legendre nodes on [0, 1] - exact for
        polynomials of degree 2 steps - 1, where the trapezoid's error falls as 1 / m^2 - plus the two endpoints as zero-weight
        steps (m = steps + 2): their forwards and backwards add nothing to the map and are the price of the residual.
        target: None - the top-1 class of the clip itself, the alpha = 1 row of the same forward, picked on the device -, an
        int (checked on the host) or an int64 [B] device tensor (not range-checked; out of range: NaN sum_attr and delta).
        The m copies of a clip are written by one kernel (gava_path_clips), go through the grad-enabled forward and the
        vision tower's backward as a batch, and the fold reduces their m patch gradients into the clip's one map
        (gava_unpatchify_path): the m full-size gradients are never in memory.  max(1, max_clips // m) whole clips run at a
        time; a chunk's copies (4.8 MB each at 224 px and T = 8) and kept activations are in memory at once.
        Works in eval() and train() mode and under no_grad (the call enables grad for itself); no parameter's .grad is
        touched, nothing survives the call, nothing waits for the device.  A per-descriptor head is refused."""
        what = "integrated_gradients"
        if (bool(multiply), reduce) not in self._IG_MODES:
            raise hip.GavaError(f"{what}: reduce must be 'sum', 'abs' or None (multiply=False: None, 'absmax' or 'l2'), got {reduce!r}")
        mode = self._IG_MODES[(bool(multiply), reduce)]
        alpha, w = hip.path_rule(rule, steps)
        m = len(alpha)
        kind = baseline if isinstance(baseline, str) else "tensor"
        taps = hip.gaussian_taps(blur_sigma) if kind == "blur" else None
        B, T, step = self._path_checks(what, x, target, m, max_clips, baseline=baseline)
        dev, P = x.device, self._shape["P"]
        with torch.cuda.device(dev):
            x = x.detach().float().contiguous()
            if kind == "zero":
                base = None
            elif kind == "blur":
                # the few dozen taps go up from pinned memory on the stream: a pageable copy would be the call's one host wait
                base = hip.blur_clips(x, taps.pin_memory().to(dev, non_blocking=True))
            else:
                base = baseline.detach().to(dev).float().contiguous()
            if target is not None and not torch.is_tensor(target):
                target = torch.full((B,), int(target), dtype=torch.int64, device=dev)
            copies = lambda i, nb: hip.path_clips(x[i:i + nb], patch=P, alpha=alpha,
                                                  baseline=base[i:i + nb] if base is not None and base.dim() == 5 else base)
            signed = None
            if multiply and reduce != "sum":
                signed = torch.empty(B, T, x.shape[3], x.shape[4], dtype=torch.float32, device=dev)
            maps, logits, target = self._path_maps(x, copies, mode, w, target, m - 1, step, base=base, signed=signed)
            sum_attr = delta = None
            if multiply:
                d = hip.path_delta(maps if signed is None else signed, logits, target.contiguous(), m=m, k_lo=0, k_hi=m - 1)
                sum_attr, delta = d["sum_attr"], d["delta"]
            logits = logits.view(B, m, -1)[:, m - 1].contiguous()
        return PathAttribution(maps, logits, target, sum_attr, delta, torch.tensor(alpha, dtype=torch.float32), torch.tensor(w, dtype=torch.float32))

    def smooth_grad(self, x, target=None, samples=16, sigma=0.15, relative=True, seed=0, reduce="absmax", max_clips=64):
        """SmoothGrad (Smilkov et al., "SmoothGrad: removing noise by adding noise"): the mean over `samples` noisy copies
        x + sigma_b z, z ~ N(0, 1), of the gradient saliency() takes -> (maps, logits [B, C] of x itself, target int64 [B]),
        like saliency; maps is fp32 [B, T, S, S] (reduce="absmax" / "l2", saliency's map rules on the MEAN gradient) or the mean
        gradient itself, [B, 3, T, S, S] (reduce=None).
        sigma: with relative=True the noise level as a share of each clip's own max - min (gava_clip_range; the paper's 10-20 %),
        else absolute, in the normalised space clips live in.  The noise is counter-based (Philox4x32-10 keyed by `seed`,
        counted by clip, sample and element - gava_path_clips): a call repeats bit for bit, and neither the batch a clip
        arrives in nor max_clips changes its noise.  A clip that holds a NaN gets a NaN map.
        target: None - the top-1 class of x itself - an int or an int64 [B] device tensor, as for saliency.  The plain no-grad
        forward of x that gives `logits` (and that target) runs in every case, max_clips clips at a time (it keeps no
        activations).  Chunks, memory and the guarantees are
        integrated_gradients': max(1, max_clips // samples) clips at a time, the fold (gava_unpatchify_path) averages the
        copies' patch gradients on the way, no .grad is touched, nothing waits for the device."""
        what = "smooth_grad"
        if reduce not in self._SMOOTH_MODES:
            raise hip.GavaError(f"{what}: reduce must be 'absmax', 'l2' or None, got {reduce!r}")
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= hip.PATH_MAX_STEPS:
            raise hip.GavaError(f"{what}: samples must be an int in [1, {hip.PATH_MAX_STEPS}], got {samples!r}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (math.isfinite(sigma) and sigma >= 0):
            raise hip.GavaError(f"{what}: sigma must be a finite number >= 0, got {sigma!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise hip.GavaError(f"{what}: seed must be an int in [0, 2^64), got {seed!r}")
        m = samples
        B, T, step = self._path_checks(what, x, target, m, max_clips, noise=True)
        dev, P = x.device, self._shape["P"]
        with torch.cuda.device(dev):
            x = x.detach().float().contiguous()
            plain = min(max_clips, hip.MAX_GRID_FRAMES // T)        # the plain forward keeps nothing: max_clips clips at a time
            with torch.no_grad():
                logits = None
                for i in range(0, B, plain):
                    lg = self.local_logits(self._forward_impl(x[i:i + plain], None, None, False)[0])
                    if lg.shape[0] == B:
                        logits = lg
                        break
                    if logits is None:
                        logits = torch.empty(B, lg.shape[-1], dtype=torch.float32, device=dev)
                    logits[i:i + plain] = lg
                self.last["local_batch"] = B
            if target is None:
                target = logits.argmax(dim=1)
            elif not torch.is_tensor(target):
                target = torch.full((B,), int(target), dtype=torch.int64, device=dev)
            sg = hip.clip_range(x, float(sigma))[2] if relative else torch.full((B,), float(sigma), dtype=torch.float32, device=dev)
            copies = lambda i, nb: hip.path_clips(x[i:i + nb], patch=P, sigma=sg[i:i + nb], samples=m, seed=seed, clip0=i)
            maps, _, _ = self._path_maps(x, copies, self._SMOOTH_MODES[reduce], [1.0 / m] * m, target, 0, step)
        return maps, logits, target

    def attention_maps(self, x, mode="rollout", layer=-1, heads="mean", max_clips=None):
        """What the CLS token of every frame attends to -> AttentionMaps (see there for the fields).
          mode="rollout"  attention rollout of the CLS token through all blocks: row 0 of A^_L ... A^_1, A^_l = (I + mean_h
                          A_l,h) / 2, A_l,h = block l's probabilities restricted to the frame's own tokens (CLS + patches) and
                          renormalised per row - the prompt tokens are rebuilt in every block and carry no path between
                          blocks.  Run as a vector chain from the last block to the first (gava_attention_mass, one launch
                          per block; no matrix product).  patches + cls sum to 1 per frame.  `layer` is ignored, `heads`
                          must be "mean".
          mode="cls"      the CLS row of block `layer` (negative: from the end) over ALL its keys, split by key group:
                          patches, cls, global_prompts, local_prompts, summary; heads="mean" averages over the heads,
                          heads=None keeps them as an axis after T.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it (decoded uint8 videos: `preprocessor.batch(videos)`
        first).  T need not be num_frames: the blocks regroup the B*T frames by the model's num_frames, and so do the local
        prompts' columns.
        The clips run through the activation-keeping forward of the training path (encode_video(kept=...)) under no_grad,
        in chunks of whole num_frames groups whose kept activations (training.kept_bytes) fit keep_activation_bytes;
        max_clips sets the clips per chunk instead.  The buffers are reused from chunk to chunk.  `logits` come from the
        inference head on THIS forward's features: the kept forward packs its operands plainly (no weight-lo pass, no
        16-bit residual pair), so they can differ from forward()'s within the operand rounding.
        Works in eval() and train() mode; no .grad is touched, no graph is left, nothing waits for the device.  With an
        initialised process group every rank keeps its own clips.  A per-descriptor (use_descriptor) head is refused."""
        from . import training
        if mode not in ("rollout", "cls"):
            raise hip.GavaError(f"attention_maps: mode must be 'rollout' or 'cls', got {mode!r}")
        if heads not in ("mean", None):
            raise hip.GavaError(f"attention_maps: heads must be 'mean' or None, got {heads!r}")
        if mode == "rollout" and heads is None:
            raise hip.GavaError("attention_maps: rollout averages over the heads in every block (heads='mean'); per-head maps are mode='cls'")
        sh, Tm = self._shape, self.num_frames
        NL, D, H, G = sh["layers"], sh["D"], sh["H"], sh["G"]
        if mode == "cls":
            if not (isinstance(layer, int) and -NL <= layer < NL):
                raise hip.GavaError(f"attention_maps: layer {layer!r} is outside the {NL} blocks")
            layer = layer % NL
        else:
            layer = None
        if not (torch.is_tensor(x) and x.dim() == 5 and x.is_floating_point() and x.shape[1] == 3 and x.shape[3] == x.shape[4] == sh["size"]):
            raise hip.GavaError(f"attention_maps takes a floating-point clip batch [B, 3, T, {sh['size']}, {sh['size']}], got "
                                f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        if not x.is_cuda:
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError("attention_maps: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class")
        B, T = x.shape[0], x.shape[2]
        unit = Tm // math.gcd(T, Tm)                  # the fewest clips that are whole num_frames groups
        if B == 0 or B % unit:
            raise hip.GavaError(f"attention_maps: {B} clips of {T} frames are not whole groups of num_frames = {Tm}")
        g = sh["size"] // sh["P"]
        n1 = g * g + 1
        n_all = n1 + G + Tm + 1
        if n_all > hip.ATTENTION_MASS_MAX_KEYS:
            raise hip.GavaError(f"attention_maps: {n_all} keys per frame, gava_attention_mass takes at most {hip.ATTENTION_MASS_MAX_KEYS}")
        if max_clips is None:
            step = B // unit * unit
            while step > unit and training.kept_bytes(self, step, T) > self.keep_activation_bytes:
                step = (step // unit + 1) // 2 * unit
        else:
            step = min(B, max(int(max_clips) // unit * unit, unit))
        dev = x.device
        mass = dict(heads=H, n_kmain=n1, prec=self.prec, n_g=G, T=Tm, has_summary=True)
        with torch.cuda.device(dev), torch.no_grad():
            self._attach_encoders()
            self._pack()
            kept = training.alloc_kept(self, step, T, dev)
            video = torch.empty(B, sh["E"], dtype=torch.float32, device=dev)
            maps = torch.empty((B * T, n1) if mode == "rollout" else (B * T, H, n_all), dtype=torch.float32, device=dev)
            for i in range(0, B, step):
                nb = min(step, B - i)
                kb = kept
                if nb != step:          # the last, smaller chunk: the same memory under that chunk's shapes
                    shapes = {k: v.shape for k, v in training.alloc_kept(self, nb, T, "meta").items()}
                    kb = {k: kept[k].view(-1)[:math.prod(shp)].view(shp) for k, shp in shapes.items()}
                video[i:i + nb] = self.encode_video(x[i:i + nb], kept=kb)[0]
                BT = nb * T
                keys = lambda l: dict(k=kb["qkv"][l][:, D:2 * D], side_k=kb["sidekv"][l][:, :D])
                out = maps[i * T:(i + nb) * T]
                if mode == "cls":
                    if layer == NL - 1:     # the kept last block has its CLS queries only, in a buffer of their own
                        hip.attention_mass(kb["last_q"], out=out, batch=BT, n_q=1, q_batch_rows=1, **keys(layer), **mass)
                    else:
                        hip.attention_mass(kb["qkv"][layer][:, :D], out=out, batch=BT, n_q=1, q_batch_rows=n1, **keys(layer), **mass)
                    continue
                r = hip.attention_mass(kb["last_q"], batch=BT, n_q=1, q_batch_rows=1, renorm=True, **keys(NL - 1), **mass).mean(1).mul_(0.5)
                r[:, 0] += 0.5              # r = e_cls / 2 + mean_h A_L[0] / 2
                for l in range(NL - 2, -1, -1):
                    o = hip.attention_mass(kb["qkv"][l][:, :D], batch=BT, n_q=n1, w=r, renorm=True, **keys(l), **mass)
                    r = (0.5 * r).add_(o.mean(1), alpha=0.5)
                out.copy_(r)
            logits = self._maps_logits(video)
        if mode == "rollout":
            m = maps.view(B, T, n1)
            return AttentionMaps(mode, None, m[..., 1:].reshape(B, T, g, g), m[..., 0], logits)
        m = (maps.mean(1) if heads == "mean" else maps).view(B, T, *(() if heads == "mean" else (H,)), n_all)
        return AttentionMaps(mode, layer, m[..., 1:n1].reshape(*m.shape[:-1], g, g), m[..., 0], logits,
                             global_prompts=m[..., n1:n1 + G], local_prompts=m[..., n1 + G:n1 + G + Tm], summary=m[..., n_all - 1])

    def relevance_maps(self, x, target=None, max_clips=None):
        """Which patches and frames of the clips speak FOR a class -> RelevanceMaps (patches [B, T, g, g], cls [B, T], logits
        [B, C], target [B]): gradient-weighted attention relevance (Chefer et al., "Generic Attention-model Explainability",
        the self-attention rule).  It is the class-specific counterpart of attention_maps(mode="rollout"), with every block's
        attention matrix replaced by  A-_l = mean_h max(0, grad A_l,h * A_l,h):
          A_l,h   block l's probabilities over ALL its keys, as the forward used them (not renormalised, unlike the rollout),
          grad    d s / d A_l,h for s = sum_b logits[b, target_b], the raw logits, as saliency() differentiates them,
        both restricted to the frame's own tokens (CLS + patches).  The relevance of the CLS token is row 0 of
        (I + A-_L) ... (I + A-_1), run as the vector chain r <- e_cls, r <- r + r A-_l from the last block to the first
        inside the HIP backward of the vision tower (gava_attention_relevance, one launch per block, on the d mix the backward
        forms anyway; neither the probabilities nor their gradients are ever in memory).
        The result is NOT normalised: its scale is the gradient's (patches >= 0, cls >= 1, no fixed sum); compare maps of one
        call, or normalise them yourself.  The prompt tokens are rebuilt in every block and carry no token identity between
        blocks - the restriction the rollout documents -, so relevance that flows through the local-prompt / summary path
        from frame to frame is NOT attributed; the gradient itself is the true one, prompt path included.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it (decoded uint8 videos: `preprocessor.batch(videos)`
        first).  T need not be num_frames; the B*T frames must be whole num_frames groups, as for attention_maps.  target: as
        for saliency - None (the top-1 class of this very forward, picked on the device), an int (checked on the host) or an
        int64 [B] device tensor (not range-checked).  The clips run in chunks of whole groups whose kept activations
        (training.kept_bytes) fit keep_activation_bytes - a chunk that still does not fit recomputes its blocks, in bf16 -;
        max_clips sets the clips per chunk instead.  Chunking does not change a bit of the result.
        Works in eval() and train() mode, whatever is trainable; no .grad is touched, no graph and no kept activation survives
        the call, nothing waits for the device.  A per-descriptor (use_descriptor) head is refused, and so is a shape with more
        keys per frame than gava_attention_relevance takes."""
        from . import training
        sh, Tm = self._shape, self.num_frames
        if not (torch.is_tensor(x) and x.dim() == 5 and x.is_floating_point() and x.shape[1] == 3 and x.shape[3] == x.shape[4] == sh["size"]):
            raise hip.GavaError(f"relevance_maps takes a floating-point clip batch [B, 3, T, {sh['size']}, {sh['size']}], got "
                                f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        if not x.is_cuda:
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError("relevance_maps: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class to differentiate")
        B, T = x.shape[0], x.shape[2]
        n_cls = self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]
        if target is not None and not torch.is_tensor(target):
            if not 0 <= int(target) < n_cls:
                raise hip.GavaError(f"relevance_maps: target {target} is outside the {n_cls} classes")
        elif target is not None and not (target.is_cuda and target.dtype == torch.int64 and tuple(target.shape) == (B,)):
            raise hip.GavaError(f"relevance_maps: a tensor target must be int64 [{B}] on the device")
        unit = Tm // math.gcd(T, Tm)                  # the fewest clips that are whole num_frames groups
        if B == 0 or B % unit:
            raise hip.GavaError(f"relevance_maps: {B} clips of {T} frames are not whole groups of num_frames = {Tm}")
        g = sh["size"] // sh["P"]
        n1 = g * g + 1
        n_all = n1 + sh["G"] + Tm + 1
        if n_all > hip.ATTENTION_RELEVANCE_MAX_KEYS:
            raise hip.GavaError(f"relevance_maps: {n_all} keys per frame, gava_attention_relevance takes at most {hip.ATTENTION_RELEVANCE_MAX_KEYS}")
        if max_clips is None:
            step = B // unit * unit
            while step > unit and training.kept_bytes(self, step, T) > self.keep_activation_bytes:
                step = (step // unit + 1) // 2 * unit
        else:
            step = min(B, max(int(max_clips) // unit * unit, unit))
        rs, logits, targets = [], [], []
        for i in range(0, B, step):
            tg = target[i:i + step] if torch.is_tensor(target) else target
            r, lg, tg = self._relevance_chunk(x[i:i + step], tg, {})
            rs.append(r), logits.append(lg), targets.append(tg)
        m = (rs[0] if len(rs) == 1 else torch.cat(rs, 0)).view(B, T, n1)
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, 0)
        return RelevanceMaps(m[..., 1:].reshape(B, T, g, g), m[..., 0], cat(logits), target if torch.is_tensor(target) else cat(targets))

    def _relevance_chunk(self, x, target, state):
        """One chunk of relevance_maps: the grad-enabled forward of whole groups and the vision tower's backward with the
        relevance request.  state: the request's state ({}; tests pass dict(capture=[]), see training._relevance_step).
        -> (r fp32 [B*T, n1], logits [B, C], target int64 [B])."""
        with torch.cuda.device(x.device), torch.enable_grad():
            xg = x.detach().float().contiguous().requires_grad_()       # a leaf of this call's own: it makes the tower differentiable
            request = dict(relevance=state)
            logits = self._forward_impl(xg, None, None, False, input_request=request)[0]
            if target is None:
                target = logits.detach().argmax(dim=1)
            elif not torch.is_tensor(target):
                target = torch.full((x.shape[0],), int(target), dtype=torch.int64, device=x.device)
            score = logits.gather(1, target.view(-1, 1)).sum()
            torch.autograd.grad(score, [xg], allow_unused=True)          # runs the vision tower's backward, nothing else
        if torch.is_tensor(self.text_features) and self.text_features.requires_grad:
            self.text_features = self.text_features.detach()        # the last reference into this call's graph
        state.pop("r", None)
        return request.pop("out"), logits.detach(), target

    def perturbation_curves(self, x, scores, mode="deletion", target=None, steps=10, fractions=None, scope="clip",
                            baseline="zero", blur_sigma=5.0, max_clips=None):
        """How faithful an importance map is to the model: the deletion or insertion curve of every clip (Petsiuk et al.,
        "RISE"; the test Chefer et al. report for relevance) -> PerturbationCurves (see there for the fields).
          mode="deletion"   the most important units are replaced by the baseline first: the target's score should FALL fast
          mode="insertion"  start from the baseline and put the most important units back first: it should RISE fast
        x: fp32 device clips [B, 3, T, S, S], as for saliency.  scores: what to rank by, fp32 on x's device -
        [B, T, g, g] (patches, g = S / P: attention_maps(x).patches, relevance_maps(x).patches), [B, T, S, S] (pixels, summed
        over each patch: saliency(x)[0]) or [B, T] (frames: the maps' .cls, or any per-frame score).  scope="clip" ranks all
        units of a clip together, scope="frame" the patches of every frame among themselves (every frame then loses the same
        number of patches per step; refused for frame scores).  The order is exact: descending, ties to the lower index,
        NaNs last (gava_patch_ranks).
        fractions: the share of a ranking's n units perturbed at each step - by default linspace(0, 1, steps + 1), else a
        strictly increasing list from 0 to 1; step s perturbs the k_s = floor(f_s n + 0.5) first units of the ranking.
        baseline: "zero" (the dataset's mean colour, in the normalised space clips live in), "blur" (the clip itself under a
        Gaussian of blur_sigma pixels, radius ceil(3 sigma), border replicated), an fp32 tensor [3] (one value per channel) or
        one shaped like x.  target: as for saliency - None (each clip's top-1 class on its UNPERTURBED step, picked on the
        device), an int (checked on the host) or an int64 [B] device tensor (out of range: that clip's curves are NaN).
        Evaluation only: call it under torch.no_grad() on a model in eval() mode.  The S1 = len(fractions) perturbed copies
        of a clip are written by one kernel (gava_perturb_clips) and go through the plain forward, max(1, max_clips // S1)
        whole clips at a time; max_clips defaults to the most clips one launch's grid covers (65535 frames).  A chunk's
        nb * S1 perturbed clips are in memory at once (4.8 MB each at 224 px and T = 8) next to the forward's workspace: lower
        max_clips for big batches.  Chunking changes no bit.  The text features are cached for the duration of the call (cache_text_features is restored afterwards).  The
        call ends with one gava_perturb_scores launch over all clips and never waits for the device.
        Several ranks: every rank passes its own clips and gets the curves of its own clips (the forward gathers the
        perturbed clips' features of all ranks, local_logits() takes this rank's rows back out); every rank must therefore
        pass the same B, the same number of fractions and the same max_clips."""
        what = "perturbation_curves"
        if torch.is_grad_enabled() or self.training:
            raise hip.GavaError(f"{what} is an evaluation path: call it under torch.no_grad() on a model in eval() mode")
        if mode not in ("deletion", "insertion"):
            raise hip.GavaError(f"{what}: mode must be 'deletion' or 'insertion', got {mode!r}")
        if scope not in ("clip", "frame"):
            raise hip.GavaError(f"{what}: scope must be 'clip' or 'frame', got {scope!r}")
        sh = self._shape
        S, P = sh["size"], sh["P"]
        if not (torch.is_tensor(x) and x.dim() == 5 and x.is_floating_point() and x.shape[1] == 3 and x.shape[3] == x.shape[4] == S
                and x.shape[0] > 0 and x.shape[2] > 0):
            raise hip.GavaError(f"{what} takes a floating-point clip batch [B, 3, T, {S}, {S}], got "
                                f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        B, T, g = x.shape[0], x.shape[2], S // P
        layouts = {(B, T, g, g): "patch", (B, T, S, S): "pixel", (B, T): "frame"}
        if not (torch.is_tensor(scores) and scores.is_floating_point() and tuple(scores.shape) in layouts):
            raise hip.GavaError(f"{what}: scores must be a floating-point [{B}, {T}, {g}, {g}] (patches), [{B}, {T}, {S}, {S}] (pixels) or "
                                f"[{B}, {T}] (frames) tensor, got {(scores.dtype, tuple(scores.shape)) if torch.is_tensor(scores) else type(scores)}")
        layout = layouts[tuple(scores.shape)]
        if layout == "frame" and scope == "frame":
            raise hip.GavaError(f"{what}: scope='frame' ranks the patches of a frame; frame scores have one unit per frame")
        n = T if layout == "frame" else T * g * g if scope == "clip" else g * g
        if n > hip.PERTURB_MAX_UNITS:
            raise hip.GavaError(f"{what}: {n} units per ranking, at most {hip.PERTURB_MAX_UNITS} are supported")
        fr, ks = hip.perturb_thresholds(n, steps, fractions)
        S1 = len(fr)
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError(f"{what}: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class")
        n_cls = self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]
        if target is not None and not torch.is_tensor(target):
            if not 0 <= int(target) < n_cls:
                raise hip.GavaError(f"{what}: target {target} is outside the {n_cls} classes")
        elif target is not None and not (target.dtype == torch.int64 and tuple(target.shape) == (B,)):
            raise hip.GavaError(f"{what}: a tensor target must be int64 [{B}] on the device")
        kind = baseline if isinstance(baseline, str) else "tensor"
        if kind not in ("zero", "blur", "tensor") or (kind == "tensor" and not (
                torch.is_tensor(baseline) and baseline.is_floating_point() and (tuple(baseline.shape) == (3,) or baseline.shape == x.shape))):
            raise hip.GavaError(f"{what}: baseline must be 'zero', 'blur', a floating-point tensor [3] or one shaped like x, got "
                                f"{(baseline.dtype, tuple(baseline.shape)) if torch.is_tensor(baseline) else baseline!r}")
        taps = hip.gaussian_taps(blur_sigma) if kind == "blur" else None
        fit = hip.MAX_GRID_FRAMES // T
        if fit < S1:
            raise hip.GavaError(f"{what}: one clip's {S1} steps x {T} frames are past the {hip.MAX_GRID_FRAMES} frames one launch covers")
        step = max(1, (fit if max_clips is None else min(fit, int(max_clips))) // S1)
        if not x.is_cuda or not scores.is_cuda or (torch.is_tensor(target) and not target.is_cuda):
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        dev = x.device
        cached = self.cache_text_features
        self.cache_text_features = True
        try:
            with torch.cuda.device(dev):
                x = x.detach().float().contiguous()
                ranks = hip.patch_ranks(scores.detach().to(dev).float().contiguous(), patch=P if layout == "pixel" else None, scope=scope)
                if kind == "zero":
                    base = None
                elif kind == "blur":
                    base = hip.blur_clips(x, taps)
                else:
                    base = baseline.detach().to(dev).float().contiguous()
                if target is not None and not torch.is_tensor(target):
                    target = torch.full((B,), int(target), dtype=torch.int64, device=dev)
                logits = None
                for i in range(0, B, step):
                    nb = min(step, B - i)
                    b = base[i:i + nb] if base is not None and base.dim() == 5 else base
                    xp = hip.perturb_clips(x[i:i + nb], ranks[i:i + nb], ks, patch=P, mode=mode, baseline=b)
                    lg = self.local_logits(self._forward_impl(xp.view(nb * S1, 3, T, S, S), None, None, False)[0])
                    if nb == B:
                        logits = lg
                        break
                    if logits is None:
                        logits = torch.empty(B * S1, lg.shape[-1], dtype=torch.float32, device=dev)
                    logits[i * S1:(i + nb) * S1] = lg
                self.last["local_batch"] = B
                res = hip.perturb_scores(logits, fr, ref_step=0 if mode == "deletion" else S1 - 1,
                                         target=target.contiguous() if target is not None else None)
        finally:
            self.cache_text_features = cached
        return PerturbationCurves(mode, torch.tensor(fr, dtype=torch.float32), res["logit"], res["prob"], res["top1"],
                                  res["auc_logit"], res["auc_prob"], res["target"], ranks)

    _FAITHFULNESS_METHODS = ("rollout", "relevance", "saliency", "integrated", "smoothgrad")

    def faithfulness(self, x, methods=("rollout", "relevance", "saliency"), target=None, seed=0, **kw):
        """Which map to believe for this model and these clips: both perturbation curves of every method's map, for one and
        the same target, next to a random ranking -> Faithfulness, {name: {"deletion": ..., "insertion": ...}}; print its
        .table().  methods: any of "rollout" (attention_maps(x).patches), "relevance" (relevance_maps(x, target).patches) and
        "saliency" (saliency(x, target)[0], pixels pooled to patches), and on request "integrated"
        (integrated_gradients(x, target).maps, the signed sum: what speaks FOR the class goes first, as with relevance) and
        "smoothgrad" (smooth_grad(x, target)[0]), both with their defaults; the control "random" ranks by uniform scores drawn from
        a device generator seeded with `seed`, so a call repeats bit for bit.  target: as for perturbation_curves; None is the
        top-1 class of the plain forward of x, picked on the device once and used for every method.  **kw goes to
        perturbation_curves (steps, fractions, scope, baseline, blur_sigma, max_clips; not mode).  Evaluation only, like
        perturbation_curves; the maps' own rules apply to x (whole num_frames groups).  Nothing waits for the device."""
        if torch.is_grad_enabled() or self.training:
            raise hip.GavaError("faithfulness is an evaluation path: call it under torch.no_grad() on a model in eval() mode")
        methods = tuple(methods)
        if not methods or any(m not in self._FAITHFULNESS_METHODS for m in methods) or len(set(methods)) != len(methods):
            raise hip.GavaError(f"faithfulness: methods must be distinct names out of {self._FAITHFULNESS_METHODS}, got {methods!r}")
        if "mode" in kw:
            raise hip.GavaError("faithfulness runs both modes: mode is not an argument")
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 5):
            raise hip.GavaError("faithfulness takes a device clip batch [B, 3, T, S, S]: there is no CPU fallback")
        B, T = x.shape[0], x.shape[2]
        g = self._shape["size"] // self._shape["P"]
        with torch.cuda.device(x.device):
            if target is None:
                target = self.local_logits(self._forward_impl(x, None, None, False)[0]).argmax(dim=1)
            elif not torch.is_tensor(target):
                n_cls = self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]
                if not 0 <= int(target) < n_cls:
                    raise hip.GavaError(f"faithfulness: target {target} is outside the {n_cls} classes")
                target = torch.full((B,), int(target), dtype=torch.int64, device=x.device)
            maps = {}
            for m in methods:
                if m == "rollout":
                    maps[m] = self.attention_maps(x).patches
                elif m == "relevance":
                    maps[m] = self.relevance_maps(x, target).patches
                elif m == "integrated":
                    maps[m] = self.integrated_gradients(x, target).maps
                elif m == "smoothgrad":
                    maps[m] = self.smooth_grad(x, target)[0]
                else:
                    maps[m] = self.saliency(x, target)[0]
            gen = torch.Generator(device=x.device)
            gen.manual_seed(int(seed))
            maps["random"] = torch.rand(B, T, g, g, generator=gen, dtype=torch.float32, device=x.device)
            out = Faithfulness()
            for name, s in maps.items():
                out[name] = {md: self.perturbation_curves(x, s.detach().contiguous(), mode=md, target=target, **kw) for md in ("deletion", "insertion")}
        return out

    def _maps_logits(self, video):
        """The inference head (gava_similarity_head) on this rank's clip features; text features from the cache when it is
        valid, else from the text tower on the current stream.  Leaves text_features, the cache and `last` alone."""
        dev, sh = video.device, self._shape
        if self.use_text_prompt_learning:
            pl_params = list(self.prompt_learner.parameters())
            key = ((self._pack_key(), tuple(q._version for q in pl_params), tuple(q.data_ptr() for q in pl_params))
                   if (self.cache_text_features and not self.training) else None)
            hit = key is not None and self._text_cache is not None and self._text_cache[0] == key
            text = self._text_cache[1] if hit else self.encode_text()
            n_kv = self.prompt_learner.n_kv
        else:
            text, n_kv = self.text_features.detach().to(device=dev, dtype=torch.float32).contiguous(), 1
        Bg, n_cls = video.shape[0], text.shape[0] // n_kv
        logits = torch.empty(Bg, n_cls, dtype=torch.float32, device=dev)
        tfeat = torch.empty(n_cls, sh["E"], dtype=torch.float32, device=dev)
        vnorm = torch.empty(Bg, sh["E"], dtype=torch.float32, device=dev)
        ls = self.logit_scale.detach().float().reshape(1)
        lb = self.logit_bias.detach().float().reshape(1) if self.logit_bias is not None else None
        hip.check(hip.load().gava_similarity_head(hip.ptr(video), hip.ptr(text), hip.ptr(ls), hip.ptr(lb), Bg, n_cls, n_kv,
                                                  sh["E"], hip.ptr(logits), hip.ptr(tfeat), hip.ptr(vnorm), hip.stream_ptr(dev)),
                  "gava_similarity_head")
        return logits

    def _forward_impl(self, x, memory, video_nte, desc_wise, clips=None, input_request=None):
        lib = hip.load()
        if clips is not None:
            B, T = clips[1], clips[2]
        else:
            B, Cc, T, Hh, Ww = x.size()
        self.last["local_batch"] = B
        sh = self._shape
        if not x.is_cuda:
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")
        want_dx = clips is None and torch.is_grad_enabled() and x.requires_grad
        if want_dx and x.dtype != torch.float32:
            raise hip.GavaError(f"the gradient with respect to the input clip is computed for fp32 clips only, x is {x.dtype}: "
                                "pass x.float(), or detach x")
        text, text_stream = None, None
        self._attach_encoders()
        self._pack()   # (re)pack weights on the caller's stream, before any fork
        if self.use_text_prompt_learning:
            if desc_wise:
                assert self.training == False
            # the cached text features depend on the packed weights AND on the (pass-through) context vectors
            pl_params = list(self.prompt_learner.parameters())
            key = ((self._pack_key(), tuple(q._version for q in pl_params), tuple(q.data_ptr() for q in pl_params))
                   if (self.cache_text_features and not self.training) else None)
            train_text = torch.is_grad_enabled() and any(q.requires_grad for q in pl_params)
            if train_text:
                # differentiable text tower (gava_clip_amd/training.py): HIP kernels in both directions; the
                # knowledge-aware context MLP (if any) is torch glue in front of it
                from .training import TextTowerFn
                ctx_full = self.prompt_learner.full_context()
                if self.text_on_side_stream:
                    # own stream, like the inference path; autograd runs TextTowerFn.backward on this stream too
                    # (and inserts the cross-stream waits), so the text tower overlaps the vision tower both ways
                    main = torch.cuda.current_stream(x.device)
                    if self._text_stream is None or self._text_stream.device != x.device:
                        self._text_stream = self._overlapping_stream(x.device)
                    text_stream = self._text_stream
                    text_stream.wait_stream(main)
                    with torch.cuda.stream(text_stream):
                        text = TextTowerFn.apply(self, ctx_full)
                else:
                    text = TextTowerFn.apply(self, ctx_full)
            elif key is not None and self._text_cache is not None and self._text_cache[0] == key:
                text = self._text_cache[1]
            else:
                # The text tower does not depend on the clip: it runs on its own HIP stream beside the
                # vision tower (its few-workgroup kernels slot in between the big GEMMs) and joins at the head.
                main = torch.cuda.current_stream(x.device)
                if self.text_on_side_stream:
                    if self._text_stream is None or self._text_stream.device != x.device:
                        self._text_stream = self._overlapping_stream(x.device)
                    text_stream = self._text_stream
                    text_stream.wait_stream(main)
                    with torch.cuda.stream(text_stream):
                        text = self.encode_text()
                else:
                    text = self.encode_text()
                self._text_cache = (key, text) if key is not None else None
        else:
            text = self.text_features.to(device=x.device, dtype=torch.float32).contiguous()
        train_vision = want_dx or (torch.is_grad_enabled() and any(p.requires_grad for _, p in self._vision_trainables()))
        if train_vision:
            # differentiable vision tower (gava_clip_amd/training.py): gradients of the prompt parameters and, for an fp32 x
            # that requires grad (in train() or eval() mode, whatever is frozen), of the clip itself
            from .training import VisionTowerFn
            cls_x, summary = VisionTowerFn.apply(self, x, clips, input_request, *[p for _, p in self._vision_trainables()])
        else:
            cls_x, summary = self.encode_video(x, clips=clips)
        # The all-gather of the clip embeddings goes out on the main stream as soon as the vision tower is enqueued - BEFORE the
        # join with the text stream, so that it overlaps what is left of the text tower (it does not depend on it).
        # Under autograd every rank keeps its own clips (the reference's DDP computes the loss on local logits).
        video = cls_x if cls_x.requires_grad else self._gather(cls_x)
        if text_stream is not None:
            torch.cuda.current_stream(x.device).wait_stream(text_stream)
            text.record_stream(torch.cuda.current_stream(x.device))
        if torch.is_grad_enabled() and (text.requires_grad or video.requires_grad or self.logit_scale.requires_grad):
            # training: the 2*B*C*E-flop head is traced by torch so that d logits reaches both towers' HIP backward
            if self.train_head == "hip":
                logits = self._train_head_hip(video, text, summary, desc_wise)
            elif self.train_head == "torch":
                logits = self._train_head(video, text, summary, desc_wise)
            else:
                raise hip.GavaError(f"train_head must be 'torch' or 'hip', got {self.train_head!r}")
        else:
            Bg, Cn = video.shape[0], text.shape[0]
            n_kv = self.prompt_learner.n_kv if self.use_text_prompt_learning else 1
            ragged = n_kv is None        # use_descriptor: the head runs per prompt, the (tiny) class means follow in torch
            if (desc_wise and self.use_text_prompt_learning) or ragged:
                n_cls, n_kv = Cn, 1      # per-description logits (VitaCLIP_model.py:265-276): every prompt is its own "class"
            else:
                n_cls = Cn // n_kv
            empty = Bg == 0          # no clips (upstream returns (0, C) logits and still refreshes text_features): one dummy row
            if empty:
                video, Bg = torch.zeros(1, sh["E"], dtype=torch.float32, device=x.device), 1
            logits = torch.empty(Bg, n_cls, dtype=torch.float32, device=x.device)
            tfeat = torch.empty(n_cls, sh["E"], dtype=torch.float32, device=x.device)
            vnorm = torch.empty(Bg, sh["E"], dtype=torch.float32, device=x.device)
            ls = self.logit_scale.detach().float().reshape(1)
            lb = self.logit_bias.detach().float().reshape(1) if self.logit_bias is not None else None
            hip.check(lib.gava_similarity_head(hip.ptr(video), hip.ptr(text), hip.ptr(ls), hip.ptr(lb), Bg, n_cls, n_kv,
                                               sh["E"], hip.ptr(logits), hip.ptr(tfeat), hip.ptr(vnorm), hip.stream_ptr(x.device)),
                      "gava_similarity_head")
            if empty:
                logits, vnorm = logits[:0], vnorm[:0]
            self.last.update(video_features=vnorm, summary=summary)
            if desc_wise and self.use_text_prompt_learning:
                self.text_features = tfeat            # upstream leaves the last class's features here; not relied upon
                logits = list(torch.split(logits, self.prompt_learner.kv_counts, dim=1))     # list of (B, n_kv_c)
            elif ragged:
                A = self._class_mean_matrix(x.device)                                        # VitaCLIP_model.py:288-291
                logits = logits @ A      # (a logit_bias, added per prompt by the head, survives the mean unchanged)
                tf = A.t() @ tfeat
                self.text_features = tf / tf.norm(dim=-1, keepdim=True)
            elif self.use_text_prompt_learning:
                self.text_features = tfeat            # VitaCLIP_model.py:293

        # auxiliary heads: inactive at every accelerated configuration; by default PyTorch glue on the device so that
        # callers passing video_nte / memory still get the reference's outputs - and, in training, its gradients
        # (`summary` and `text_features` carry the towers' autograd nodes); aux_heads = "hip" runs them as HIP kernels.
        hip_aux = self.aux_heads == "hip"   # NteHeadFn / MemoryHeadFn: the same outputs and gradients from the kernels of aux_heads.hip
        if hip_aux and self.add_nte and video_nte is not None:
            from .training import NteHeadFn
            logits_vm = NteHeadFn.apply(summary, self.sum_proj.weight, self.sum_proj.bias, video_nte, self.logit_scale_vm)
        elif self.add_nte and video_nte is not None:            # VitaCLIP_model.py:311-345
            sp = self.sum_proj(summary)
            sp = sp / sp.norm(dim=-1, keepdim=True)
            with torch.no_grad():
                valid_idx = ((video_nte.sum(dim=-1).sum(dim=-1)) != 0).float()
                valid_mat = valid_idx.unsqueeze(1) * valid_idx.unsqueeze(0)
            video_nte = video_nte / video_nte.norm(dim=-1, keepdim=True)
            similarity = torch.bmm(sp.unsqueeze(0).expand(NUM_COMB, -1, -1), video_nte.permute(1, 2, 0)).mean(0)
            logits_mat = self.logit_scale_vm * (similarity * valid_mat)
            logits_vm = F.log_softmax(logits_mat, dim=-1) + F.log_softmax(logits_mat, dim=-2)
        else:
            logits_vm = None
        if hip_aux and self.use_support_memory and memory is not None:
            logits_mt = self._memory_head_hip(memory, self.text_features.detach() if self.detach_features else self.text_features)
        elif self.use_support_memory and memory is not None:    # VitaCLIP_model.py:347-398
            text_features = self.text_features.detach() if self.detach_features else self.text_features
            memory = memory.mean(dim=1)
            logits_mt = torch.empty(memory.size(0), 0).to(memory.device)
            for cid, mproj in enumerate(self.memory_project):
                tf = self.tf_project(text_features[cid])
                tf = tf / tf.norm(dim=-1, keepdim=True)
                memo = mproj(memory)
                memo = memo / memo.norm(dim=-1, keepdim=True)
                logits_mt = torch.concat([logits_mt, (self.logit_scale_mt * memo @ tf.t()).unsqueeze(-1)], dim=1)
            logits_mt = F.log_softmax(logits_mt, dim=-1)
            if self.logit_bias_mt is not None:
                logits_mt += self.logit_bias_mt
        else:
            logits_mt = None
        return logits, logits_mt, logits_vm
