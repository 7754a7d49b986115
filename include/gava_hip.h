/* gava_hip.h — C ABI of libgava_hip.so: the MI355X (gfx950) implementation of the GaVA-CLIP
 * video-frame forward path.
 *
 * The reference (lisqzqng/GaVA-CLIP) is pure PyTorch and has no FFI or operator registry; its
 * boundary for this path is the Python class VitaCLIP(nn.Module)
 * (training/VitaCLIP_model.py:22-401).  Each entry point below replaces the stock PyTorch ops
 * of one stretch of that forward; the citation says which.  The host-side mirror
 * (gava_clip_amd/model.py) binds them with ctypes, see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; nothing is allocated, freed or
 *     synchronised inside a call; all work is enqueued on `stream` (a hipStream_t).
 *   - return value: 0 on success, negative GAVA_E* on a rejected call (nothing launched).
 *   - "h16" = 16-bit MFMA operand storage, fp16 or bf16 as selected by `prec`
 *     (GAVA_PREC_*).  Accumulators, LayerNorm, softmax, residual stream and the
 *     similarity head are always fp32.
 *   - weights are [out_features][in_features] row-major (nn.Linear layout).
 */
#ifndef GAVA_HIP_H
#define GAVA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAVA_OK 0
#define GAVA_EINVAL (-1)   /* shape/alignment the kernels do not support */
#define GAVA_EWORKSPACE (-2) /* workspace too small */
#define GAVA_ELAUNCH (-3)  /* hipGetLastError() != hipSuccess after a launch */

#define GAVA_PREC_F16 0
#define GAVA_PREC_BF16 1

/* GEMM epilogues */
#define GAVA_EPI_H16 0        /* out16 = (acc + bias) * (col < scale_cols ? scale : 1)        */
#define GAVA_EPI_H16_QGELU 1  /* out16 = quickgelu(acc + bias), x*sigmoid(1.702x)              */
#define GAVA_EPI_F32 2        /* out32 = acc + bias (+ resid32, may alias out32)               */
#define GAVA_EPI_F32_PATCH 3  /* patch-embed: row remap + pos/time embedding (see below)       */
#define GAVA_EPI_H16_QGELU_BWD 4 /* backward: out16 = acc * quickgelu'(aux16), aux = pre-activation [M][ldo] */

typedef void* gava_stream_t;

int gava_abi_version(void);
/* Debug hook: device buffer (u64[8] per wave) that instrumented kernels fill with per-segment cycle
 * sums; NULL (default) disables every stamp.  Not used by the product path. */
int gava_debug_set_buffer(void* dev_u64);
/* Measurement hook (bench.py `roofline`): while enabled, gava_vision_forward brackets ONE kernel of every full-width block
 * with a pair of HIP events on the stream it launches on: on = GAVA_PROBE_FC1 (the fc1 GEMM), _OUT (out_proj), _FC2,
 * _QKV (the LayerNorm-folded qkv GEMM: blocks 1 .. layers-2) or _ATTN; 0 = off.  gava_probe_fc1_read waits for the last
 * pair and returns the number of block slots, writing up to `cap` elapsed times in ms (-1 in the slots of blocks the probed
 * kernel did not run in: _QKV leaves slot 0 unused).  Off by default; never enabled by the model code. */
#define GAVA_PROBE_FC1 1
#define GAVA_PROBE_OUT 2
#define GAVA_PROBE_FC2 3
#define GAVA_PROBE_QKV 4
#define GAVA_PROBE_ATTN 5
int gava_probe_fc1_enable(int on);
int gava_probe_fc1_read(float* ms, int cap);

/* C[M,N] = A[M,K] · W[N,K]^T with a fused epilogue.  Replaces nn.Linear / the conv-as-GEMM of
 * ImagePatchEmbed2D (VitaCLIP_vision_encoder_utils.py:66,79,110-115,215-219;
 * VitaCLIP_text_encoder.py:73-77 and the projections inside nn.MultiheadAttention :71).
 * Requirements: N % 128 == 0, K % 64 == 0, lda/ldw multiples of 8 elements, 16-byte aligned
 * pointers.  M is arbitrary. */
/* One decoded video for the fused input path: the patch-embedding GEMM builds its A tiles straight from
 * the uint8 RGB frames [n_frames][height][width][3] - temporal crop, (u8/255 - mean)/std, bilinear short-side resize and
 * centre crop of video_dataset/dataset.py:117-139 are evaluated per loaded pixel, with the arithmetic of
 * gava_preprocess_clip (bit-identical values), and the fp32 clip is never written to HBM.  gava_clip_geometry() fills the
 * derived fields from the video's size.  Device array, one entry per clip of the batch. */
typedef struct {
  const uint8_t* frames; int n_frames, height, width;
  int t_st, rate;                   /* frame(t) = min(t_st + t*rate, n_frames-1)                    */
  int h_st, w_st;                   /* crop offset inside the resized frame                          */
  float scale_h, scale_w;           /* source / resized extent (align_corners = False)               */
  /* Source box inside the decoded frame: the bilinear taps read rows box_y + [0, box_h) and columns box_x + [0, box_w) only,
   * and the neighbour of the box's last row / column is that row / column itself (the reference interpolates the cropped
   * tensor, transform.py:570-577); the row pitch stays `width`.  Evaluation branch: the whole frame. */
  int box_y, box_x, box_h, box_w;
  /* Which of torch's two CPU bilinear kernels the pixels follow.  0: the separable one (lerp along x, then along y) that
   * F.interpolate runs when output height + width > 128 - every evaluation-branch descriptor, as before the box existed.
   * T > 0 (the clip's frame count): the four-weight one it runs for smaller outputs, where the frames are the vectorised
   * dimension: out = w00*p00 + w01*p01 + w10*p10 + w11*p11 with w = products of the two lerp weights, accumulated by fma
   * from w10*p10 in the order p11, p01, p00 for the frames in whole groups of 8, from w01*p01 in the order p00, p10, p11 for
   * the T % 8 frames left over.  gava_clip_geometry_box sets it when 2*size <= 128.  The rule was derived from the CPU build
   * of torch 2.10 on x86 (the same with its AVX2 and AVX512 code paths, any thread count; its scalar no-fma path differs
   * from both kernels' forms): if tests/test_train_preprocess.py's small-size cases stop matching after a torch upgrade while
   * the CPU restatement still reproduces the fixtures, this rule is what changed.  The evaluation branch deliberately does
   * NOT follow it: gava_clip_geometry always sets 0, also where the resized frame is that small, to keep its bits. */
  int lerp4_frames;
  /* Frame table: device int[T] with the source frame of every output frame, or NULL = the arithmetic form above.  TSN
   * sampling (sampling_rate < 0, dataset.py:205-209) has no arithmetic form. */
  const int* frame_idx;
} gava_clip_desc;
/* host helper: the integer / float geometry of dataset.py:124-129,163-186 for one video (evaluation branch: whole-frame box,
 * no frame table); 0 on success */
int gava_clip_geometry(gava_clip_desc* d, int T, int rate, int size, int first_temporal_view, int first_spatial_view);
/* host helper: the geometry of ONE of the n_spatial x n_temporal evaluation crops of a video (dataset.py:135-136 builds them
 * all), view = sv * n_temporal + tv in the order of upstream's list (spatial-major).  d->frames / n_frames / height / width are
 * set by the caller, as for gava_clip_geometry.
 *   temporal (:160-175)  slide_len = max(n_frames - ((T-1)*rate + 1), 0); t_st = slide_len / 2 when n_temporal == 1, else
 *                        Python's round(slide_len / (n_temporal-1) * tv): the double quotient first, then the product, rounded
 *                        half to even.  frame(t) = min(t_st + t*rate, n_frames-1) supplies upstream's last-frame padding.
 *   spatial (:178-199)   n_spatial == 1: the centred crop; n_spatial == 3: offsets (0, margin/2, margin) along the longer
 *                        resized side, margin = max(new_h, new_w) - size, 0 along the other (a square frame: three equal views).
 * GAVA_EINVAL for any other n_spatial, n_temporal < 1 or view outside [0, n_spatial*n_temporal).  View 0 is, byte for byte, what
 * gava_clip_geometry writes with first_temporal_view = n_temporal > 1 and first_spatial_view = n_spatial == 3. */
int gava_clip_geometry_view(gava_clip_desc* d, int T, int rate, int size, int n_spatial, int n_temporal, int view);
/* host helper for the random-sample branch (dataset.py:93-114 with auto_augment=None): frames idx[0..T) of the video, the box
 * rows i + [0, h), columns j + [0, w) of each (transform.py:545-577 random_resized_crop) resized to size x size, i.e.
 * h_st = w_st = 0, scale_h = (float)h / size, scale_w = (float)w / size.  d->frames / n_frames / height / width are set by
 * the caller.  idx_host: the T indices for checking; idx_dev: the same T ints in device memory, stored as d->frame_idx.
 * GAVA_EINVAL for an empty box, a box that leaves the frame, or an index outside [0, n_frames): descriptors that pass go to
 * the device as they are, and the kernels still clamp box and index into the video (wrong pixels at worst, never a wild read). */
int gava_clip_geometry_box(gava_clip_desc* d, int size, int T, const int* idx_host, const int* idx_dev, int i, int j, int h, int w);

typedef struct {
  const void* A; int64_t lda;       /* h16 [M][lda]                                    */
  const void* W; int64_t ldw;       /* h16 [N][ldw]                                    */
  const float* bias;                /* [N] or NULL                                     */
  void* out; int64_t ldo;           /* h16 or fp32 [rows][ldo]                         */
  const float* resid; int64_t ldr;  /* EPI_F32: optional fp32 residual, may alias out  */
  int M, N, K;
  int epilogue;                     /* GAVA_EPI_*                                      */
  int prec;                         /* GAVA_PREC_*                                     */
  int scale_cols; float scale;      /* EPI_H16: columns [0,scale_cols) are multiplied  */
  /* EPI_F32_PATCH: GEMM row m = frame*n_patches + p is written to output row
   * frame*(n_patches+1) + 1 + p with + pos[(1+p)][:] + time[(frame % T)][:]
   * (VitaCLIP_vision_encoder.py:108-111,86-100). */
  const float* pos; const float* time; int n_patches; int T;
  /* EPI_F32_PATCH with A == NULL: im2col-free patch embedding.  The A tile is built on the fly from the
   * frames `frames` = fp32 (B,3,T,size,size): row m = frame*n_patches + p, column k = (c,ky,kx) reads
   * frames[b][c][t][py*P+ky][px*P+kx] (frame = b*T+t); loaded coalesced, converted to h16 and written to
   * the swizzled LDS tile, never materialised in HBM.  K = 3*P*P rounded up to 64 (W zero-padded). */
  const float* frames; int frame_size; int patch;
  /* EPI_H16 / EPI_H16_QGELU: split-precision output.  Row layout becomes [hi(N) | lo(N) | hi(N)]
   * (ldo >= 3N) with lo = h16(v - hi): the A operand of a following GEMM whose weight is packed
   * [W_hi | W_hi | W_lo] (K' = 3K), i.e. A_hi W_hi + A_lo W_hi + A_hi W_lo in one pass. */
  int split_out;
  const void* aux;                  /* EPI_H16_QGELU_BWD: h16 pre-activations, rows as out (ld = ldo) */
  int aux_prec;                     /* ... stored as GAVA_PREC_F16 / _BF16 (may differ from `prec`: activations kept
                                     * from an fp16 forward, gradients in bf16) */
  void* aux_out;                    /* EPI_H16_QGELU (training forward): also store the pre-activation acc + bias as
                                     * h16 [M][ldo] here; NULL = off */
  /* LayerNorm folded into the NEXT GEMM ("LayerNorm folding").  Producer side, EPI_F32: besides out32 also
   * store x16 = h16(out) [M][ld_x16] and, per row and 64-column group, the partial sums (sum x, sum x^2) as
   * float2 rowsum[M][N/64].  gava_row_stats turns them into (mean, rstd).  Consumer side, EPI_H16 / EPI_H16_QGELU with
   * A = x16 and W = h16(gamma * W): out = rstd_m * (acc - mean_m * fold_s[n]) + fold_t[n], fold_s[n] = sum_k W[n][k],
   * fold_t[n] = sum_k beta[k] * W0[n][k] + bias[n] (bias must then be NULL). */
  void* x16_out; int64_t ld_x16; float* rowsum_out;
  const float* fold_stats; const float* fold_s; const float* fold_t;
  /* persistent (one workgroup per CU) kernels only: leave this many CUs out of the grid, so that small kernels the
   * caller runs on another stream beside this GEMM get CUs of their own (0 = use every CU).  Per call: the library keeps
   * no launch state between calls. */
  int cu_reserve;
  /* LayerNorm folding without the gava_row_stats launch in between (big-M GEMMs: the persistent kernel only; N % 256 == 0,
   * N <= 1024; anything else is rejected, never silently routed to another path).  Producer: rowsum_reduced != 0 makes
   * rowsum_out float2 [ceil(M/256)*256][4] - slot n/256 of row m holds (sum x, sum x^2) over columns [256*(n/256), +256),
   * partial sums added in a fixed order.  Consumer: fold_partials = that array (instead of fold_stats); the
   * kernel derives (mean, rstd) of its rows itself (eps 1e-5, variance = E[x^2] - mean^2, fixed summation order). */
  int rowsum_reduced;
  const float* fold_partials;
  /* EPI_F32_PATCH with A == NULL and frames == NULL: the uint8 source (see gava_clip_desc): clips = device array
   * [M / (n_patches * T)], frame_size = the crop size, clip_lut = device fp32 [3][256]: lut[c][v] = (v/255 - mean[c]) / std[c]
   * as the caller's fp32 arithmetic gives it (the reference's own torch expression: the normalisation is then exact). */
  const gava_clip_desc* clips; const float* clip_lut;
  /* Kernel selection.  0 = automatic (by shape and epilogue, the only value the forward drivers pass).  Tests and A/B
   * timing may name a kernel: GAVA_KERNEL_256 = the persistent 256 x 256 kernel (one 512-thread workgroup per CU),
   * GAVA_KERNEL_PAIR = the persistent 128 x 256 kernel run as two 256-thread workgroups per CU (EPI_F32 only: the
   * residual-stream GEMMs out_proj / fc2 and their folding-producer form; N % 256 == 0, N <= 1024, K % 128 == 0).  A named
   * kernel that does not take the shape is rejected (GAVA_EINVAL), never replaced. */
  int kernel;
  /* Weight-lo pass (DESIGN.md "Numerics", round 4).  With 16-bit operands the rounding of the frozen WEIGHTS, not of the
   * activations, sets the logits error (tools/error_budget.py), so the product can be completed by A . W_lo^T with
   * W_lo = W - h16(W) while A stays a single 16-bit operand:
   *   w_lo = 1: W rows are [W_hi (K) | W_lo (K)] h16, ldw >= 2K; the k-loop runs 2K deep and re-reads A for the second half
   *             (nothing is stored twice).  K stays the number of columns of A.  Every kernel but GAVA_KERNEL_PAIR.
   *   w_lo = 2: the lo product at 8 bits on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4: twice the 16-bit
   *             rate): after the K-deep 16-bit loop, K more columns with A8 = bf8 (e5m2) copy of A, bytes [M][lda8], and
   *             W8 = e4m3 rows [N][ldw8] holding 2^w8_exp * W_lo (the MFMA's E8M0 scale operand takes the 2^-w8_exp back, so
   *             both products share the accumulators).  W stays [N][K] = W_hi.  K % 128 == 0; the 8-bit rows keep the BYTE
   *             pitch of their 16-bit twins, lda8 == 2 lda and ldw8 == 2 ldw (the kernel then addresses both phases with one
   *             set of offsets; half of each 8-bit row's pitch is unused); the persistent 256 x 256 kernel only (rejected
   *             elsewhere, never replaced).
   * Producers of a w_lo = 2 operand: out8 (EPI_H16 / EPI_H16_QGELU) = bf8 copy of the 16-bit output rows, bytes [M][ldo8];
   * x8_out (EPI_F32 with x16_out) = bf8 copy of x16_out, bytes [M][ld_x8].  bf8 = the fp16 value rounded to 2 mantissa
   * bits (fp16 operands only). */
  int w_lo;
  const void* A8; int64_t lda8; const void* W8; int64_t ldw8; int w8_exp;
  void* out8; int64_t ldo8; void* x8_out; int64_t ld_x8;
  /* The residual stream as a 16-bit pair (round 4; inference driver of the vision tower, DESIGN.md "Residual stream").  EPI_F32
   * with resid16 != NULL: the residual is read as resid16 + resid_lo (both [M][ldr]: hi in the operand type, lo in fp16 whatever
   * the operand type) and the result x = resid + A W^T + bias leaves as x16_out = h16(x) and xlo_out = fp16(x - h16(x)) (both
   * [M][ld_x16]) together with the producer's row sums (rowsum_out, computed from the fp32 x): 8 bytes per element through the
   * epilogue instead of 10 (fp32 in, fp32 out, 16-bit copy), and the hi half IS the operand of the GEMM that consumes the
   * LayerNorm fold.  |x - hi - lo| <= 2^-22 |x| (fp16 operands; 2^-19 with bf16).  out and resid must be NULL, x16_out /
   * xlo_out may alias resid16 / resid_lo (every element is read and written by the same lane).  The persistent 256 x 256
   * kernel with the ping-pong loop only (N % 256 == 0, K % 128 == 0, K >= 256, w_lo <= 1); rejected elsewhere. */
  const void* resid16; const void* resid_lo; void* xlo_out;
} gava_gemm_args;
#define GAVA_KERNEL_AUTO 0
#define GAVA_KERNEL_256 3
#define GAVA_KERNEL_PAIR 4
#define GAVA_KERNEL_PP 5    /* round 4: the persistent 256 x 256 kernel with the "ping-pong" k-loop (four 16-MFMA phases per k-tile,
                               the two wave groups one barrier apart, half-tiles staged six ahead): EPI_H16 / EPI_H16_QGELU
                               with the LayerNorm fold, plain EPI_H16, EPI_F32 with a residual (and its producer extras);
                               N % 256 == 0, K % 128 == 0, K >= 256 */
int gava_gemm(const gava_gemm_args* a, gava_stream_t stream);
/* Measurement helper (bench.py names the kernel instantiation a GEMM runs as): 1 when an EPI_F32 GEMM of M x N on the
 * persistent 256 x 256 kernel of the CURRENT device takes the aligned tile walk (the <..., ALIGN = true> instantiation:
 * super-tile blocks dealt to the XCDs), 0 when it takes the plain walk.  The same decision gava_gemm makes. */
int gava_gemm_aligned_walk(int M, int N, int cu_reserve);

/* Row LayerNorm (eps 1e-5, affine) fp32 -> h16 and/or fp32; one wave per row.  Replaces
 * LayerNorm (VitaCLIP_vision_encoder_utils.py:22-28, VitaCLIP_text_encoder.py:19-25).
 * gamma == NULL means "no normalisation": the row is only converted (used to feed cls_proj,
 * utils:164-165).  in_row_index (optional, int32[rows]) gathers input rows. D % 4 == 0, D <= 1024. */
typedef struct {
  const float* in; int64_t in_stride; const int32_t* in_row_index;
  const float* gamma; const float* beta;
  void* out16; int64_t out16_stride;     /* may be NULL */
  float* out32; int64_t out32_stride;    /* may be NULL; may alias in */
  int rows, D, prec;
  int split_out;                         /* out16 row = [hi(D) | lo(D) | hi(D)], see gava_gemm_args */
  /* Optional second LayerNorm applied to the first one's fp32 result in the same pass (both NULL = off): out32 then
   * receives LN(in; gamma, beta) and out16 receives LN(LN(in; gamma, beta); gamma2, beta2).  ln_pre followed by norm1 of
   * block 0 (VitaCLIP_vision_encoder.py:113, VitaCLIP_vision_encoder_utils.py:190): one read of the embedding instead
   * of two row passes. */
  const float* gamma2; const float* beta2;
  /* Optional 16-bit pair of what out32 receives (see gava_gemm_args.resid16): out_hi = h16(y), out_lo = fp16(y - h16(y)),
   * rows out_hl_stride apart, y = the FIRST LayerNorm's result (or the converted row when gamma == NULL).  Both or neither;
   * out32 may then be NULL. */
  void* out_hi; void* out_lo; int64_t out_hl_stride;
} gava_layernorm_args;
int gava_layernorm(const gava_layernorm_args* a, gava_stream_t stream);

/* Fused softmax(QK^T)V for head dim 64, key rows resident in LDS or streamed (see below).
 * Replaces Attention.forward's einsum/softmax/einsum (VitaCLIP_vision_encoder_utils.py:71-77)
 * and the scaled-dot-product inside nn.MultiheadAttention (VitaCLIP_text_encoder.py:81-83).
 * Q must already carry the 1/sqrt(64) factor.  Problem (n, h): queries are rows
 * n*n_q .. n*n_q+n_q-1 of q; keys/values are n_kmain rows n*n_kmain.. of k/v followed by
 * "side" rows taken from side_k/side_v (vision prompt tokens, see gava_vision_forward):
 *   n_g rows [0,n_g)                            shared by every problem   (global prompts)
 *   T   rows n_g + (n / T)*T + [0,T)            shared by the T frames of a clip (local prompts)
 *   1   row  n_g + batch + n                    per problem               (summary token)
 * With n_side == 0 there are no side rows.  causal: key j is visible to query i iff j <= i.
 * Up to 320 keys the key set is resident in LDS (single-pass softmax); longer non-causal key sets (long clips,
 * 336/384 px inputs) take a key-streaming online-softmax kernel.  causal: at most 320 keys. */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;  /* h16, element strides */
  const void* side_k; const void* side_v; int64_t ld_side;
  void* out; int64_t ld_out;                                     /* h16 [batch*n_q][ld_out] */
  int batch, heads, n_q, n_kmain;
  int n_g, T, has_summary;                                       /* side-row structure      */
  int causal, prec;
  int split_out;   /* out row = [hi(heads*64) | lo | hi], see gava_gemm_args */
  /* optional query addressing (0 = defaults): queries of problem n are rows n*q_batch_rows + [0,n_q)
   * of q with row stride ld_q.  Defaults: q_batch_rows = n_q, ld_q = ld_qkv.  Lets the last vision
   * block run only its CLS queries (n_q = 1, q_batch_rows = tokens per frame). */
  int q_batch_rows; int64_t ld_q;
} gava_attention_args;
int gava_attention(const gava_attention_args* a, gava_stream_t stream);

/* Exact-fp32 softmax attention for SHORT sequences (the text tower in inference: 77 padded tokens, 15-20 after the rows behind
 * the EOT are trimmed): q, k, v fp32 rows [batch*L][ld] (head h = columns [64h, 64h+64)), scores = scale * q.k (+ causal
 * mask), softmax and P.V in fp32 on the vector ALU - no 16-bit rounding of Q, K, V or P anywhere.  out: h16 rows
 * [batch*L][ld_out]; split_out != 0 writes [hi | lo | hi] copies heads*64 columns apart (A operand of a split-precision
 * GEMM, see gava_gemm_args.split_out).  Replaces the scaled-dot-product core of nn.MultiheadAttention
 * (VitaCLIP_text_encoder.py:71,83) where 16-bit MFMA operands would set the error of the text features.  L <= 128. */
typedef struct {
  const float* q; const float* k; const float* v; int64_t ld;
  void* out; int64_t ld_out;
  int batch, heads, L, causal, prec, split_out;
  float scale;
} gava_attention_f32_args;
int gava_attention_f32(const gava_attention_f32_args* a, gava_stream_t stream);

/* ---- fused drivers ---------------------------------------------------------------------- */

typedef struct {                 /* one TransformerEncoderLayer, utils:93-203 */
  const void* w_qkv; const float* b_qkv;   /* [3D][D]: q_proj;k_proj;v_proj stacked          */
  const void* w_out; const float* b_out;   /* [D][D]                                         */
  const void* w_fc1; const float* b_fc1;   /* [F][D]                                         */
  const void* w_fc2; const float* b_fc2;   /* [D][F]                                         */
  const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
  const void* w_cls; const float* b_cls;   /* cls_proj [D][D]                                */
  const float* sln_g; const float* sln_b;  /* summary_ln                                     */
  const void* w_sqkv; const float* b_sqkv; /* summary_attn_layer q;k;v stacked [3D][D]       */
  const void* w_sout; const float* b_sout;
  const float* local_prompts;              /* [T][D] fp32                                    */
  const float* global_prompts;             /* [G][D] fp32 (row i of visual.global_prompts)   */
  /* Optional (all NULL = off): LayerNorm folded into the consumer GEMM, inference driver only (see gava_gemm_args).
   * w_*_fold = h16(gamma * W) [N][D]; *_fold_s[n] = sum_k w_fold[n][k] (of the ROUNDED weight);
   * *_fold_t[n] = sum_k beta[k] * W[n][k] + bias[n] in fp32.  qkv: norm1 of this block, fc1: norm2. */
  const void* w_qkv_fold; const float* qkv_fold_s; const float* qkv_fold_t;
  const void* w_fc1_fold; const float* fc1_fold_s; const float* fc1_fold_t;
  /* Optional (all NULL = off), read for the LAST block of the inference driver only: its B*T CLS rows - the only rows
   * of that block that reach the outputs (VitaCLIP_vision_encoder.py:126) - run q_proj, out_proj, fc1 and fc2 in split
   * precision (weights packed [W_hi | W_hi | W_lo], see gava_gemm_args.split_out): 1/197 of the block's rows, and their
   * rounding lands on the video feature directly.  w_q_split [D][3D], w_out_split [D][3D], w_fc1_split [F][3D],
   * w_fc2_split [D][3F]. */
  const void* w_q_split; const void* w_out_split; const void* w_fc1_split; const void* w_fc2_split;
} gava_vision_layer;

typedef struct {
  int B, T_in, T_model;          /* clips, frames per clip in x, num_frames of the model      */
  int size, P, D, H, layers, F, E, G;
  int prec;
  const void* w_patch; const float* b_patch;   /* [D][Kp] h16, Kp = 3*P*P rounded up to 64   */
  const float* cls_token; const float* pos_embed; const float* time_embed; /* time: [T_in][D] */
  const float* lnpre_g; const float* lnpre_b; const float* lnpost_g; const float* lnpost_b;
  const void* w_proj;                          /* visual.proj transposed, split-packed: [E][3D] =
                                                  [W_hi | W_hi | W_lo] h16 (see gava_gemm_args)  */
  const gava_vision_layer* layer;              /* host array [layers]                         */
  /* optional uint8 input (gava_gemm_args.clips): when clips != NULL the drivers' `x` argument is ignored (may be NULL) */
  const gava_clip_desc* clips; const float* clip_lut;   /* fp32 [3][256], see gava_gemm_args */
  /* Weight-lo pass (gava_gemm_args.w_lo), inference drivers only (gava_vision_forward; the training drivers reject it).
   * w_lo = 1: w_patch and every 16-bit weight of gava_vision_layer except the *_split ones are packed [W_hi | W_lo] with
   * twice the columns ([3D][2D], [F][2D], [D][2F], ...; the folded copies too, their fold_s = row sums of hi + lo).
   * w_lo = 2 (fp16 operands): packed as 1, and the LayerNorm-folded qkv / fc1 GEMMs and fc2 over all B*T*(n+1) rows run their
   * lo product at 8 bits from the layer's *8 weights (gava_vision_layer8), their A operands leaving the producers (out_proj,
   * fc2, fc1) with a bf8 copy; every other GEMM (and every shape the persistent kernel does not take) as in w_lo = 1. */
  int w_lo;
  const struct gava_vision_layer8* layer8;     /* host array [layers], w_lo = 2 only */
} gava_vision_model;

/* e4m3 rows of 2^exp * W_lo for the 8-bit lo product (gava_gemm_args.W8 / w8_exp) of the GEMMs that run it - the
 * LayerNorm-folded qkv and fc1 (W_lo of the folded weight h16(gamma * W)) and fc2: [3D] / [F] rows of D bytes, [D] rows of F
 * bytes, each row 4x its length apart (ldw8 = 2 ldw, and the 16-bit weight rows are [W_hi | W_lo], gava_vision_model.w_lo).
 * *_fold_s8[n] = sum_k (W_hi[n][k] + 2^-exp W8[n][k]), the row sums of the weight these GEMMs multiply by.
 * out_proj keeps the 16-bit lo product (its A operand, the attention output, has no 8-bit copy). */
typedef struct gava_vision_layer8 {
  const void* w_qkv_fold8; const void* w_fc1_fold8; const void* w_fc28;
  const float* qkv_fold_s8; const float* fc1_fold_s8;
  int qkv_fold_exp, fc1_fold_exp, fc2_exp;
} gava_vision_layer8;

/* CLIPVisionEncoder.forward (VitaCLIP_vision_encoder.py:102-132).
 * x: fp32 (B,3,T_in,size,size) contiguous.  cls_x: fp32 [B][E] (un-normalised, :126-128),
 * summary: fp32 [B][D] (:129-130).  debug_cls (optional): fp32 [layers][B*T_in][D] receives the
 * CLS row of every frame after each block. */
size_t gava_vision_workspace_bytes(const gava_vision_model* m);
/* Measurement / test helper: 1 when gava_vision_forward keeps the residual stream of this model and batch as a 16-bit pair
 * between ln_pre and the last block (gava_gemm_args.resid16: big batches with every block's LayerNorms folded), else 0.  The
 * decision the driver makes (environment switch GAVA_PAIR_STREAM=0: never). */
int gava_vision_pair_stream(const gava_vision_model* m);
int gava_vision_forward(const gava_vision_model* m, const float* x, float* cls_x, float* summary,
                        float* debug_cls, void* workspace, size_t workspace_bytes,
                        gava_stream_t stream);

typedef struct {                 /* ResidualAttentionBlock, VitaCLIP_text_encoder.py:67-88 */
  const void* w_qkv; const float* b_qkv;   /* attn.in_proj_weight [3W][W]                    */
  const void* w_out; const float* b_out;
  const void* w_fc; const float* b_fc;     /* mlp.c_fc [4W][W]                               */
  const void* w_proj; const float* b_proj; /* mlp.c_proj [W][4W]                             */
  const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
} gava_text_layer;

typedef struct {
  int n_prompts, L, W, H, layers, E, n_ctx, prec;
  int split;                               /* 1: split-precision GEMMs; every weight below is then
                                              packed [W_hi | W_hi | W_lo] with 3x the columns    */
  int attn_f32;                            /* with split, inference, L <= 128: q/k/v leave their GEMM in fp32 and the
                                              attention core runs in fp32 (gava_attention_f32)  */
  const float* token_embedding;            /* [vocab][W] fp32                                */
  const float* positional_embedding;       /* [L][W]                                         */
  const float* lnf_g; const float* lnf_b;
  const void* w_tproj;                     /* text_projection transposed [E][W] h16          */
  const gava_text_layer* layer;            /* host array [layers]                            */
} gava_text_model;

/* TextPromptLearner.forward + CLIPTextEncoder.forward for all prompts in one batch
 * (VitaCLIP_text_encoder.py:310-332,154-171; the per-class Python loop of
 * VitaCLIP_model.py:282-285).  tokens: int32 [n_prompts][L]; ctx: fp32 [n_prompts][n_ctx][W];
 * eot_index: int32 [n_prompts], FLAT row n*L + column of the token vocab-1 (text_encoder.py:169).
 * out: fp32 [n_prompts][E].
 * tokens == NULL: direct mode = CLIPTextEncoder.forward(prompts, tokenized_prompts) called on ready-made prompt
 * embeddings (evaluation/zero_shot.py:75-76, utils/prepare_embedding.py): ctx is then fp32 [n_prompts][L][W], the
 * whole `prompts` argument; n_ctx is ignored. */
size_t gava_text_workspace_bytes(const gava_text_model* m);
int gava_text_forward(const gava_text_model* m, const int32_t* tokens, const float* ctx,
                      const int32_t* eot_index, float* out, void* workspace,
                      size_t workspace_bytes, gava_stream_t stream);

/* Similarity head (VitaCLIP_model.py:255,287-293): L2-normalise video [B][E] and text
 * [C*n_kv][E] rows (no epsilon), logits[b][c] = exp(logit_scale) * mean_k <v_b, t_{c,k}>
 * (+ logit_bias if not NULL), computed as one exact-fp32 GEMM against the class means of the unit
 * prompt features (the mean commutes with the dot product); text_features[c] = normalise(mean_k
 * t_{c,k}) [C][E].  n_kv = prompts per class (1 for plain prompts, the number of knowledge versions
 * for KAPT).  All fp32.  video_norm receives the normalised video features. */
int gava_similarity_head(const float* video, const float* text, const float* logit_scale,
                         const float* logit_bias, int B, int C, int n_kv, int E, float* logits,
                         float* text_features, float* video_norm, gava_stream_t stream);

/* Multi-view score fusion (evaluation/evaluate.py:275-288 with every view kept: softmax over the classes per view, :283, then
 * the mean over the num_spatial_views x num_temporal_views crops of a video that the upstream recipe takes).  All fp32:
 *   scores[b][c] = 1/V * sum_v exp(logit(b,v,c) - max_c' logit(b,v,c')) / sum_c' exp(logit(b,v,c') - max),
 * one launch for the batch, one workgroup per video: a wave per view reduces max and sum over the classes (lanes stride the
 * classes), the per-view (max, 1/sum) pairs meet in LDS, and every class then adds its V terms in view order - the result does
 * not depend on timing (no atomics).  Any V >= 1 and C >= 1; B == 0 succeeds without a launch. */
typedef struct {
  const float* logits; int64_t ld_video, ld_view;   /* logit(b,v,c) = logits[b*ld_video + v*ld_view + c] */
  int B, V, C;
  float* scores;      /* fp32 [B][C] contiguous: mean over the V views of softmax over the C classes */
  int* top1;          /* optional int32 [B]: argmax_c scores[b][c], lowest index on ties */
} gava_view_scores_args;
int gava_view_scores(const gava_view_scores_args* a, gava_stream_t stream);

/* ---- Backward of the trainable subset (training/train.py:441-490) --------------------------
 * Every transformer weight of the reference is frozen (VitaCLIP_model.py:230-239): the gradient only has to flow
 * THROUGH the GEMMs to the prompt parameters.  dgrad is gava_gemm on a transposed weight copy
 * (dX = dY . W == gemm(A = dY, W = W^T stored [in][out])); the three kernels below are the rest of the chain.
 * Gradient operands are 16-bit (bf16 recommended: fp32 range), accumulation and LayerNorm arithmetic fp32. */

/* LayerNorm backward (torch.nn.functional.layer_norm, eps 1e-5): dx = rstd*(g - mean(g) - xhat*mean(g*xhat)),
 * g = dy*gamma.  x rows may be gathered (x_row_index) and dx rows scattered (dx_row_index); accumulate != 0 adds
 * into dx (the residual branch).  dgamma/dbeta (both or neither) are accumulated with atomics.  dx16 (optional,
 * not with dx_row_index): an h16 copy of the final dx rows, i.e. the A operand of the next dgrad GEMM. */
typedef struct {
  const float* x; int64_t x_stride; const int32_t* x_row_index;
  const float* gamma;
  const float* dy; int64_t dy_stride;
  float* dx; int64_t dx_stride; const int32_t* dx_row_index;
  float* dgamma; float* dbeta;
  int rows, D, accumulate;
  void* dx16; int64_t dx16_stride; int prec;
} gava_layernorm_bwd_args;
int gava_layernorm_backward(const gava_layernorm_bwd_args* a, gava_stream_t stream);

/* QuickGELU backward: dpre = dh * s*(1 + 1.702*pre*(1-s)), s = sigmoid(1.702*pre); h16 in/out, n % 4 == 0. */
int gava_qgelu_backward(const void* pre, const void* dh, void* dpre, size_t n, int prec, gava_stream_t stream);

/* Softmax-attention backward (MFMA kernels).  q (already scaled by 1/sqrt(dh)), k, v, dout: h16 rows [batch*n][ld],
 * head h at columns [64h, 64h+64); writes dq (times q_scale, the factor folded into q), dk, dv as h16 rows
 * [batch*n][ld_dqkv].  Non-causal: any n; past 320 keys (n + prompt rows) or 288 query rows the dQ and dK/dV
 * kernels stream the other side through LDS in blocks.  causal: n <= 288.
 *   - plain or causal sequences without prompt rows (side_k == NULL): the text tower (nn.MultiheadAttention at
 *     text_encoder.py:71,83) and the T-token summary attention (vision_encoder_utils.py:169-170);
 *   - vision blocks (vision_encoder_utils.py:190-191): keys = the n rows of the frame + the gathered prompt rows
 *     [n_g global | T local rows of the clip | the frame's summary row] of side_k/side_v (same layout as
 *     gava_attention).  Prompt rows are shared between frames, so their gradients come out as
 *     per-frame partials dside_k / dside_v fp32 [batch][n_g + T + 1][ld_dside] (plain stores; row order global,
 *     local, summary) which the caller sums over the frames sharing a row.  n_q != 0: only the first n_q rows of
 *     each frame are queries.
 * `workspace`: gava_attention_backward_workspace_bytes(batch, heads, n_q) bytes of scratch (per-query softmax
 * statistics handed from the dQ kernel to the dK/dV kernel). */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* dout; int64_t ld_dout;
  void* dq; void* dk; void* dv; int64_t ld_dqkv;
  int batch, heads, n, causal, prec;
  float q_scale;
  const void* side_k; const void* side_v; int64_t ld_side;
  float* dside_k; float* dside_v; int64_t ld_dside;
  int n_g, T, has_summary, n_q;
  void* workspace;
  int act_prec_set, act_prec;   /* vision path only: q/k/v/side_* are stored as act_prec (fp16 activations kept from the
                                 * forward) while dout / dq / dk / dv use prec (bf16); 0 = same as prec */
  int q_batch_rows; int64_t ld_q, ld_dq; /* vision path, != 0: q, dout and dq are separate buffers holding q_batch_rows rows
                                 * per frame (strides ld_q, ld_dout, ld_dq), as gava_attention's q_batch_rows: the CLS-only
                                 * last block */
} gava_attention_bwd_args;
int gava_attention_backward(const gava_attention_bwd_args* a, gava_stream_t stream);
size_t gava_attention_backward_workspace_bytes(int batch, int heads, int n_q);

/* gava_text_forward that also keeps what the backward recomputes from: saved_x fp32 [layers+1][n_prompts*L][W] =
 * the input of every residual block and the final stream (before ln_final). */
int gava_text_forward_train(const gava_text_model* m, const int32_t* tokens, const float* ctx,
                            const int32_t* eot_index, float* out, float* saved_x, void* workspace,
                            size_t workspace_bytes, gava_stream_t stream);

/* (mean, rstd) per row from the producers' partial sums: rowsum float2 [rows][slots] -> stats float2 [rows], D columns,
 * eps 1e-5, variance = max(E[x^2] - mean^2, 0) in fp32 with a fixed summation order (deterministic).  The difference cancels:
 * its error is 2^-24 (E[x^2] + mean^2) times a small constant, whatever the variance - rows on a large common offset lose
 * that much of rstd (profiles/rowops_edges_errors.txt, row_stats / offset).  1 <= slots <= 32. */
int gava_row_stats(const float* rowsum, int slots, int D, int rows, float* stats, gava_stream_t stream);

/* gava_vision_forward that also keeps what the backward recomputes from: saved_x fp32 [layers+2][B*T_in*(n+1)][D] =
 * the embedding before ln_pre, the input of every block, and the final residual stream. */
int gava_vision_forward_train(const gava_vision_model* m, const float* x, float* cls_x, float* summary,
                              float* debug_cls, float* saved_x, void* workspace, size_t workspace_bytes,
                              gava_stream_t stream);

/* Training forward that keeps the backward's activations instead of leaving them to be recomputed.  With
 * R = B*T_in*(n+1), SR = G + 2*B*T_in:  e0 fp32 [R][D] (embedding before ln_pre);  x fp32 [layers+1][R][D] (block inputs,
 * last slot = final stream);  x1 fp32 [L1][R][D] (stream after the attention branch);  qkv h16 [layers][R][3D];
 * pre h16 [L1][R][F] (fc1 output before QuickGELU);  sidekv h16 [layers][SR][2D] (prompt-row keys/values).
 * L1 = layers when last_* (below) are NULL; with last_* the last block's x1 / pre slot is never touched, so L1 = layers-1
 * slots suffice (at least one: the pointers must not be NULL).  training.alloc_kept allocates max(layers-1, 1).
 * Nothing is copied: the residual stream hops x[i] -> x1[i] -> x[i+1]. */
typedef struct {
  float* e0; float* x; float* x1; void* qkv; void* pre; void* sidekv;
  /* optional (all three or none): run the LAST block on the CLS rows only, as gava_vision_forward does, and keep its
   * CLS-row activations here: last_q h16 [B*T_in][D] (scaled queries), last_x1 fp32 [B*T_in][D], last_pre h16
   * [B*T_in][F].  The block's K/V then sit in columns D..3D of its qkv slot (its q columns are not written); x1 / pre
   * have no slot for that block, and only the CLS rows of the final stream x[layers] are written. */
  void* last_q; float* last_x1; void* last_pre;
} gava_vision_saved;
int gava_vision_forward_keep(const gava_vision_model* m, const float* x, float* cls_x, float* summary,
                             const gava_vision_saved* saved, void* workspace, size_t workspace_bytes,
                             gava_stream_t stream);

/* Clip preprocessing of the evaluation data path (video_dataset/dataset.py:117-139, the
 * num_spatial_views = num_temporal_views = 1 case that every eval script uses): from the decoded RGB frames of
 * one video, uint8 [n_frames][height][width][3], to the model input slot fp32 [3][T][size][size]:
 *   temporal crop   frame(t) = min(st + t*rate, n_frames-1), st = max(n_frames - ((T-1)*rate+1), 0) / 2
 *                   (:163-177, a short video repeats its last frame);
 *   value           (u8/255 - mean[c]) / std[c]                                       (:119,121);
 *   resize          short side -> size, bilinear, align_corners=False, no antialias   (:124-133), i.e.
 *                   src = max((dst+0.5)*in/out - 0.5, 0), taps floor(src) and min(+1, in-1);
 *   crop            centre size x size window                                          (:181-186).
 * out_stride_c / out_stride_t are element strides of the output (frames are contiguous size*size planes), so
 * the kernel can write straight into clip b of a [B][3][T][size][size] batch.  HBM-bound byte work. */
typedef struct {
  const uint8_t* frames; int n_frames, height, width;
  float mean[3], std[3];
  int T, rate, size;
  float* out; int64_t out_stride_c, out_stride_t;
  /* the dataset returns only the FIRST of its num_spatial_views x num_temporal_views crops (`frames = frames[0]`,
   * :136-139): with more than one temporal view that is the crop starting at frame 0 (:171-172), with three spatial
   * views the top / left one (:188-199).  first_temporal_view / first_spatial_view != 0 select those; 0 = centred. */
  int first_temporal_view, first_spatial_view;
  /* optional device table fp32 [3][256] with (v/255 - mean[c]) / std[c] for every byte value (see gava_gemm_args.clip_lut):
   * when given, the kernel looks the normalised value up instead of dividing - the same bits as the fused uint8 patch loader */
  const float* lut;
} gava_preprocess_args;
int gava_preprocess_clip(const gava_preprocess_args* a, gava_stream_t stream);

/* The same pixels for a whole batch in ONE launch: B descriptors (device array, either branch, videos of different sizes)
 * -> out fp32 [B][3][T][size][size] by element strides (size*size planes contiguous).  lut = the fp32 [3][256] table of
 * gava_preprocess_args.lut, required.  Grid = clips x frames x rows; B*T <= 65535.  Same bits as B gava_preprocess_clip calls. */
typedef struct {
  const gava_clip_desc* clips; const float* lut;
  int B, T, size;
  float* out; int64_t out_stride_b, out_stride_c, out_stride_t;
} gava_preprocess_clips_args;
int gava_preprocess_clips(const gava_preprocess_clips_args* a, gava_stream_t stream);

/* The unfold half of ImagePatchEmbed2D (VitaCLIP_vision_encoder_utils.py:31-53: Conv2d(3, D, P, stride P) == patches x
 * W^T) as one HBM-bound pass: the 16-bit patch matrix the patch-embedding GEMM (gava_gemm, EPI_F32_PATCH with A given)
 * then reads by LDS-DMA like any other operand.
 *   out[(b*T + t) * n_patches + py*g + px][c*P*P + ky*P + kx] = h16( in(b, c, t, py*P + ky, px*P + kx) ),  g = size / P,
 * columns [3*P*P, ldo) are zeroed (K is padded to a multiple of 64 for ViT-L/14).  The input is either
 *   x      fp32 [B][3][T][size][size], the tensor VitaCLIP.forward takes (VitaCLIP_model.py:241), or
 *   clips  decoded uint8 videos: device array of B descriptors (gava_clip_desc) + clip_lut fp32 [3][256], evaluated with
 *          the arithmetic of gava_preprocess_clip (video_dataset/dataset.py:117-139) - the same bits as preprocessing to
 *          fp32 first, a quarter of the HBM traffic and no fp32 clip in memory.
 * Rounding to 16 bits is the one the GEMM's own fp32 loader applies (round to nearest even), so the product is unchanged. */
typedef struct {
  const float* x;
  const gava_clip_desc* clips; const float* clip_lut;
  int B, T, size, patch, prec;
  void* out; int64_t ldo;             /* ldo >= 3*patch*patch, multiple of 8; out 16-byte aligned */
} gava_patchify_args;
int gava_patchify(const gava_patchify_args* a, gava_stream_t stream);

/* fp32 -> h16 conversion of a contiguous array (weight packing at load time).  Round to nearest even, ties included; results
 * below the 16-bit normal range are subnormals (nothing is flushed), fp16 overflows to inf from 65520 on, NaN stays NaN.
 * n = 0 is accepted and writes nothing. */
int gava_convert_h16(const float* in, void* out, size_t n, int prec, gava_stream_t stream);

/* ---- training head and criterion (opt-in: VitaCLIP.train_head = "hip", gava_clip_amd.TrainCriterion) ----------------------
 *
 * Criterion of the reference's training loop (training/train.py:360-362,446-452, training/loss_utils.py:9-46): per-sample
 * cross-entropy, optionally times the ordinal-focal weight, then the mean.  Per sample i with label y (clamped to [0, C) on
 * the device), all in fp32:
 *   p = softmax(z_i);  ce_i = logsumexp(z_i) - z_iy;  k_i = argmax_c z_ic (the lowest index on ties)
 *   w_i = scale * (beta * |y - k_i| / (C - 1) + alpha * (1 - p_y)^gamma);   l_i = weighted ? ce_i * w_i : ce_i
 *   loss = mean_i l_i;  hits = #{i : k_i == y};  conf[y][k_i] += 1 (optional, int32 [C][C], ACCUMULATED by integer atomics)
 * The forward leaves four floats per sample in `saved` (row max, log of the sum of exp, the gradient's factor a_i, 1 - p_y);
 * the backward reads them, the logits, the labels and the upstream gradient of `loss` FROM DEVICE MEMORY (grad_loss, one
 * float: GradScaler's scale never visits the host) and writes
 *   dlogits[i][c] = a_i * (p_c - [c == y]) * grad_loss / B,   a_i = w_i + ce_i * scale * alpha * gamma * (1 - p_y)^(gamma-1) * p_y
 * (a_i = 1 unweighted; the ordinal term has no gradient, as in the reference, whose autograd passes the focal factor only).
 * GAVA_EINVAL: weighted with gamma < 1 (the derivative is unbounded at p_y = 1) or C < 2, B < 1, C < 1, a null pointer among
 * the required ones (forward: logits, labels, loss, per_sample, weight, top1, hits, saved; backward: logits, labels, saved,
 * grad_loss, dlogits).  No floating-point atomics: the same bits on every run.  Two launches forward, one backward, no
 * host synchronisation. */
typedef struct {
  const float* logits; int64_t ld_logits;     /* fp32 [B][C], rows ld_logits elements apart */
  const int64_t* labels;                      /* [B] */
  int B, C, weighted;
  float alpha, gamma, beta, scale;
  float* loss; float* per_sample; float* weight; int32_t* top1; int32_t* hits;
  int32_t* conf;                              /* optional */
  float* saved;                               /* [B][4] */
  const float* grad_loss; float* dlogits; int64_t ld_dlogits;     /* backward only */
} gava_train_criterion_args;
int gava_train_criterion(const gava_train_criterion_args* a, gava_stream_t stream);
int gava_train_criterion_backward(const gava_train_criterion_args* a, gava_stream_t stream);

/* The similarity head under autograd (VitaCLIP_model.py:248,255,287-293,308-309), fp32.  video [B][E] and text [P][E] are
 * the towers' raw outputs; class_offsets int32 [C+1] (device) gives the prompts of class c as rows offsets[c] .. offsets[c+1]
 * of text, offsets[C] == P (one prompt per class, n_kv per class, or the ragged descriptor mode).
 *   logits[b][c] = exp(logit_scale) * <vn_b, m_c> + logit_bias,  vn = video / |video|,  m_c = mean of the unit prompt rows of c
 *   text_features[c] = m_c / |m_c|
 * The forward runs the kernels of gava_similarity_head: with equal counts, logits and text_features have that head's bits.
 * It keeps video_norm [B][E], video_inv [B], text_norm [P][E], text_inv [P] (unit rows and 1 / |row|) and class_mean [C][E].
 * A class without prompts (offsets[c] == offsets[c+1]) has the class mean 0: its logits are logit_bias, its text_features row
 * is undefined (0 / 0), and no prompt row receives its gradient.
 * The backward takes dlogits [B][C] (contiguous) and optionally dtext_features [C][E] (NULL = zero) plus what the forward
 * kept and its logits - it reads neither video, text nor text_features, which may be NULL there - and writes dvideo [B][E], dtext [P][E], dlogit_scale (1), dlogit_bias (1, optional):
 *   dvn = s * dlogits @ m,  dm = s * dlogits^T @ vn + (dtf - tf <tf, dtf>) / |m|,  s = exp(logit_scale)   (fp32 MFMA tiles,
 *   zero-filled past B, C, E)
 *   dlogit_scale = sum dlogits * (logits - logit_bias),  dlogit_bias = sum dlogits              (one wave, fixed order)
 *   dvideo = (dvn - vn <vn, dvn>) / |video|;  per prompt k of class c: dtn = dm_c / count_c, dtext = (dtn - tn <tn, dtn>) / |text_k|
 * workspace: (B + C) * E floats.  E % 4 == 0.  Two launches; no atomics, the same bits on every run. */
typedef struct {
  const float* video; const float* text; const int32_t* class_offsets;
  const float* logit_scale; const float* logit_bias;        /* logit_bias optional */
  int B, C, P, E;
  float* logits; float* text_features;
  float* video_norm; float* video_inv; float* text_norm; float* text_inv; float* class_mean;
  const float* dlogits; const float* dtext_features;        /* backward only from here; dtext_features optional */
  float* dvideo; float* dtext; float* dlogit_scale; float* dlogit_bias;
  float* workspace;
} gava_train_head_args;
int gava_train_head(const gava_train_head_args* a, gava_stream_t stream);
int gava_train_head_backward(const gava_train_head_args* a, gava_stream_t stream);

/* sizeof of the two structs above, in that order, like gava_struct_sizes (whose list is closed at its 17 entries: a binding
 * compares that call's return value with its own count).  Writes min(cap, 2) entries, returns 2. */
int gava_train_struct_sizes(size_t* out, int cap);

/* ---- auxiliary heads and their loss terms (opt-in: VitaCLIP.aux_heads = "hip", gava_clip_amd.AuxCriterion) ------------------
 *
 * All fp32, no atomics (the same bits on every run), no host synchronisation; upstream gradients are read from device memory.
 * The number of launches of an entry point does not depend on B, M, C or S.  Pointers that rows are read from 16 bytes at a
 * time (summary, weight, video_nte, memory, text_features, the weights, the kept buffers) must be 16-byte aligned.
 *
 * Video <-> NTE head (VitaCLIP_model.py:311-345).  summary [B][D], weight [E][D] and bias [E] of sum_proj (bias optional),
 * video_nte [B][K][E], logit_scale one float (multiplied as it is, no exp).
 *   sp = unit rows of summary weight^T + bias;  n[j] = mean over k of the unit rows of video_nte[j];  valid[j] = (the sum of
 *   all elements of video_nte[j] != 0);  sim = sp n^T valid_i valid_j  (the mean of the K products of the reference, by
 *   linearity);  lm = logit_scale * sim;  logits_vm = log_softmax(lm, rows) + log_softmax(lm, columns)
 * The forward keeps sp_norm [B][E], sp_inv [B] (1 / |row|), nte_mean [B][E], valid [B] (0 / 1), sim [B][B] (masked), lm [B][B],
 * row_lse [B], col_lse [B].  The backward takes dlogits [B][B] and what was kept (video_nte and logits_vm may be NULL there):
 *   dlm = 2 g - exp(lm - row_lse_i) sum_j g_ij - exp(lm - col_lse_j) sum_i g_ij;   dlogit_scale = sum dlm sim
 *   dsp = (dlm logit_scale valid_i valid_j) n;   dy = (dsp - sp <sp, dsp>) sp_inv;   dweight = dy^T summary, dbias = sum_b dy,
 *   dsummary = dy weight
 * workspace: B * (B + E + 3) floats.  D % 4 == 0, E % 4 == 0, E <= 1024, B <= 32767.  A video_nte row of norm zero gives
 * unspecified (NaN) outputs, as in the reference; every index stays in range.  Five launches forward, five backward. */
typedef struct {
  const float* summary; const float* weight; const float* bias; const float* video_nte; const float* logit_scale;
  int B, D, E, K;
  float* logits_vm;
  float* sp_norm; float* sp_inv; float* nte_mean; float* valid; float* sim; float* lm; float* row_lse; float* col_lse;
  const float* dlogits;                                      /* backward only from here */
  float* dsummary; float* dweight; float* dbias; float* dlogit_scale;
  float* workspace;
} gava_nte_head_args;
int gava_nte_head(const gava_nte_head_args* a, gava_stream_t stream);
int gava_nte_head_backward(const gava_nte_head_args* a, gava_stream_t stream);

/* Support-memory <-> text head (VitaCLIP_model.py:347-398).  memory [M][S][E], text_features [C][E]; an MLP is Linear E -> H1 =
 * E / 4, tanh, Linear H1 -> H2 = E / 8.  tf_project's four parameters are passed directly (tf_w1 [H1][E], tf_b1 [H1], tf_w2
 * [H2][H1], tf_b2 [H2]); memory_project[c]'s through mem_params, a DEVICE table of C x 4 pointers in that order (built once
 * by the caller: nothing is launched or copied per class).  logit_scale one float (no exp), logit_bias optional.
 *   mm = mean_s memory;  z_c = memory_project[c](mm) [M][H2];  u_c = tf_project(text_features[c]) [H2]
 *   cos[m][c] = <z_c[m], u_c> / (|z_c[m]| |u_c|);   logits_mt = log_softmax(logit_scale * cos, classes) + logit_bias
 * The forward keeps mem_mean [M][E], mem_h [C][M][H1] (tanh outputs), mem_z [C][M][H2], mem_inv [M][C] (1 / |z_c[m]|), tf_h
 * [C][H1], tf_u [C][H2], tf_inv [C], cosine [M][C], lse [M].  The backward takes dlogits [M][C] and what was kept (memory and
 * logits_mt may be NULL there) and writes the stacked gradients dmem_w1 [C][H1][E], dmem_b1 [C][H1], dmem_w2 [C][H2][H1],
 * dmem_b2 [C][H2], tf_project's dtf_* (summed over the classes in class order), dlogit_scale, dlogit_bias (required when
 * logit_bias is given) and dtext_features [C][E] (optional: NULL = not computed):
 *   draw = g - softmax sum_c g;  dlogit_scale = sum draw cos;  dlogit_bias = sum g;  dcos = draw logit_scale
 *   dz_c[m] = dcos (u^ - z^ cos) / |z|;   du_c = (d - u^ <u^, d>) / |u|,  d = sum_m dcos[m][c] z^_c[m];   then each MLP's backward
 * workspace: gava_memory_head_backward_workspace_floats.  E % 16 == 0, C <= 65535.  Six launches forward, ten backward (nine
 * without dtext_features). */
typedef struct {
  const float* memory; const float* text_features;
  const float* tf_w1; const float* tf_b1; const float* tf_w2; const float* tf_b2;
  const float* const* mem_params;
  const float* logit_scale; const float* logit_bias;
  int M, S, C, E;
  float* logits_mt;
  float* mem_mean; float* mem_h; float* mem_z; float* mem_inv; float* tf_h; float* tf_u; float* tf_inv; float* cosine; float* lse;
  const float* dlogits;                                      /* backward only from here */
  float* dmem_w1; float* dmem_b1; float* dmem_w2; float* dmem_b2;
  float* dtf_w1; float* dtf_b1; float* dtf_w2; float* dtf_b2;
  float* dlogit_scale; float* dlogit_bias; float* dtext_features;
  float* workspace;
} gava_memory_head_args;
int gava_memory_head(const gava_memory_head_args* a, gava_stream_t stream);
int gava_memory_head_backward(const gava_memory_head_args* a, gava_stream_t stream);
size_t gava_memory_head_backward_workspace_floats(int M, int C, int E);
size_t gava_nte_head_backward_workspace_floats(int B, int E);

/* sigmoid_focal_loss of training/loss_utils.py:139-177 on integer labels, then the mean over the samples.  With t = +1 at the
 * label and -1 elsewhere, ce = softplus(-t x) (= -logsigmoid(t x), written so that large |x| loses no accuracy) and
 * q = sigmoid(-t x) = 1 - p_t:
 *   per_sample[m] = scale * sum_c (use_focal ? alpha_t q^gamma ce : ce),  alpha_t = alpha at the label, 1 - alpha elsewhere
 *   loss = mean_m per_sample;   dlogits = grad_loss / M * scale * -t (use_focal ? alpha_t q^gamma (gamma (1 - q) ce + q) : q)
 * A label outside [0, C) marks no class.  GAVA_EINVAL: use_focal with gamma < 1, M < 1, C < 1, a null pointer among the required
 * ones.  Two launches forward (rows, mean), one backward. */
typedef struct {
  const float* logits; int64_t ld_logits;     /* fp32 [M][C], rows ld_logits elements apart */
  const int64_t* labels;                      /* [M] */
  int M, C, use_focal;
  float alpha, gamma, scale;
  float* loss; float* per_sample;
  const float* grad_loss; float* dlogits; int64_t ld_dlogits;     /* backward only */
} gava_sigmoid_criterion_args;
int gava_sigmoid_criterion(const gava_sigmoid_criterion_args* a, gava_stream_t stream);
int gava_sigmoid_criterion_backward(const gava_sigmoid_criterion_args* a, gava_stream_t stream);

/* loss = -weight * mean_i logits_vm[i][i] (training/train.py:471-475), logits_vm [B][B] contiguous; the backward writes the
 * whole dlogits_vm [B][B] (-weight * grad_loss / B on the diagonal, zero elsewhere).  One launch each. */
typedef struct {
  const float* logits_vm; int B; float weight;
  float* loss;
  const float* grad_loss; float* dlogits_vm;                      /* backward only */
} gava_nte_diag_args;
int gava_nte_diag_loss(const gava_nte_diag_args* a, gava_stream_t stream);
int gava_nte_diag_loss_backward(const gava_nte_diag_args* a, gava_stream_t stream);

/* sizeof of the four structs above, in that order, like gava_train_struct_sizes.  Writes min(cap, 4) entries, returns 4. */
int gava_aux_struct_sizes(size_t* out, int cap);

/* ---- fused AdamW step (opt-in: gava_clip_amd.FusedAdamW) ---------------------------------------------------------------------
 *
 * Multi-tensor AdamW (torch.optim.AdamW with amsgrad = False, maximize = False) over a DEVICE-resident table of tensor
 * descriptors, in two launches however many tensors the table holds (the update over a chunk list, then the step counts),
 * with no allocation and no host synchronisation.  Per element, in fp32, with t = *step + 1 read from the device:
 *   g <- g * (1 / *grad_scale);  p <- p * (1 - lr * wd);  m <- m + (g - m) * (1 - beta1);  v <- beta2 * v + (1 - beta2) * g * g
 *   p <- p - (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * 1 - lr * wd and the two bias corrections are evaluated in double, once per workgroup.  g is read only: the unscaled gradient is not
 * written back.  If *found_inf != 0 the call changes nothing (not p, m, v, the step counts or any copy); otherwise every step
 * count of a tensor with a gradient goes up by one in the trailing launch, after every chunk has computed from the old one.
 *
 * A table entry describes one parameter.  g == NULL skips it entirely (no decay, no step increment, no copy: torch's behaviour
 * for p.grad is None).  Besides the update the kernel writes up to four copies of the UPDATED parameter from the values it
 * holds in registers, the parameter seen as a rows x cols matrix (rows * cols == n; NULL = no such copy):
 *   copy_f32     fp32,                      copy_f32[r * ld_f32 + c]
 *   copy16       prec16 (GAVA_PREC_*),      copy16[r * ld16 + c]
 *   copy_bf16    bf16,                      copy_bf16[r * ld_bf16 + c]
 *   copy_bf16_t  bf16, the transpose,       copy_bf16_t[c * ld_bf16_t + r]      (through an LDS tile: both sides coalesced)
 * with explicit leading dimensions (in elements), so that separate q, k and v parameters land in the row blocks of one
 * [3D][D] copy and in the column blocks of one [D][3D] transposed copy.  The 16-bit values are the bits gava_convert_h16
 * gives for the updated parameter.  16-byte loads and stores are used wherever the addresses allow, element-wise ones elsewhere:
 * no alignment is required beyond the element's own.
 *
 * The chunk list (DEVICE, one workgroup per entry) is written by gava_adamw_plan from the HOST copy of the table: at most 4096
 * elements of one tensor per chunk, as a linear range or, for a tensor with a transposed copy, a 64 x 64 tile.  Tensors
 * without a gradient get no chunk.  gava_adamw_plan writes min(cap, count) entries and returns count (call it with cap = 0 to
 * size the buffer), or GAVA_EINVAL.
 *
 * gava_adamw_step reads table_host (the same descriptors in host memory; it is not kept) to validate before any launch.
 * GAVA_EINVAL: null args, a null table or table_host with n_tensors > 0, null chunks with n_chunks > 0, n_groups outside
 * [1, GAVA_ADAMW_MAX_GROUPS], and per tensor with a gradient: a null p, m, v or step, n < 0, a group index outside [0, n_groups),
 * with a 16-bit copy16 a prec16 outside {GAVA_PREC_F16, GAVA_PREC_BF16}, with any copy target rows * cols != n or a leading
 * dimension smaller than the row it holds.  The hyper-parameters travel BY VALUE: a schedule that changes lr every step
 * uploads nothing. */
#define GAVA_ADAMW_MAX_GROUPS 8
typedef struct {
  float* p; const float* g; float* m; float* v;     /* fp32, n elements each, contiguous */
  float* step;                                      /* this tensor's step count, one fp32 */
  float* copy_f32; void* copy16; void* copy_bf16; void* copy_bf16_t;
  int64_t ld_f32, ld16, ld_bf16, ld_bf16_t;
  int n, group, rows, cols, prec16, reserved;
} gava_adamw_tensor;
typedef struct { int tensor, a, b, reserved; } gava_adamw_chunk;   /* linear: elements [a, a + b); tile: rows from a, columns from b */
typedef struct { double lr, beta1, beta2, eps, weight_decay; } gava_adamw_group;
typedef struct {
  const gava_adamw_tensor* table;        /* DEVICE, n_tensors entries */
  const gava_adamw_tensor* table_host;   /* the same entries in host memory (validation only) */
  const gava_adamw_chunk* chunks;        /* DEVICE, n_chunks entries (gava_adamw_plan) */
  int n_tensors, n_chunks, n_groups, reserved;
  gava_adamw_group groups[GAVA_ADAMW_MAX_GROUPS];
  const float* grad_scale; const float* found_inf;   /* device scalars, either may be NULL */
} gava_adamw_args;
int gava_adamw_plan(const gava_adamw_tensor* table_host, int n_tensors, int n_groups, gava_adamw_chunk* out, int cap);
int gava_adamw_step(const gava_adamw_args* a, gava_stream_t stream);

/* sizeof of gava_adamw_tensor, gava_adamw_args, gava_adamw_chunk, in that order, like gava_aux_struct_sizes.  Writes
 * min(cap, 3) entries, returns 3. */
int gava_optim_struct_sizes(size_t* out, int cap);

/* ---- gradient clipping by global norm inside the fused step (FusedAdamW(max_grad_norm=...)) ------------------------------------
 *
 * gava_grad_norm measures, gava_adamw_step_clipped applies: torch's unscale_ + clip_grad_norm_(norm_type = 2) + step without
 * writing a gradient.  Both read the table and the chunk list of gava_adamw_step (the chunk list as gava_adamw_plan writes it:
 * in table order, either chunk form), so the norm counts exactly the elements the step updates, each once.
 *
 * gava_grad_norm.  For every table entry with g != NULL and every element i of it, x_i = fl32(g_i * inv_scale) with
 * inv_scale = 1.0f / *grad_scale (1 when grad_scale is NULL): the single-precision product the step forms.  x_i * x_i is
 * accumulated in double in a fixed order: within a lane in element order, across the 256 lanes of a chunk's workgroup through a
 * fixed tree (one partial per chunk), the chunk partials of a tensor in chunk order, the tensors in table order.  No
 * floating-point atomics, nothing depends on which workgroup finishes first: the same inputs give the same bits on every run
 * and on every rank.  With total the sum over everything, all outputs DEVICE memory:
 *   tensor_norm[i] = fl32(sqrt(sum over entry i)), n_tensors values, optional (NULL); 0 for an entry without a gradient
 *   stats[0] = fl32(sqrt(total))
 *   stats[1] = fl32(min(1, max_norm / (sqrt(total) + 1e-6))), evaluated in double: clip_grad_norm_'s coefficient
 *   stats[2] = 1 if total is not finite (an inf or a NaN anywhere), else 0; when it is 1, stats[1] is written as 1
 *   stats[3] = 0 (reserved)
 * max_norm = +inf measures only: the coefficient is then exactly 1.  found_inf plays no part: the stats are written either way.
 * workspace: 8 * (n_chunks + n_tensors) bytes of DEVICE memory, 8-byte aligned; every word that is read is written first in
 * the same call, as is every output, so nothing needs a memset and nothing is carried from call to call.  At most two launches
 * (the per-chunk sums; one workgroup for the rest) whatever n_tensors is, no allocation, no host synchronisation.  Gradients
 * are loaded 16 bytes per lane where the address allows and element-wise elsewhere.
 * The chunk list must be in table order (non-decreasing tensor index), as gava_adamw_plan writes it, and the DEVICE table must
 * equal table_host: neither can be checked from the host.  Otherwise the sums are undefined (a tensor's partials are found as
 * one range of the list; an entry the step would skip for its group index is still counted); nothing is read or written outside
 * the table, the list, the gradients the table names and the workspace.
 * GAVA_EINVAL, before any launch: null args, a null table or table_host with n_tensors > 0, max_norm <= 0 or NaN, n_chunks < 0,
 * null chunks, stats or workspace with n_chunks > 0, a workspace that is not 8-byte aligned, and whatever gava_adamw_step
 * refuses in the table.  With n_chunks == 0 the outputs that are given are still written (norm 0, coefficient 1).
 *
 * gava_adamw_step_clipped is gava_adamw_step with two differences: the gradient it uses is fl32(fl32(g * inv_scale) * stats[1]),
 * the two roundings of torch's unscale-then-clip, and when stats[2] != 0 the whole step is skipped exactly as for
 * *found_inf != 0 (not p, m, v, the step counts or any copy changes).  With stats[1] == 1 and g * inv_scale exact (grad_scale
 * NULL or a power of two, as GradScaler's always is) it gives gava_adamw_step's bits.
 * stats: the four DEVICE floats gava_grad_norm wrote; NULL is GAVA_EINVAL, the rest of the checks are gava_adamw_step's.
 * Unlike torch, whose clip_grad_norm_(error_if_nonfinite = False) scales by NaN and poisons every parameter, a non-finite norm
 * costs one skipped step. */
typedef struct {
  const gava_adamw_tensor* table;        /* DEVICE, n_tensors entries */
  const gava_adamw_tensor* table_host;   /* the same entries in host memory (validation only) */
  const gava_adamw_chunk* chunks;        /* DEVICE, n_chunks entries */
  int n_tensors, n_chunks, n_groups, reserved;
  const float* grad_scale;               /* device scalar, may be NULL */
  double max_norm;
  void* workspace;
  float* tensor_norm;                    /* may be NULL */
  float* stats;
} gava_grad_norm_args;
int gava_grad_norm(const gava_grad_norm_args* a, gava_stream_t stream);
int gava_adamw_step_clipped(const gava_adamw_args* a, const float* stats, gava_stream_t stream);

/* sizeof of gava_grad_norm_args, like gava_optim_struct_sizes.  Writes min(cap, 1) entries, returns 1. */
int gava_grad_clip_struct_sizes(size_t* out, int cap);

/* ---- gradient with respect to the input clip: the fold half of ImagePatchEmbed2D ----------------------------------------------
 *
 * The transpose of gava_patchify's index map, as one HBM-bound pass over fp32 data.  dpatch is d(embedding rows) x the patch
 * weight: fp32, B*T frames of frame_rows rows each, rows ld floats apart.  Of every frame the kernel reads the n = (size/P)^2
 * rows row_offset ... row_offset + n - 1 (frame_rows = n + 1, row_offset = 1 skips the CLS row of the embedding output;
 * frame_rows = n, row_offset = 0 is the dense form) and of every row the columns [0, 3*P*P): columns [3*P*P, ld) are the GEMM's
 * padding and are never read.  With g(b, c, t, py*P + ky, px*P + kx) = dpatch[(b*T + t) * frame_rows + row_offset + py*(size/P) + px]
 * [c*P*P + ky*P + kx]:
 *   GAVA_UNPATCH_GRAD          out fp32 [B][3][T][size][size] = g: a permutation of the input values, bit for bit
 *   GAVA_UNPATCH_ABSMAX        out fp32 [B][T][size][size]    = max over c of |g|
 *   GAVA_UNPATCH_L2            out                            = sqrt(g_0^2 + g_1^2 + g_2^2)
 *   GAVA_UNPATCH_GRAD_X_INPUT  out                            = g_0 x_0 + g_1 x_1 + g_2 x_2, x the fp32 clip [B][3][T][size][size]
 * The channel sums run in the order c = 0, 1, 2 in fp32 (fused multiply-adds, a correctly rounded square root); no atomics, so
 * a call repeats bit for bit.  The three map modes never form the [B][3][T][size][size] gradient.  One workgroup owns P whole
 * image rows of a frame: its stores are contiguous rows, its loads P-float segments; 16-byte accesses when P and ld are
 * multiples of 4, 8-byte when they are even (P = 14), single floats otherwise.  Any number of frames goes in one launch.
 * GAVA_EINVAL, before any launch: null args, a null dpatch or out, a pointer (x included) that is not 16-byte aligned,
 * B, T, size or patch < 1 or B*T past 2^31 - 1, size % patch != 0, ld < 3*patch*patch, row_offset < 0 or
 * row_offset + n > frame_rows, a mode outside the four, x given in a mode other than GRAD_X_INPUT or missing in it. */
#define GAVA_UNPATCH_GRAD 0
#define GAVA_UNPATCH_ABSMAX 1
#define GAVA_UNPATCH_L2 2
#define GAVA_UNPATCH_GRAD_X_INPUT 3
typedef struct {
  const float* dpatch; int64_t ld;
  const float* x;                      /* GAVA_UNPATCH_GRAD_X_INPUT only, NULL otherwise */
  float* out;
  int B, T, size, patch, mode, frame_rows, row_offset, reserved;
} gava_unpatchify_args;
int gava_unpatchify(const gava_unpatchify_args* a, gava_stream_t stream);

/* sizeof of gava_unpatchify_args, like gava_optim_struct_sizes.  Writes min(cap, 1) entries, returns 1. */
int gava_input_grad_struct_sizes(size_t* out, int cap);

/* ---- attention maps: where a vision block's attention goes -------------------------------------------------------------------
 *
 * The probabilities softmax(Q K^T) of Attention.forward (VitaCLIP_vision_encoder_utils.py:71-77), which gava_attention never
 * writes, summed over the queries with a weight.  Operands are addressed as by gava_attention: problem (f, h) = frame f,
 * head h (columns [64h, 64h + 64)); q is h16 and already carries the 1/sqrt(64) factor, queries are rows f*q_batch_rows +
 * [0, n_q) of q with row stride ld_q (defaults, when 0: q_batch_rows = n_q, ld_q = ld_qkv); the keys are the n_kmain rows
 * f*n_kmain + [0, n_kmain) of k followed by the side rows [n_g global | T local of the frame's clip | summary] of side_k, in
 * gava_attention's layout (n_g + batch + batch rows; n_g = T = has_summary = 0: no side rows).  With
 *   P[i][j] = softmax_j(q_i . k_j) over all n_keys = n_kmain + n_side keys,
 *   renorm = 0:  out[f][h][j] = sum_i w[f][i] * P[i][j]                                   j in [0, n_keys)
 *   renorm = 1:  out[f][h][j] = sum_i w[f][i] * P[i][j] / sum_{j' < n_kmain} P[i][j']     j in [0, n_kmain)
 * (renorm = 1 is the softmax over the frame's own keys alone, and is computed as that: the side rows are then not read.)
 * w: fp32 [batch][n_q], NULL = every weight 1 (the same bits as an array of ones).  out: fp32 [batch][heads][n_out],
 * n_out = n_keys or n_kmain.  n_q = 1 with w = NULL is the CLS row of a block (the only form a kept last block allows: its
 * queries are gava_vision_saved.last_q, its keys columns D..2D of its qkv slot); n_q = n_kmain with renorm = 1 is one step of
 * the attention-rollout chain r <- r/2 + mean_h(out)/2.
 * Scores are MFMA products accumulated in fp32, the softmax is fp32 in exp2 form, nothing is rounded to 16 bits.  Every
 * output element is summed by one wave in a fixed order (queries ascending per lane, then a fixed butterfly over sixteen
 * lanes): no atomics, two runs give the same bits.  One launch on `stream`.
 * Limits: K of one (frame, head) is resident in LDS, so n_keys <= 640 in either form (594 keys = 384 px at P = 16 with T = 8, G = 8);
 * n_q <= n_kmain.  GAVA_EINVAL, before any launch: beyond those limits, null args / q / k / out, batch, heads, n_q or
 * n_kmain < 1, ld_qkv / ld_side / ld_q not a multiple of 8 or below heads*64, q / k / side_k not 16-byte aligned, w / out not
 * 4-byte aligned, side rows asked for without side_k or with batch % T != 0, q_batch_rows < n_q, renorm outside {0, 1}, an
 * unknown prec. */
typedef struct {
  const void* q; const void* k; int64_t ld_qkv;     /* h16, element strides */
  const void* side_k; int64_t ld_side;
  const float* w;                                   /* fp32 [batch][n_q] or NULL */
  float* out;                                       /* fp32 [batch][heads][renorm ? n_kmain : n_kmain + n_side] */
  int batch, heads, n_q, n_kmain;
  int n_g, T, has_summary;
  int renorm, prec;
  int q_batch_rows; int64_t ld_q;
} gava_attention_mass_args;
int gava_attention_mass(const gava_attention_mass_args* a, gava_stream_t stream);

/* sizeof of gava_attention_mass_args, like gava_input_grad_struct_sizes.  Writes min(cap, 1) entries, returns 1. */
int gava_attention_maps_struct_sizes(size_t* out, int cap);

/* ---- relevance maps: one step of gradient-weighted attention relevance ------------------------------------------------------
 *
 * The class-specific counterpart of the rollout step above (Chefer et al., "Generic Attention-model Explainability", the
 * self-attention rule): the block's probabilities times their gradient, clamped at zero, summed over the queries with a weight.
 * Neither the probabilities nor their gradients exist in memory; both are formed here from what the forward kept and from the
 * backward's gradient of the attention output.  Operands are addressed as by gava_attention_mass and gava_attention_backward:
 * problem (f, h) = frame f, head h (columns [64h, 64h + 64)); q is h16 and already carries the 1/sqrt(64) factor; queries are
 * rows f*q_batch_rows + [0, n_q) of q (row stride ld_q) and of dout (row stride ld_dout) - defaults, when 0: q_batch_rows = n_q,
 * ld_q = ld_qkv; keys and values are the n_kmain rows f*n_kmain + [0, n_kmain) of k / v; the side rows [n_g global | T local of
 * the frame's clip | summary] of side_k, in gava_attention's layout, are further KEYS of the softmax (n_g = T = has_summary =
 * 0: none) - their values are not needed, because only the frame's own columns are written.  dout is the gradient of the
 * scalar being explained with respect to the attention output (the input of out_proj), h16 of `prec`.  With
 *   P[i][j] = softmax_j(q_i . k_j) over all n_kmain + n_side keys           (no renormalisation: what the forward used)
 *   G[i][j] = sum_c dout[i][64h + c] * v[j][64h + c]                        (= d s / d P_h[i][j])
 *   out[f][h][j] = sum_{i < n_q} w[f][i] * max(0, P[i][j] * G[i][j])        j in [0, n_kmain)
 * w: fp32 [batch][n_q], NULL = every weight 1 (the same bits as an array of ones); the clamp is applied before the weight.
 * out: fp32 [batch][heads][n_kmain].  n_q = 1 with w = NULL is the step of a block whose CLS row alone carries a gradient
 * (the last one; on a kept last block q and dout are [batch][D] buffers of their own: q_batch_rows = 1); n_q = n_kmain with
 * w = r is the chain step r <- r + mean_h(out) of every other block.
 * prec is dout's type; act_prec_set / act_prec have gava_attention_backward's meaning: q / k / v / side_k are stored as
 * act_prec (fp16 activations kept from the forward) while dout is prec (bf16); 0 = same as prec.  The scores are products of
 * the STORED q and k (the forward's probabilities); v is converted to prec as it is loaded, as the backward does, and G is a
 * product in prec.  MFMA products accumulated in fp32, fp32 softmax in exp2 form, nothing is rounded to 16 bits after the
 * MFMAs.  Every output element is summed by one wave in a fixed order (queries ascending per lane, then a fixed butterfly over
 * sixteen lanes): no atomics, two runs give the same bits.  One launch on `stream`.
 * Limits: K of one (frame, head) is resident in LDS, so n_kmain + n_side <= 640; n_q <= n_kmain.  GAVA_EINVAL, before any
 * launch: beyond those limits, null args / q / k / v / dout / out, batch, heads, n_q or n_kmain < 1, ld_qkv / ld_side /
 * ld_dout / ld_q not a multiple of 8 or below heads*64, q / k / v / dout / side_k not 16-byte aligned, w / out not 4-byte
 * aligned, side rows asked for without side_k or with batch % T != 0, q_batch_rows < n_q, an unknown prec or act_prec or a
 * pair other than (f16, f16), (bf16, bf16), (prec bf16, act_prec f16). */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;     /* h16 of act_prec, element strides */
  const void* side_k; int64_t ld_side;
  const void* dout; int64_t ld_dout;                               /* h16 of prec */
  const float* w;                                                  /* fp32 [batch][n_q] or NULL */
  float* out;                                                      /* fp32 [batch][heads][n_kmain] */
  int batch, heads, n_q, n_kmain;
  int n_g, T, has_summary;
  int prec, act_prec_set, act_prec;
  int q_batch_rows, reserved; int64_t ld_q;
} gava_attention_relevance_args;
int gava_attention_relevance(const gava_attention_relevance_args* a, gava_stream_t stream);

/* sizeof of gava_attention_relevance_args, like gava_attention_maps_struct_sizes.  Writes min(cap, 1) entries, returns 1. */
int gava_attention_relevance_struct_sizes(size_t* out, int cap);

/* ---- faithfulness curves: deletion / insertion by patch or frame -------------------------------------------------------------
 *
 * The perturbation test of an importance map (Petsiuk et al., RISE; Chefer et al. for relevance): rank a clip's patches or
 * frames by a score map (gava_patch_ranks), build for each of S1 thresholds the clip with its k_s most important units
 * replaced by a baseline - or with only those kept - (gava_perturb_clips; the baseline may be the blurred clip,
 * gava_blur_clips), run the plain forward on the nb * S1 clips, and reduce the logits to the curves and the areas under them
 * (gava_perturb_scores).  None of the four uses an atomic: a call repeats bit for bit.  One launch each on `stream`, except
 * gava_blur_clips (two: rows, then columns) and gava_patch_ranks on pixel scores (two: pool, then rank).
 *
 * gava_patch_ranks.  scores fp32, by layout:
 *   GAVA_RANK_PATCH  [B][T][g][g]                the unit is a patch
 *   GAVA_RANK_PIXEL  [B][T][g*patch][g*patch]    a patch's score is the fp32 sum of its patch x patch pixels, formed by a launch of
 *                                                its own into `pooled`: a wave per patch, lane l adds pixels l, l + 64, ... of the
 *                                                patch (row-major) in that order, then a fixed xor butterfly over the lanes
 *   GAVA_RANK_FRAME  [B][T]                      the unit is a frame (g, patch ignored)
 * scope GAVA_SCOPE_CLIP: one ranking per clip over its n = T*g*g patches (n = T frames); GAVA_SCOPE_FRAME: one ranking per
 * frame over its n = g*g patches (patch units only).  ranks int32, [B][T*g*g] (or [B][T]) in the scores' own unit order.
 * Unit j comes BEFORE unit i when s_j > s_i, or s_j == s_i (so -0 == +0) and j < i; every NaN comes after -inf, NaNs among
 * themselves by index.  rank_i = #{j : j before i}: 0 is the most important unit, the ranks of a ranking are a permutation
 * of 0 .. n-1.  Counted, not sorted: a workgroup owns 256 units of one ranking and streams all n scores of it through LDS.
 * GAVA_EINVAL: null args / scores / ranks, B, T, g < 1, patch < 1 or no `pooled` in the pixel layout, an unknown layout or scope, the frame
 * scope with the frame layout, n > GAVA_PERTURB_MAX_UNITS, more than 2^31 - 1 units or rankings in all.
 *
 * gava_blur_clips.  Separable Gaussian blur of every one of the B*3*T planes of x fp32 [B][3][T][size][size] -> out, the same
 * shape; taps: DEVICE fp32 [2*radius + 1], applied along x then along y with the border replicated (indices clamped), each
 * output a chain of fused multiply-adds over the taps in ascending order.  tmp: fp32 workspace of x's size (the row pass's
 * output); x, tmp and out are three different buffers.  GAVA_EINVAL: a null pointer, B, T or size < 1, radius outside
 * [0, GAVA_BLUR_MAX_RADIUS].
 *
 * gava_perturb_clips.  x fp32 [nb][3][T][size][size]; ranks as gava_patch_ranks writes them, [nb][T*g*g] (units
 * GAVA_UNITS_PATCH, g = size/patch) or [nb][T] (GAVA_UNITS_FRAME); k[0 .. n_steps): the thresholds, by value, non-decreasing.
 * out fp32 [nb][n_steps][3][T][size][size]:
 *   GAVA_PERTURB_DELETION   out[b][s] = rank(unit of the pixel) < k[s] ? baseline : x
 *   GAVA_PERTURB_INSERTION  out[b][s] = rank(unit of the pixel) < k[s] ? x : baseline
 * a selection: every output word is x's or the baseline's, bit for bit.  baseline: GAVA_BASELINE_ZERO (+0.0f), _CHANNEL
 * (baseline = DEVICE fp32 [3], one value per channel) or _TENSOR (baseline fp32 shaped like x).  x is read once and written
 * n_steps times, 16 bytes per lane when patch is a multiple of 4, 8 when it is even (P = 14), single floats otherwise.
 * Offsets are 64-bit: out may hold more than 2^31 elements.  GAVA_EINVAL: null args / x / ranks / out, a baseline pointer that
 * does not go with the kind, nb, T, size, patch < 1 or size % patch != 0, n_steps outside [1, GAVA_PERTURB_MAX_STEPS], a
 * negative or decreasing k, an unknown mode / units / kind, x / out / a tensor baseline not 16-byte aligned.
 *
 * gava_perturb_scores.  logits fp32, nb * n_steps rows of C (row b * n_steps + s, rows ld floats apart); target: DEVICE int64
 * [nb] or NULL - then clip b's target is the top-1 class of its row ref_step (the unperturbed step), found here; fractions:
 * the curves' abscissae, by value.  Per clip and step: logit = the target's raw logit (a copy), prob = its softmax
 * probability (fp32: exp(x_t - max) / sum_c exp(x_c - max), lanes stride the classes, a xor butterfly), top1 = the row's
 * largest logit, the lowest class on ties (0 for a row of NaNs).  Per clip: auc = sum_s (f_s - f_{s-1}) * (y_s + y_{s-1}) / 2
 * for y = logit and y = prob, added in step order in fp32 (0 for n_steps = 1), and target_out = the target used.  A target
 * outside [0, C) is not read through: that clip's logit, prob and both areas are NaN, top1 and target_out are written as
 * usual.  One workgroup per clip.  GAVA_EINVAL: null args or a null logits / logit / prob / top1 / auc / target_out pointer,
 * nb or C < 1, ld < C, n_steps outside [1, GAVA_PERTURB_MAX_STEPS], ref_step outside [0, n_steps). */
#define GAVA_PERTURB_MAX_UNITS 65536
#define GAVA_PERTURB_MAX_STEPS 128
#define GAVA_BLUR_MAX_RADIUS 64
#define GAVA_RANK_PATCH 0
#define GAVA_RANK_PIXEL 1
#define GAVA_RANK_FRAME 2
#define GAVA_SCOPE_CLIP 0
#define GAVA_SCOPE_FRAME 1
#define GAVA_UNITS_PATCH 0
#define GAVA_UNITS_FRAME 1
#define GAVA_PERTURB_DELETION 0
#define GAVA_PERTURB_INSERTION 1
#define GAVA_BASELINE_ZERO 0
#define GAVA_BASELINE_CHANNEL 1
#define GAVA_BASELINE_TENSOR 2
typedef struct {
  const float* scores; int32_t* ranks;
  float* pooled;                               /* GAVA_RANK_PIXEL: fp32 workspace [B][T][g][g]; ignored otherwise */
  int B, T, g, patch, layout, scope;
} gava_patch_ranks_args;
int gava_patch_ranks(const gava_patch_ranks_args* a, gava_stream_t stream);

typedef struct {
  const float* x; const float* taps; float* tmp; float* out;
  int B, T, size, radius;
} gava_blur_clips_args;
int gava_blur_clips(const gava_blur_clips_args* a, gava_stream_t stream);

typedef struct {
  const float* x; const int32_t* ranks; const float* baseline; float* out;
  int nb, T, size, patch, units, mode, baseline_kind, n_steps;
  int k[GAVA_PERTURB_MAX_STEPS];
} gava_perturb_clips_args;
int gava_perturb_clips(const gava_perturb_clips_args* a, gava_stream_t stream);

typedef struct {
  const float* logits; int64_t ld;
  const int64_t* target;                       /* DEVICE [nb] or NULL */
  float* logit; float* prob; int32_t* top1;    /* [nb][n_steps] */
  float* auc_logit; float* auc_prob;           /* [nb] */
  int64_t* target_out;                         /* [nb] */
  int nb, n_steps, C, ref_step;
  float fractions[GAVA_PERTURB_MAX_STEPS];
} gava_perturb_scores_args;
int gava_perturb_scores(const gava_perturb_scores_args* a, gava_stream_t stream);

/* sizeof of gava_patch_ranks_args, gava_blur_clips_args, gava_perturb_clips_args, gava_perturb_scores_args, in that order,
 * like gava_attention_relevance_struct_sizes.  Writes min(cap, 4) entries, returns 4. */
int gava_perturbation_struct_sizes(size_t* out, int cap);

/* ---- path gradients: integrated gradients and SmoothGrad, accumulated in the fold -------------------------------------------
 *
 * Both repairs of the plain pixel gradient are m gradients of near-copies of a clip reduced to one map: integrated gradients
 * (Sundararajan et al.) (x - x0) * sum_k w_k df/dx(x0 + alpha_k (x - x0)) along the straight path from a baseline x0, SmoothGrad
 * (Smilkov et al.) the mean gradient over m noisy copies.  gava_path_clips writes the m copies of every clip, the forward and
 * the backward run on the nb * m clips as on any batch, gava_unpatchify_path folds the patch gradients of a clip's m copies
 * into ONE map - the m full-size gradients are never in memory -, gava_path_delta is the completeness residual
 * sum(attributions) - (f(x) - f(x0)), and gava_clip_range gives the noise its scale.  None of the four uses an atomic: a call
 * repeats bit for bit.  Offsets are 64-bit.  One launch each on `stream`, except gava_clip_range (two).  The vector width is
 * gava_unpatchify's and gava_perturb_clips': 16 bytes per lane when patch is a multiple of 4 (the fold: and ld too), 8 when
 * they are even (P = 14), single floats otherwise.
 *
 * gava_path_clips.  x fp32 [nb][3][T][size][size] -> out fp32 [nb][m][3][T][size][size]; x (and a tensor baseline) is read
 * once and written m times.
 *   GAVA_PATH_LINE   out[b][k] = fma(alpha[k], x, beta[k] * x0): one rounded product, one fused multiply-add.  alpha, beta:
 *                    fp32 by value, beta = 1 - alpha formed by the caller (in double, then rounded); alpha = 0, beta = 1 gives
 *                    x0 and alpha = 1, beta = 0 gives x, value for value.  x0: GAVA_BASELINE_ZERO (+0.0f), _CHANNEL (baseline =
 *                    DEVICE fp32 [3]) or _TENSOR (baseline fp32 shaped like x).  sigma must be NULL.
 *   GAVA_PATH_NOISE  out[b][k] = fma(sigma[b], z, x), sigma DEVICE fp32 [nb], z a standard normal that depends on (seed,
 *                    clip0 + b, k, the element's index within the clip) and on nothing else - not on nb, not on how the clips
 *                    are cut into calls, not on the launch.  Philox4x32-10 with key (seed's low word, seed's high word) and
 *                    counter (e4's low word, e4's high word, k, clip0 + b), e4 = the index of a group of four consecutive
 *                    floats of the clip; its output words r0..r3 give the group's four normals by two Box-Muller pairs:
 *                    u1 = ((r0 >> 8) + 1) * 2^-24, u2 = (r1 >> 8) * 2^-24, z0 = sqrtf(-2 logf(u1)) * cosf(2 pi u2), z1 the
 *                    same with sinf; r2, r3 give z2, z3 the same way.  clip0: the global index of this call's first clip.
 *                    size must be even (3*T*size*size is then a multiple of 4); baseline NULL, kind GAVA_BASELINE_ZERO.
 * GAVA_EINVAL: null args / x / out, a baseline pointer that does not go with the kind (or any in noise mode), nb, T, size,
 * patch < 1 or size % patch != 0, m outside [1, GAVA_PATH_MAX_STEPS], an unknown mode or kind, x / out / a tensor baseline
 * not 16-byte aligned, line mode: sigma given, an alpha or beta outside [0, 1] or not finite; noise mode: sigma missing, an
 * odd size, clip0 < 0 or clip0 + nb past 2^31 - 1.
 *
 * gava_clip_range.  x fp32 [nb][3][T][size][size] -> min[b], max[b] over the whole clip and sigma[b] = fl(rel * fl(max - min)),
 * DEVICE fp32 [nb] each.  Two launches: GAVA_CLIP_RANGE_PARTS workgroups per clip leave their partial results in workspace
 * (fp32, nb * GAVA_CLIP_RANGE_PARTS * 2 floats), one workgroup per clip finishes.  Exact (min and max do not depend on the
 * order).  A NaN propagates: a clip that holds one gets min = max = sigma = NaN, and so do its noisy copies and their map.
 * GAVA_EINVAL: a null pointer, nb, T or size < 1, nb > 65535, a pointer that is not 4-byte aligned.
 *
 * gava_unpatchify_path.  gava_unpatchify's geometry and argument checks (dpatch, ld, frame_rows, row_offset, size, patch as
 * there), with one difference: out has B clips while dpatch holds the frames of B*m - clip b's copies are batch indices
 * b*m + k, k in [0, m) - and they are reduced while folding.  With g_c(j) gava_unpatchify's g of batch index j,
 *   G_c = sum_k w[k] * g_c(b*m + k)
 * as the chain G <- fma(w[k], g, G) over k = 0 ... m-1 from +0.0f; steps with w[k] == 0 are skipped (their rows are not read).
 * w: fp32 by value.
 *   GAVA_PATH_GRAD      out fp32 [B][3][T][size][size] = G
 *   GAVA_PATH_ABSMAX    out fp32 [B][T][size][size]    = max over c of |G_c|
 *   GAVA_PATH_L2        out                            = sqrt(G_0^2 + G_1^2 + G_2^2), as GAVA_UNPATCH_L2 forms it
 *   GAVA_PATH_ATTR      out fp32 [B][3][T][size][size] = a_c = fl(fl(x_c - x0_c) * G_c)
 *   GAVA_PATH_ATTR_SUM  out fp32 [B][T][size][size]    = (a_0 + a_1) + a_2
 *   GAVA_PATH_ATTR_ABS  out                            = (|a_0| + |a_1|) + |a_2|
 * x: the fp32 clips [B][3][T][size][size]; x0 by baseline_kind as for gava_path_clips.  Both belong to the three ATTR modes
 * and are refused in the others (baseline NULL, kind GAVA_BASELINE_ZERO there).  With m = 1 and w = {1} the first three modes
 * give gava_unpatchify's values.  One workgroup owns P image rows of a frame of the OUTPUT: it reads m times 12 B per pixel
 * and writes 4 or 12.  GAVA_EINVAL: gava_unpatchify's list (B*T*m in place of B*T), m outside [1, GAVA_PATH_MAX_STEPS], a
 * weight that is not finite, an unknown mode or kind, x missing in an ATTR mode, x or a baseline given in another, a baseline
 * pointer that does not go with the kind, x / a tensor baseline not 16-byte aligned.
 *
 * gava_path_delta.  map: the signed attribution map fp32 [B][T][size][size] (GAVA_PATH_ATTR_SUM); logits fp32, B*m rows of C
 * (row b*m + k, rows ld floats apart); target DEVICE int64 [B].  Per clip, DEVICE fp32 [B] each:
 *   sum_attr = the sum of the clip's map, f_diff = fl(logits[b*m + k_hi][target] - logits[b*m + k_lo][target]),
 *   delta = fl(sum_attr - f_diff)
 * (k_lo: the step that is x0, k_hi: the step that is x).  One workgroup of 256 threads per clip; the sum runs in double in a
 * fixed order - thread i adds elements i, i + 256, ... in that order, a fixed xor butterfly over the lanes of a wave, then the
 * four waves in order - and is rounded to fp32 once.  A target outside [0, C) is not read through: that clip's three outputs
 * are NaN.  GAVA_EINVAL: a null pointer, B, T, size or C < 1, ld < C, m outside [1, GAVA_PATH_MAX_STEPS], k_lo or k_hi
 * outside [0, m), a misaligned pointer. */
#define GAVA_PATH_MAX_STEPS 64
#define GAVA_CLIP_RANGE_PARTS 64
#define GAVA_PATH_LINE 0
#define GAVA_PATH_NOISE 1
#define GAVA_PATH_GRAD 0
#define GAVA_PATH_ABSMAX 1
#define GAVA_PATH_L2 2
#define GAVA_PATH_ATTR 3
#define GAVA_PATH_ATTR_SUM 4
#define GAVA_PATH_ATTR_ABS 5
typedef struct {
  const float* x; const float* baseline; const float* sigma; float* out;
  int nb, T, size, patch, mode, baseline_kind, m, clip0;
  uint64_t seed;
  float alpha[GAVA_PATH_MAX_STEPS]; float beta[GAVA_PATH_MAX_STEPS];
} gava_path_clips_args;
int gava_path_clips(const gava_path_clips_args* a, gava_stream_t stream);

typedef struct {
  const float* x; float* min; float* max; float* sigma;
  float* workspace;                            /* fp32 [nb][GAVA_CLIP_RANGE_PARTS][2] */
  int nb, T, size; float rel;
} gava_clip_range_args;
int gava_clip_range(const gava_clip_range_args* a, gava_stream_t stream);

typedef struct {
  const float* dpatch; int64_t ld;
  const float* x; const float* baseline;       /* the ATTR modes only, NULL otherwise */
  float* out;
  int B, T, size, patch, mode, baseline_kind, frame_rows, row_offset, m, reserved;
  float w[GAVA_PATH_MAX_STEPS];
} gava_unpatchify_path_args;
int gava_unpatchify_path(const gava_unpatchify_path_args* a, gava_stream_t stream);

typedef struct {
  const float* map; const float* logits; int64_t ld;
  const int64_t* target;                       /* DEVICE [B] */
  float* sum_attr; float* f_diff; float* delta;        /* [B] */
  int B, T, size, m, C, k_lo, k_hi, reserved;
} gava_path_delta_args;
int gava_path_delta(const gava_path_delta_args* a, gava_stream_t stream);

/* sizeof of gava_path_clips_args, gava_clip_range_args, gava_unpatchify_path_args, gava_path_delta_args, in that order, like
 * gava_perturbation_struct_sizes.  Writes min(cap, 4) entries, returns 4. */
int gava_path_grad_struct_sizes(size_t* out, int cap);

/* ---- Mixup / CutMix on the device and the criterion for soft targets (opt-in: gava_clip_amd.ClipMixer, SoftTargetCriterion) --
 *
 * The reference's loss code takes targets of the logits' shape (training/loss_utils.py:32-44 and CrossEntropyLoss with class
 * probabilities); its loop keeps the branch for them (training/train.py:477) but ships no mixing code.  This section is the
 * mix of the clips, the targets that go with it, and that criterion.  gava_train_criterion and the sigmoid criterion keep
 * taking integer labels only.  fp32 throughout, no floating-point atomics: the same bits on every run.
 *
 * gava_mix_clips: x, out fp32 [B][planes][H][W], contiguous (planes = 3 T for a [B, 3, T, S, S] batch), one descriptor per
 * clip.  For clip i with partner j = desc[i].partner, own pixel a and the partner's pixel b at the same position:
 *   j == i                         out = a: a copy, bit for bit (nothing is computed)
 *   y1 > y0 && x1 > x0  (CutMix)   out = b where y0 <= h < y1 and x0 <= w < x1 (a tube through all planes), a elsewhere: a
 *                                  selection, bit for bit; lam is not read
 *   otherwise           (Mixup)    out = fma(lam, a, fl(fl(1 - lam) * b)); lam == 1 copies a and lam == 0 copies b, whatever
 *                                  the values
 * out != x: any partner; x and out must not overlap.  out == x (in place): partner must be an involution
 * (partner[partner[i]] == i); one thread owns a position of both clips of a pair, reads both originals and writes both
 * results, each by its clip's own descriptor, so the members of a pair may differ in lam, box and kind - with the bits of
 * the out-of-place call.  Positions that no descriptor changes are not written in place.  Rows are walked with 16-byte
 * accesses when W % 4 == 0 and both bases are 16-byte aligned (box edges off a multiple of 4 select per element inside the
 * vector), element by element otherwise; no address outside the tensors is formed.  The grid's y extent is the clip, split
 * into launches of 65535 clips; within a clip a grid-stride loop.
 * The arguments carry the descriptor table twice: desc_host is read by the entry point, desc (the same B entries in device
 * memory) by the kernel.  GAVA_EINVAL, before any launch: a null pointer; B, planes, H or W < 1; planes * H * W >= 2^31; a
 * partner outside [0, B); a box outside [0, H] x [0, W] or inverted (y1 < y0 or x1 < x0); lam outside [0, 1] or NaN;
 * out == x with a partner table that is no involution; x and out overlapping without being equal.
 *
 * gava_mix_targets: targets [B][C] fp32 (rows ld_targets apart) from int64 labels (DEVICE, clamped to [0, C) like
 * gava_train_criterion's), the same device descriptor table and a label smoothing eps in [0, 1]:
 *   s(y)[c] = (1 - eps) [c == y] + eps / C;   targets[i] = lam_i s(y_i) + (1 - lam_i) s(y_partner(i))
 * formed in fp64 and rounded once; exact for eps == 0 and lam in {0, 1}; a clip that is its own partner gets s(y_i) whatever
 * its lam.  One launch.  The descriptors are not validated
 * here (they are device memory); a partner outside [0, B) is clamped.
 *
 * gava_soft_criterion / gava_soft_criterion_backward: per sample i with logits z, targets t >= 0 of the same shape and
 * tau = sum_c t_c (need not be 1):
 *   p = softmax(z);  lse = logsumexp(z);  ce = sum_c t_c (lse - z_c)                 (every term >= 0)
 *   k = argmax_c z_c,  y* = argmax_c t_c                                             (the lowest index on ties, as torch.argmax)
 *   w = scale * (fl32(beta * fl32(|y* - k| / (C - 1))) * tau + alpha * sum_c t_c (1 - p_c)^gamma)
 *   l = weighted ? ce * w : ce;   loss = mean_i l_i;   hits = #{i : k_i == y*_i};   conf[y*][k] += 1 (optional, ACCUMULATED)
 *   Q = sum_c t_c (1 - p_c)^(gamma - 1) p_c
 *   dlogits[i][c] = (w (tau p_c - t_c) + ce scale alpha gamma p_c (Q - t_c (1 - p_c)^(gamma - 1))) * grad_loss / B
 * (unweighted: (tau p_c - t_c) * grad_loss / B; the ordinal term has no gradient, as in the reference).  With one-hot targets
 * this is gava_train_criterion's formula.  One wave per sample: logsumexp = m + log1p(s1) with m the row maximum and s1 the
 * sum of exp(z_c - m) over the other classes; 1 - p_c = s1 / (1 + s1) for the top class, ((1 + s1) - e_c) / (1 + s1)
 * otherwise.  Classes with t_c == 0 add nothing: an all-zero target row has loss and gradient exactly 0.  The forward leaves
 * eight floats per sample in `saved` (m, log1p(s1), s1, the bits of k; w, ce scale alpha gamma, Q, tau); the backward reads
 * them, the logits, the targets, `weighted` and `gamma` from the same struct, and the upstream gradient FROM DEVICE MEMORY
 * (grad_loss, one float).  No gradient is formed for the targets.
 * GAVA_EINVAL: weighted with gamma < 1 or C < 2, B < 1, C < 1, a row stride below C, a null pointer among the required ones
 * (forward: logits, targets, loss, per_sample, weight, top1, target1, hits, saved; backward: logits, targets, saved,
 * grad_loss, dlogits).  Two launches forward, one backward, no host synchronisation. */
typedef struct { int32_t partner; float lam; int32_t y0, y1, x0, x1; } gava_mix_desc;

typedef struct {
  const float* x; float* out;                 /* fp32 [B][planes][H][W]; out == x mixes in place */
  const gava_mix_desc* desc_host;             /* [B], host memory: validated by the entry point */
  const gava_mix_desc* desc;                  /* [B], the same table in device memory: read by the kernel */
  int B, planes, H, W;
} gava_mix_clips_args;
int gava_mix_clips(const gava_mix_clips_args* a, gava_stream_t stream);

typedef struct {
  const int64_t* labels;                      /* DEVICE [B] */
  const gava_mix_desc* desc;                  /* DEVICE [B] */
  float* targets; int64_t ld_targets;         /* fp32 [B][C] */
  int B, C; float smoothing; int reserved;
} gava_mix_targets_args;
int gava_mix_targets(const gava_mix_targets_args* a, gava_stream_t stream);

typedef struct {
  const float* logits; int64_t ld_logits;     /* fp32 [B][C], rows ld_logits elements apart */
  const float* targets; int64_t ld_targets;   /* fp32 [B][C], rows ld_targets elements apart */
  int B, C, weighted;
  float alpha, gamma, beta, scale;
  float* loss; float* per_sample; float* weight; int32_t* top1; int32_t* target1; int32_t* hits;
  int32_t* conf;                              /* optional */
  float* saved;                               /* [B][8] */
  const float* grad_loss; float* dlogits; int64_t ld_dlogits;     /* backward only */
} gava_soft_criterion_args;
int gava_soft_criterion(const gava_soft_criterion_args* a, gava_stream_t stream);
int gava_soft_criterion_backward(const gava_soft_criterion_args* a, gava_stream_t stream);

/* sizeof of gava_mix_desc, gava_mix_clips_args, gava_mix_targets_args, gava_soft_criterion_args, in that order, like
 * gava_path_grad_struct_sizes.  Writes min(cap, 4) entries, returns 4. */
int gava_mix_struct_sizes(size_t* out, int cap);

/* ---- RandAugment on the device (opt-in: gava_clip_amd.RandAugment, AugmentedClipPreprocessor) ------------------------------------
 *
 * The reference's auto_augment step (video_dataset/dataset.py:98-108, rand_augment.py) runs its ops through Pillow on the host,
 * between the frame draw and random_resized_crop.  This section is that step on packed uint8 RGB frames [H][W][3] (rows of 3 W
 * bytes, no alignment asked), with Pillow's results byte for byte.  One call handles one LAYER of the policy: a table of n
 * descriptors, one per frame, of any mix of sizes and ops; the host draws the policy and builds the tables.  Each entry point
 * is one launch whatever n is (none where no frame of the layer needs it), nothing waits for the device, integer atomics only.
 *
 * kind GAVA_AUG_TABLE: dst[p][c] = lut[c][src[p][c]], the 3 x 256 table built by gava_augment_luts in slot lut_slot from op:
 *   INVERT        255 - i                      POSTERIZE   i & ~(2^(8 - iarg) - 1)   (iarg >= 8: i)
 *   SOLARIZE      i < iarg ? i : 255 - i       SOLARIZE_ADD  i < 128 ? min(255, i + iarg) : i
 *   BRIGHTNESS    blend(0, i, factor)
 *   CONTRAST      blend(mean, i, factor), mean = int(sum_i i hL[i] / sum_i hL[i] + 0.5) in fp64 from the histogram hL of
 *                 L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *   AUTOCONTRAST  per channel, lo / hi the first / last non-empty bin: i if hi <= lo, else with scale = 255.0 / (hi - lo) in
 *                 fp64 clamp(int(i * scale + (-lo * scale)), 0, 255), int truncating toward zero
 *   EQUALIZE      per channel, in integers: with the non-empty bins nz, step = (sum nz - nz[last]) / 255; i if there is at most
 *                 one non-empty bin or step == 0, else min(255, (step / 2 + sum_{j < i} h[j]) / step)
 *   The last three read the frame's histograms - uint32 [4][256] for R, G, B, L in slot hist_slot - which gava_augment_hist
 *   counts from src (CONTRAST: L only; the other two: R, G, B only).  The histogram buffer must be zero before the first layer;
 *   gava_augment_luts zeroes every slot it reads, so the buffer is ready for the next layer.
 * kind GAVA_AUG_COLOR: dst = blend(L, v, factor) per channel.
 * kind GAVA_AUG_SHARPNESS: dst = blend(smooth(v), v, factor); smooth is Pillow's SMOOTH filter: fp32, from 0.5, adding
 *   pixel * fl32(k / 13) row-major with k = 1 1 1 / 1 5 1 / 1 1 1, clipped to [0, 255] and truncated; the one-pixel border is
 *   copied.
 * kind GAVA_AUG_AFFINE: Image.transform(AFFINE, m, filter, fill 128) in fp64: xin = m0 (xo + .5) + m1 (yo + .5) + m2, yin
 *   likewise from m3..m5; outside [0, W) x [0, H) the pixel is 128; else xin -= .5, x = floor(xin), dx = xin - x (and y), and
 *   BILINEAR  v = a + (b - a) d along x on rows clip(y), clip(y + 1), then along y; truncated
 *   BICUBIC   rows clip(y - 1 .. y + 2), columns clip(x - 1 .. x + 2); p1 = v2, p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4,
 *             p4 = -v1 + v2 - v3 + v4, v = p1 + d (p2 + d (p3 + d p4)) along x, then along y; <= 0 -> 0, >= 255 -> 255, else
 *             truncated
 * blend(a, b, f) = a + fl32(f) (b - a) in fp32: truncated for 0 <= f <= 1, else clipped to [0, 255] and truncated.  No product
 * is fused into the add that follows it (Pillow's CPU builds do not contract).
 *
 * The arguments carry the table twice, like gava_mix_clips: desc_host is validated by every entry point, desc (the same n
 * entries in device memory) is read by the kernels.  GAVA_EINVAL, before any launch: a null table, n < 1, n_hist or n_luts < 0;
 * per descriptor a null src or dst, H or W < 1, a frame of 2^31 bytes or more, src == dst (or overlapping frames), an unknown
 * kind, op or filter, a non-finite factor or matrix entry, iarg outside [0, 256] for the ops that read it, a table op with
 * luts null or lut_slot outside [0, n_luts), a statistics op with hist null or hist_slot outside [0, n_hist).  Fields a kind
 * does not read are ignored apart from the finiteness of factor and m. */
enum { GAVA_AUG_TABLE = 0, GAVA_AUG_COLOR = 1, GAVA_AUG_SHARPNESS = 2, GAVA_AUG_AFFINE = 3 };                 /* kind */
enum { GAVA_AUG_INVERT = 0, GAVA_AUG_POSTERIZE = 1, GAVA_AUG_SOLARIZE = 2, GAVA_AUG_SOLARIZE_ADD = 3,         /* op of a table */
       GAVA_AUG_BRIGHTNESS = 4, GAVA_AUG_CONTRAST = 5, GAVA_AUG_AUTOCONTRAST = 6, GAVA_AUG_EQUALIZE = 7 };
enum { GAVA_AUG_BILINEAR = 0, GAVA_AUG_BICUBIC = 1 };                                                          /* filter */

typedef struct {
  const uint8_t* src; uint8_t* dst;           /* one frame each, uint8 [H][W][3] */
  int32_t H, W, kind, op;
  int32_t filter, iarg; float factor; int32_t lut_slot;
  int32_t hist_slot, reserved;
  double m[6];                                /* GAVA_AUG_AFFINE: output pixel centre -> source position */
} gava_augment_desc;

typedef struct {
  const gava_augment_desc* desc_host;         /* [n], host memory: validated by the entry points */
  const gava_augment_desc* desc;              /* [n], the same table in device memory: read by the kernels */
  uint32_t* hist;                             /* DEVICE [n_hist][4][256], zero on entry to the first layer */
  uint8_t* luts;                              /* DEVICE [n_luts][3][256] */
  int32_t n, n_hist, n_luts, reserved;
} gava_augment_args;
/* a layer is these three calls in this order on one stream; the first two launch nothing where the layer needs no statistics /
 * no table */
int gava_augment_hist(const gava_augment_args* a, gava_stream_t stream);
int gava_augment_luts(const gava_augment_args* a, gava_stream_t stream);
int gava_augment_apply(const gava_augment_args* a, gava_stream_t stream);

/* sizeof of gava_augment_desc, gava_augment_args, in that order, like gava_mix_struct_sizes.  Writes min(cap, 2) entries,
 * returns 2. */
int gava_augment_struct_sizes(size_t* out, int cap);

/* sizeof of every ABI struct as the library was compiled, in the order gemm_args, layernorm_args, attention_args,
 * attention_f32_args, clip_desc, vision_layer, vision_layer8, vision_model, text_layer, text_model, layernorm_bwd_args,
 * attention_bwd_args, vision_saved, preprocess_args, patchify_args, preprocess_clips_args, view_scores_args.  Writes
 * min(cap, 17) entries, returns 17.  A binding
 * compares them with its own mirrors at load time (gava_clip_amd/hip.py does): gava_abi_version ties the library to the
 * header, this ties the header to the mirrors. */
int gava_struct_sizes(size_t* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
