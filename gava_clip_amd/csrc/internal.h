// internal.h — launchers shared between translation units of libgava_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gava_hip.h"
namespace gava {
int side_ln(const float* gp, const float* lp, const float* cp, const float* summ, const float* gamma,
            const float* beta, void* out, int G, int T, int BT, int D, int prec, hipStream_t s);
int cls_embed(float* X, const float* cls, const float* pos, const float* time, int BT, int T, int D,
              long frame_stride, hipStream_t s);
int mean_rows(const float* in, float* out, int B, int T, int D, hipStream_t s);
int copy_rows(const float* in, long in_stride, float* out, int rows, int D, hipStream_t s);
// fp32 rows = hi + lo of the residual stream's 16-bit pair (rows in_stride elements apart)
int join_rows(const void* hi, const void* lo, long in_stride, float* out, long out_stride, int rows, int D, int prec, hipStream_t s);
// gemm.hip: does gava_gemm take an EPI_F32 GEMM of this shape with the residual as a 16-bit pair (gava_gemm_args.resid16)?
bool gemm_takes_pair(int M, int N, int K, long lda, long ldw);
// gemm.hip: does gava_gemm run an EPI_F32_PATCH GEMM with a patch matrix (A != NULL) of this shape on the persistent kernel?
bool gemm_patch_on_persistent(int M, int N, long lda, long ldw);
int text_embed(const float* emb, const float* pos, const float* ctx, const int* tok, float* X,
               int n_prompts, int L, int W, int n_ctx, hipStream_t s);
// rowops.hip: l2norm_rows, class_mean (by class_offsets), logits_mfma, text_feature - the launches of gava_similarity_head, keeping
// what gava_train_head_backward reuses (unit rows, 1 / |row|, the class means before their re-normalisation)
int train_head_forward(const float* video, const float* text, const int* offsets, const float* logit_scale, const float* logit_bias,
                       int B, int C, int P, int E, float* logits, float* text_features, float* video_norm, float* video_inv,
                       float* text_norm, float* text_inv, float* class_mean, hipStream_t s);
unsigned long long* debug_buffer();   // set by gava_debug_set_buffer; nullptr = stamps off
// attention.hip: GAVA_ATTN_STREAM=1 sends every non-causal shape to the streaming kernels (forward and backward; A/B and tests)
bool stream_forced();

// Where key row `row` of frame `frame` lives.  The n_keys keys of a frame are its own n_kmain rows of the main K/V matrix
// (row = frame * n_kmain + key), then rows of the gathered prompt ("side") matrix: its n_g global rows | the T local rows
// of the frame's clip | the frame's summary row (the side matrix holds n_g + batch + batch rows).  Rows past n_keys read
// key 0: their scores are masked, and what stands in for them must be finite.
struct KeyRowSrc { bool is_main; long row; };
__device__ __forceinline__ KeyRowSrc key_row_src(int frame, int row, int n_kmain, int n_keys, int n_g, int T, int batch) {
  const int rowc = row < n_keys ? row : 0;
  const int sidx = rowc - n_kmain;                                   // >= 0: side row
  const long sr = sidx < n_g ? sidx
                : sidx < n_g + T ? n_g + (long)(frame / T) * T + (sidx - n_g)
                                 : (long)n_g + batch + frame;
  const bool is_main = rowc < n_kmain;
  return {is_main, is_main ? (long)frame * n_kmain + rowc : sr};
}

// MFMA attention backward (attention_bwd.hip), launched by gava_attention_backward (backward.hip)
struct AttnBwdMfmaParams {
  const unsigned short* q; const unsigned short* k; const unsigned short* v; long ld_qkv;
  long ld_q, ld_dq; int q_rows;  // query-side layout: rows per frame in q / dout / dq and their strides
  const unsigned short* sk; const unsigned short* sv; long ld_side;
  const unsigned short* dout; long ld_dout;
  unsigned short* dq; unsigned short* dk; unsigned short* dv; long ld_dqkv;
  float* dsk; float* dsv; long ld_dside;
  float* stats;                 // [batch*heads][q_pad][2]: log2-sum-exp and delta per query
  int batch, heads, n_q, n_kmain, n_g, T, has_summary, n_keys, q_pad;
  float q_scale;
};
int attention_bwd_mfma(const AttnBwdMfmaParams& p, int prec, int act_prec, int causal, hipStream_t s);
}  // namespace gava
