// train_head.hip — the tail of a training step on the device: the criterion of the reference's training loop (per-sample
// cross-entropy times the ordinal-focal weight, mean) with its backward, and the backward of the similarity head.  The head's
// forward runs the inference head's kernels (rowops.hip, gava::train_head_forward).  Everything is fp32; reductions run in a
// fixed order (xor butterflies inside a wave, an LDS tree across waves), integer atomics only (the confusion matrix).
#include "common.h"
#include "internal.h"

namespace {

static __device__ __forceinline__ int clamp_label(long y, int C) { return (int)(y < 0 ? 0 : (y >= C ? C - 1 : y)); }

// ---- criterion ----------------------------------------------------------------------------------------------------------------
// One wave per sample, lanes stride the classes.  With m = max_c z_c at k (the lowest such class) and s1 = sum_{c != k} exp(z_c - m):
//   logsumexp = m + log1p(s1)   (the term of k is exactly 1: a sample the model is sure of keeps a cross-entropy of relative, not
//   absolute, accuracy);  1 - p_y = (sum_{c != y} exp(z_c - m)) / (1 + s1) - the sum itself when y == k, a difference only where
//   p_y <= 1/2.
struct CritParams {
  const float* logits; long ld;
  const long long* labels;
  int B, C, weighted;
  float alpha, gamma, beta, scale;
  float* per_sample; float* weight; int* top1; int* conf;
  float4* saved;
};

__global__ __launch_bounds__(256) void criterion_rows_kernel(const CritParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B) return;
  const float* z = p.logits + (long)row * p.ld;
  const int y = clamp_label(p.labels[row], p.C);
  float m = -INFINITY;
  int k = 0x7fffffff;
  for (int c = lane; c < p.C; c += 64) {
    const float v = z[c];
    if (v > m) { m = v; k = c; }                 // c ascends within a lane: strictly greater keeps the lowest class
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    if (om > m || (om == m && ok < k)) { m = om; k = ok; }
  }
  // NaN logits (nothing compared greater): class 0 and some finite-or-NaN stand-in for the maximum keep every index in range; the
  // row's outputs are then unspecified, as they are for a row holding +-inf (z - m is NaN there)
  if (k >= p.C) { k = 0; m = wave_max(z[lane < p.C ? lane : 0]); }
  float s1 = 0.f;
  for (int c = lane; c < p.C; c += 64)
    if (c != k) s1 += expf(z[c] - m);
  s1 = wave_sum(s1);
  const float l = log1pf(s1), sum = 1.0f + s1;
  const float zy = z[y];
  const float ce = (m - zy) + l;
  const float ey = y == k ? 1.0f : expf(zy - m);
  const float py = ey / sum;
  const float omp = y == k ? s1 / sum : (sum - ey) / sum;               // 1 - p_y
  float w = 1.0f, a = 1.0f, loss = ce;
  if (p.weighted) {
    const int d = y > k ? y - k : k - y;
    const float focal = p.alpha * powf(omp, p.gamma);
    w = p.scale * (p.beta * ((float)d / (float)(p.C - 1)) + focal);
    loss = ce * w;
    // d focal / d p_y = -alpha gamma (1 - p_y)^(gamma - 1); the chain through p_y = softmax is folded into (p_c - [c == y])
    a = w + ce * p.scale * p.alpha * p.gamma * powf(omp, p.gamma - 1.0f) * py;
  }
  if (lane == 0) {
    p.per_sample[row] = loss;
    p.weight[row] = w;
    p.top1[row] = k;
    p.saved[row] = make_float4(m, l, a, omp);
    if (p.conf) atomicAdd(p.conf + (long)y * p.C + k, 1);
  }
}

// loss = mean of per_sample, hits = #{top1 == label}: one workgroup; thread t adds samples t, t + 256, ... in order, then a tree
__global__ __launch_bounds__(256) void criterion_mean_kernel(const float* per_sample, const int* top1, const long long* labels,
                                                             int B, int C, float* loss, int* hits) {
  __shared__ float fs[256];
  __shared__ int hs[256];
  float s = 0.f;
  int h = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    s += per_sample[i];
    h += top1[i] == clamp_label(labels[i], C) ? 1 : 0;
  }
  fs[threadIdx.x] = s; hs[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { fs[threadIdx.x] += fs[threadIdx.x + o]; hs[threadIdx.x] += hs[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss[0] = fs[0] / (float)B; hits[0] = hs[0]; }
}

__global__ __launch_bounds__(256) void criterion_backward_kernel(const float* logits, long ld, const long long* labels,
                                                                 const float4* saved, const float* grad_loss, int B, int C,
                                                                 float* dlogits, long ldd) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float* z = logits + (long)row * ld;
  const int y = clamp_label(labels[row], C);
  const float4 st = saved[row];                       // (max, log of the sum of exp, a_i, 1 - p_y)
  const float g = grad_loss[0] / (float)B;
  for (int c = lane; c < C; c += 64) {
    const float pc = expf((z[c] - st.x) - st.y);
    dlogits[(long)row * ldd + c] = (st.z * (c == y ? -st.w : pc)) * g;
  }
}

// ---- head backward ------------------------------------------------------------------------------------------------------------
// Launch 1, one wave per workgroup, three roles by block index:
//   [0, nv)        16 x 16 tile of dvn [B][E] = s * dlogits [B][C] @ m [C][E]            (contraction over the C classes)
//   [nv, nv + nt)  16 x 16 tile of dm  [C][E] = s * dlogits^T [C][B] @ vn [B][E]         (contraction over the B clips)
//   nv + nt        dlogit_scale = sum dlogits * (logits - bias), dlogit_bias = sum dlogits   (compensated sums per lane)
// v_mfma_f32_16x16x4_f32 as in logits_mfma_kernel (an exact fp32 fma chain): lane l feeds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; D: column = l & 15, row = 4 * (l >> 4) + r.  Rows, columns and contraction steps past the matrix are
// zeros in the operand registers; their addresses are never formed.
struct HeadBwdParams {
  const float* dlogits; const float* logits; const float* logit_scale; const float* logit_bias;
  const float* vn; const float* cm;
  float* dvn; float* dm; float* dls; float* dlb;
  int B, C, E, nv, nt;
};

__global__ __launch_bounds__(64) void head_backward_gemm_kernel(const HeadBwdParams p) {
  const int lane = threadIdx.x;
  const int i = lane & 15, kq = lane >> 4;
  const int tiles_e = (p.E + 15) / 16;
  int blk = blockIdx.x;
  if (blk < p.nv + p.nt) {
    const bool video = blk < p.nv;
    if (!video) blk -= p.nv;
    const int r0 = (blk / tiles_e) * 16, e0 = (blk % tiles_e) * 16;
    const int R = video ? p.B : p.C;              // rows of the output
    const int K = video ? p.C : p.B;              // contraction length
    const float* rhs = video ? p.cm : p.vn;       // [K][E]
    const bool row_ok = r0 + i < R, col_ok = e0 + i < p.E;
    f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + kq;
      float a = 0.f, b = 0.f;
      if (k < K) {
        if (row_ok) a = video ? p.dlogits[(long)(r0 + i) * p.C + k] : p.dlogits[(long)k * p.C + (r0 + i)];
        if (col_ok) b = rhs[(long)k * p.E + e0 + i];
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    const float ls = expf(p.logit_scale[0]);
    float* out = video ? p.dvn : p.dm;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * kq + r;
      if (row < R && col_ok) out[(long)row * p.E + e0 + i] = ls * acc[r];
    }
    return;
  }
  const float lb = p.logit_bias ? p.logit_bias[0] : 0.f;
  const long n = (long)p.B * p.C;
  // B * C / 64 terms of either sign per lane: compensated (Kahan) sums, so that the error does not grow with the batch
  float s = 0.f, t = 0.f, cs = 0.f, ct = 0.f;
  for (long j = lane; j < n; j += 64) {
    const float d = p.dlogits[j];
    const float ys = d * (p.logits[j] - lb) - cs, ns = s + ys;
    cs = (ns - s) - ys; s = ns;
    const float yt = d - ct, nt = t + yt;
    ct = (nt - t) - yt; t = nt;
  }
  s = wave_sum(s); t = wave_sum(t);
  if (lane == 0) {
    p.dls[0] = s;
    if (p.dlb) p.dlb[0] = t;
  }
}

// Launch 2, one wave per row of [video rows | prompt rows]: the backward of the L2 normalisations.
//   video row b:   dvideo = (dvn - vn <vn, dvn>) * video_inv
//   prompt row k of class c (count_c prompts): G = dm_c + (dtf_c - tf_c <tf_c, dtf_c>) / |m_c| with tf_c = m_c / |m_c| (the
//   re-normalised class mean's backward; every prompt of the class recomputes it, E values),  dtn = G / count_c,
//   dtext = (dtn - tn <tn, dtn>) * text_inv
struct HeadRowsParams {
  const float* vn; const float* vinv; const float* dvn; float* dvideo;
  const float* tn; const float* tinv; const float* cm; const float* dm; const float* dtf; float* dtext;
  const int* offsets;
  int B, C, P, E;
};

__global__ __launch_bounds__(256) void head_backward_rows_kernel(const HeadRowsParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B + p.P) return;
  if (row < p.B) {
    const float* u = p.vn + (long)row * p.E;
    const float* d = p.dvn + (long)row * p.E;
    float dot = 0.f;
    for (int e = lane; e < p.E; e += 64) dot += u[e] * d[e];
    dot = wave_sum(dot);
    const float inv = p.vinv[row];
    for (int e = lane; e < p.E; e += 64) p.dvideo[(long)row * p.E + e] = (d[e] - u[e] * dot) * inv;
    return;
  }
  const int k = row - p.B;
  // the class of prompt k: the last c with offsets[c] <= k (classes without prompts share their offset with the next one)
  int lo = 0, hi = p.C - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.offsets[mid] <= k) lo = mid; else hi = mid - 1;
  }
  const int c = lo;
  const float cnt = (float)(p.offsets[c + 1] - p.offsets[c]);
  const float* m = p.cm + (long)c * p.E;
  const float* dm = p.dm + (long)c * p.E;
  const float* u = p.tn + (long)k * p.E;
  float coef_q = 0.f, coef_m = 0.f;          // G = dm + coef_q * dtf - coef_m * m
  if (p.dtf) {
    const float* q = p.dtf + (long)c * p.E;
    float mm = 0.f, mq = 0.f;
    for (int e = lane; e < p.E; e += 64) { mm += m[e] * m[e]; mq += m[e] * q[e]; }
    mm = wave_sum(mm); mq = wave_sum(mq);
    const float rn = 1.0f / sqrtf(mm);       // 1 / |m|
    coef_q = rn;
    coef_m = mq * rn * rn * rn;              // <tf, dtf> / |m| * (tf / m) = <m, dtf> / |m|^3
  }
  float dot = 0.f;
  for (int e = lane; e < p.E; e += 64) {
    float g = dm[e];
    if (p.dtf) g += coef_q * p.dtf[(long)c * p.E + e] - coef_m * m[e];
    dot += u[e] * (g / cnt);
  }
  dot = wave_sum(dot);
  const float inv = p.tinv[k];
  for (int e = lane; e < p.E; e += 64) {
    float g = dm[e];
    if (p.dtf) g += coef_q * p.dtf[(long)c * p.E + e] - coef_m * m[e];
    p.dtext[(long)k * p.E + e] = (g / cnt - u[e] * dot) * inv;
  }
}

}  // namespace

extern "C" int gava_train_criterion(const gava_train_criterion_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->C < 1) return GAVA_EINVAL;
  if (!a->logits || !a->labels || !a->loss || !a->per_sample || !a->weight || !a->top1 || !a->hits || !a->saved) return GAVA_EINVAL;
  if (a->ld_logits < a->C) return GAVA_EINVAL;
  if (a->weighted && (!(a->gamma >= 1.0f) || a->C < 2)) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  CritParams p{a->logits, (long)a->ld_logits, (const long long*)a->labels, a->B, a->C, a->weighted, a->alpha, a->gamma, a->beta,
               a->scale, a->per_sample, a->weight, a->top1, a->conf, (float4*)a->saved};
  hipLaunchKernelGGL(criterion_rows_kernel, dim3((a->B + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(criterion_mean_kernel, dim3(1), dim3(256), 0, s, a->per_sample, a->top1, (const long long*)a->labels, a->B,
                     a->C, a->loss, a->hits);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_train_criterion_backward(const gava_train_criterion_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->C < 1) return GAVA_EINVAL;
  if (!a->logits || !a->labels || !a->saved || !a->grad_loss || !a->dlogits) return GAVA_EINVAL;
  if (a->ld_logits < a->C || a->ld_dlogits < a->C) return GAVA_EINVAL;
  hipLaunchKernelGGL(criterion_backward_kernel, dim3((a->B + 3) / 4), dim3(256), 0, (hipStream_t)stream, a->logits,
                     (long)a->ld_logits, (const long long*)a->labels, (const float4*)a->saved, a->grad_loss, a->B, a->C, a->dlogits,
                     (long)a->ld_dlogits);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

// what both directions need: the shape, the descriptor, the scale, and the buffers the forward fills and the backward reads
static bool head_shape_ok(const gava_train_head_args* a) {
  return a && a->B > 0 && a->C > 0 && a->P > 0 && a->E > 0 && a->E % 4 == 0 && a->class_offsets &&
         a->logit_scale && a->logits && a->video_norm && a->video_inv && a->text_norm && a->text_inv && a->class_mean;
}

extern "C" int gava_train_head(const gava_train_head_args* a, gava_stream_t stream) {
  if (!head_shape_ok(a) || !a->video || !a->text || !a->text_features) return GAVA_EINVAL;
  return gava::train_head_forward(a->video, a->text, a->class_offsets, a->logit_scale, a->logit_bias, a->B, a->C, a->P, a->E,
                                  a->logits, a->text_features, a->video_norm, a->video_inv, a->text_norm, a->text_inv,
                                  a->class_mean, (hipStream_t)stream);
}

extern "C" int gava_train_head_backward(const gava_train_head_args* a, gava_stream_t stream) {
  if (!head_shape_ok(a)) return GAVA_EINVAL;
  if (!a->dlogits || !a->dvideo || !a->dtext || !a->dlogit_scale || !a->workspace) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles_e = (a->E + 15) / 16;
  float* dvn = a->workspace;
  float* dm = a->workspace + (size_t)a->B * a->E;
  HeadBwdParams g{a->dlogits, a->logits, a->logit_scale, a->logit_bias, a->video_norm, a->class_mean, dvn, dm, a->dlogit_scale,
                  a->dlogit_bias, a->B, a->C, a->E, ((a->B + 15) / 16) * tiles_e, ((a->C + 15) / 16) * tiles_e};
  hipLaunchKernelGGL(head_backward_gemm_kernel, dim3(g.nv + g.nt + 1), dim3(64), 0, s, g);
  HeadRowsParams r{a->video_norm, a->video_inv, dvn, a->dvideo, a->text_norm, a->text_inv, a->class_mean, dm, a->dtext_features,
                   a->dtext, a->class_offsets, a->B, a->C, a->P, a->E};
  hipLaunchKernelGGL(head_backward_rows_kernel, dim3((a->B + a->P + 3) / 4), dim3(256), 0, s, r);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_train_struct_sizes(size_t* out, int cap) {
  const size_t v[] = {sizeof(gava_train_criterion_args), sizeof(gava_train_head_args)};
  for (int i = 0; out && i < 2 && i < cap; ++i) out[i] = v[i];
  return 2;
}
