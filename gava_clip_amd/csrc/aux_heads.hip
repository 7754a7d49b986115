// aux_heads.hip — the auxiliary heads of a training step and their loss terms on the device (opt-in: VitaCLIP.aux_heads = "hip",
// gava_clip_amd.AuxCriterion): the video<->NTE head (VitaCLIP_model.py:311-345), the support-memory<->text head (:347-398), the
// sigmoid (focal) criterion of loss_utils.py:139-177 and the diagonal NTE term of train.py:471-475, each with its backward.
// Everything is fp32.  Reductions run in a fixed order (xor butterflies inside a wave, an LDS tree across the four waves of a
// workgroup, plain ordered loops across rows); no atomics: a call repeats bit for bit.  The small matrix products are ordered fp32
// fma chains on the VALU - 16-byte loads along the contraction where it is contiguous - in three shared kernels (y = x W^T + b,
// dx = dy W, dW = dy^T x) whose z grid dimension is the class: per-class weights arrive through a device table of pointers.
// Every workgroup has 256 threads.
#include "common.h"
#include "internal.h"

namespace {

// sum / max over the 256 threads of a workgroup, in every thread; sh: 4 floats of LDS (reusable right after the call returns)
static __device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

static __device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// a * b rounded on its own: never contracted into an fma with a following add or subtract
static __device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

static __device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// ---- the three linear kernels ---------------------------------------------------------------------------------------------------
// Class z = blockIdx.z reads its weights from tab[z * 4 + slot] when a table is given (else W / b), its activations z * *_cs
// elements into each array (a class stride of 0 shares the array between the classes).
// Which fields a kernel reads (the host fills only those; the rest stay zero):
//   linear_forward_kernel:  X x_cs, W b or tab w_slot b_slot, Y y_cs, R N K act
//   linear_dx_kernel:       dY dy_cs, W or tab w_slot, H (optional), dX dx_cs, R N K
//   linear_dw_kernel:       dY dy_cs, X x_cs, dW db, R N K                      (no weights: W / tab may be null)
struct LinParams {
  const float* X; long x_cs;                     // [R][K]: the forward's input, the weight gradient's right operand
  const float* W; const float* b;                // [N][K], [N] (b optional)
  const float* const* tab; int w_slot, b_slot;
  float* Y; long y_cs;                           // forward: [R][N]
  const float* dY; long dy_cs;                   // backward: [R][N]
  const float* H; float* dX; long dx_cs;         // dx [R][K]; H: tanh outputs of dx's shape and stride, dx *= 1 - H^2 (optional)
  float* dW; float* db;                          // [Z][N][K], [Z][N]
  int R, N, K, act;                              // act 1: tanh
};

static __device__ __forceinline__ const float* lin_weight(const LinParams& p) { return p.tab ? p.tab[blockIdx.z * 4 + p.w_slot] : p.W; }

// Y[r][n] = act(<X[r], W[n]> + b[n]): one wave per output column n and 8 rows r; lanes stride the contraction 16 bytes at a time
// (K % 4 == 0), so a weight row is read once per 8 rows
__global__ __launch_bounds__(256) void linear_forward_kernel(const LinParams p) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), r0 = blockIdx.y * 8;
  if (n >= p.N) return;
  const float* X = p.X + blockIdx.z * p.x_cs;
  const float4* w4 = (const float4*)(lin_weight(p) + (long)n * p.K);
  const float* b = p.tab ? p.tab[blockIdx.z * 4 + p.b_slot] : p.b;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = lane; k < p.K / 4; k += 64) {
    const float4 w = w4[k];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r0 + r < p.R) acc[r] += dot4(w, ((const float4*)(X + (long)(r0 + r) * p.K))[k]);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float s = wave_sum(acc[r]);
    if (lane == 0 && r0 + r < p.R) {
      if (b) s += b[n];
      if (p.act) s = tanhf(s);
      p.Y[blockIdx.z * p.y_cs + (long)(r0 + r) * p.N + n] = s;
    }
  }
}

// dX[r][k] = (sum_n dY[r][n] W[n][k]) * (1 - H[r][k]^2): one thread per column k and 8 rows r, n ascending
__global__ __launch_bounds__(256) void linear_dx_kernel(const LinParams p) {
  const int k = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * 8;
  if (k >= p.K) return;
  const float* W = lin_weight(p);
  const float* dY = p.dY + blockIdx.z * p.dy_cs;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < p.N; ++n) {
    const float w = W[(long)n * p.K + k];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r0 + r < p.R) acc[r] += dY[(long)(r0 + r) * p.N + n] * w;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (r0 + r >= p.R) break;
    const long o = blockIdx.z * p.dx_cs + (long)(r0 + r) * p.K + k;
    float v = acc[r];
    if (p.H) { const float h = p.H[o]; v *= 1.0f - h * h; }
    p.dX[o] = v;
  }
}

// dW[n][k] = sum_r dY[r][n] X[r][k], db[n] = sum_r dY[r][n]: one thread per (n, k), r ascending
__global__ __launch_bounds__(256) void linear_dw_kernel(const LinParams p) {
  const int k = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (k >= p.K) return;
  const float* dY = p.dY + blockIdx.z * p.dy_cs;
  const float* X = p.X + blockIdx.z * p.x_cs;
  float acc = 0.f, sb = 0.f;
  for (int r = 0; r < p.R; ++r) {
    const float d = dY[(long)r * p.N + n];
    acc += d * X[(long)r * p.K + k];
    sb += d;
  }
  p.dW[((long)blockIdx.z * p.N + n) * p.K + k] = acc;
  if (k == 0) p.db[(long)blockIdx.z * p.N + n] = sb;
}

static void linear_forward(const LinParams& p, int classes, hipStream_t s) {
  hipLaunchKernelGGL(linear_forward_kernel, dim3((p.N + 3) / 4, (p.R + 7) / 8, classes), dim3(256), 0, s, p);
}
static void linear_dx(const LinParams& p, int classes, hipStream_t s) {
  hipLaunchKernelGGL(linear_dx_kernel, dim3((p.K + 255) / 256, (p.R + 7) / 8, classes), dim3(256), 0, s, p);
}
static void linear_dw(const LinParams& p, int classes, hipStream_t s) {
  hipLaunchKernelGGL(linear_dw_kernel, dim3((p.K + 255) / 256, p.N, classes), dim3(256), 0, s, p);
}

// out[job] = mult * sum of in[job][0 .. n): one workgroup per job (blockIdx.x = 0, 1); thread t adds t, t + 256, ... in order
__global__ __launch_bounds__(256) void reduce_sum_kernel(const float* in0, const float* in1, int n, float mult, float* out0, float* out1) {
  __shared__ float sh[4];
  const float* in = blockIdx.x ? in1 : in0;
  float* out = blockIdx.x ? out1 : out0;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += in[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = s * mult;
}

// ---- NTE head ---------------------------------------------------------------------------------------------------------------------
// The one pass over video_nte [B][K][E]: one workgroup per clip, wave w takes rows w, w + 4, ...  A row stays in registers between
// its norm and its scaling (E <= 1024: four 16-byte loads per lane).  -> mean of the unit rows, valid = (element sum != 0)
__global__ __launch_bounds__(256) void nte_reduce_kernel(const float* nte, int K, int E, float* mean, float* valid) {
  __shared__ __attribute__((aligned(16))) float acc_s[4][1024];
  __shared__ float es_s[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, E4 = E / 4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc[4] = {zero, zero, zero, zero};
  float es = 0.f;
  for (int k = w; k < K; k += 4) {
    const float4* row = (const float4*)(nte + ((long)blockIdx.x * K + k) * E);
    float4 v[4];
    float ss = 0.f, e1 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = lane + 64 * q;
      v[q] = i < E4 ? row[i] : zero;
      ss += dot4(v[q], v[q]);
      e1 += (v[q].x + v[q].y) + (v[q].z + v[q].w);
    }
    ss = wave_sum(ss);
    es += wave_sum(e1);
    const float inv = 1.0f / sqrtf(ss);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[q].x += v[q].x * inv; acc[q].y += v[q].y * inv; acc[q].z += v[q].z * inv; acc[q].w += v[q].w * inv;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    if (i < E4) ((float4*)acc_s[w])[i] = acc[q];
  }
  if (lane == 0) es_s[w] = es;
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += 256)
    mean[(long)blockIdx.x * E + e] = ((acc_s[0][e] + acc_s[1][e]) + (acc_s[2][e] + acc_s[3][e])) / (float)K;
  if (threadIdx.x == 0) valid[blockIdx.x] = ((es_s[0] + es_s[1]) + (es_s[2] + es_s[3])) != 0.f ? 1.0f : 0.f;
}

// Row i: sp[i] <- sp[i] / |sp[i]| in place (sp holds summary W^T + b on entry), then sim[i][j] = <sp[i], mean[j]> valid_i valid_j
// and lm = scale * sim, one wave per j
__global__ __launch_bounds__(256) void nte_sim_kernel(float* sp, float* sp_inv, const float* mean, const float* valid,
                                                      const float* scale, int B, int E, float* sim, float* lm) {
  __shared__ __attribute__((aligned(16))) float row[1024];
  __shared__ float sh[4];
  const int i = blockIdx.x, lane = threadIdx.x & 63;
  float ss = 0.f;
  for (int e = threadIdx.x; e < E; e += 256) { const float v = sp[(long)i * E + e]; row[e] = v; ss += v * v; }
  const float inv = 1.0f / sqrtf(block_sum(ss, sh));
  for (int e = threadIdx.x; e < E; e += 256) { const float v = row[e] * inv; row[e] = v; sp[(long)i * E + e] = v; }
  if (threadIdx.x == 0) sp_inv[i] = inv;
  __syncthreads();
  const float sc = scale[0], vi = valid[i];
  for (int j = threadIdx.x >> 6; j < B; j += 4) {
    const float4* m4 = (const float4*)(mean + (long)j * E);
    float d = 0.f;
    for (int k = lane; k < E / 4; k += 64) d += dot4(((const float4*)row)[k], m4[k]);
    d = wave_sum(d);
    if (lane == 0) {
      const float sm = d * (vi * valid[j]);
      sim[(long)i * B + j] = sm;
      lm[(long)i * B + j] = sc * sm;
    }
  }
}

// workgroups [0, B): log-sum-exp of row i of lm;  [B, 2B): of column j
__global__ __launch_bounds__(256) void nte_lse_kernel(const float* lm, int B, float* row_lse, float* col_lse) {
  __shared__ float sh[4];
  const bool col = (int)blockIdx.x >= B;
  const int r = col ? blockIdx.x - B : blockIdx.x;
  const float* base = col ? lm + r : lm + (long)r * B;
  const long step = col ? B : 1;
  float m = -INFINITY;
  for (int t = threadIdx.x; t < B; t += 256) m = fmaxf(m, base[t * step]);
  m = block_max(m, sh);
  float s = 0.f;
  for (int t = threadIdx.x; t < B; t += 256) s += expf(base[t * step] - m);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) (col ? col_lse : row_lse)[r] = m + logf(s);
}

__global__ __launch_bounds__(256) void nte_out_kernel(const float* lm, const float* row_lse, const float* col_lse, int B, float* out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)B * B) return;
  const float l = lm[t];
  out[t] = (l - row_lse[t / B]) + (l - col_lse[t % B]);
}

// workgroups [0, B): sum of row i of dlogits;  [B, 2B): of column j
__global__ __launch_bounds__(256) void nte_bwd_sums_kernel(const float* g, int B, float* gr, float* gc) {
  __shared__ float sh[4];
  const bool col = (int)blockIdx.x >= B;
  const int r = col ? blockIdx.x - B : blockIdx.x;
  const float* base = col ? g + r : g + (long)r * B;
  const long step = col ? B : 1;
  float s = 0.f;
  for (int t = threadIdx.x; t < B; t += 256) s += base[t * step];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) (col ? gc : gr)[r] = s;
}

// Row i:  dlm = 2 g - softmax_row gr_i - softmax_col gc_j;  dscale_part[i] = sum_j dlm sim;  dsim = dlm scale valid_i valid_j;
// dsp = dsim[i] @ mean (j ascending);  dy[i] = (dsp - sp <sp, dsp>) / |y|
struct NteBwdParams {
  const float* g; const float* lm; const float* sim; const float* row_lse; const float* col_lse; const float* gr; const float* gc;
  const float* valid; const float* scale; const float* mean; const float* sp; const float* sp_inv;
  float* dsim; float* dscale_part; float* dy;
  int B, E;
};

__global__ __launch_bounds__(256) void nte_bwd_rows_kernel(const NteBwdParams p) {
  __shared__ float dsp[1024];
  __shared__ float sh[4];
  const int i = blockIdx.x, B = p.B, E = p.E;
  const float sc = p.scale[0], vi = p.valid[i], rl = p.row_lse[i], gri = p.gr[i];
  float part = 0.f;
  for (int j = threadIdx.x; j < B; j += 256) {
    const long o = (long)i * B + j;
    const float l = p.lm[o];
    const float d = 2.0f * p.g[o] - expf(l - rl) * gri - expf(l - p.col_lse[j]) * p.gc[j];
    part += d * p.sim[o];
    p.dsim[o] = d * sc * (vi * p.valid[j]);
  }
  part = block_sum(part, sh);
  if (threadIdx.x == 0) p.dscale_part[i] = part;
  __syncthreads();                                  // row i of dsim, written by this workgroup, is read by all of its threads
  float dot = 0.f;
  for (int e = threadIdx.x; e < E; e += 256) {
    float a = 0.f;
    for (int j = 0; j < B; ++j) a += p.dsim[(long)i * B + j] * p.mean[(long)j * E + e];
    dsp[e] = a;
    dot += a * p.sp[(long)i * E + e];
  }
  dot = block_sum(dot, sh);
  const float inv = p.sp_inv[i];
  for (int e = threadIdx.x; e < E; e += 256) p.dy[(long)i * E + e] = (dsp[e] - p.sp[(long)i * E + e] * dot) * inv;
}

// ---- support-memory head ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void memory_mean_kernel(const float* memory, int M, int S, int E, float* mean) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int E4 = E / 4;
  if (t >= (long)M * E4) return;
  const long m = t / E4, e = t % E4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < S; ++s) {
    const float4 v = ((const float4*)(memory + (m * S + s) * E))[e];
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  const float n = (float)S;
  ((float4*)(mean + m * E))[e] = make_float4(a.x / n, a.y / n, a.z / n, a.w / n);
}

// Memory row m: one wave per class c: cos[m][c] = <z_c[m], u_c> / (|z_c[m]| |u_c|); then the log-softmax of scale * cos over the
// classes, + bias
struct MemLogitsParams {
  const float* z; const float* u; const float* scale; const float* bias;
  float* zinv; float* uinv; float* cosine; float* lse; float* logits;
  int M, C, H2;
};

__global__ __launch_bounds__(256) void memory_logits_kernel(const MemLogitsParams p) {
  __shared__ float sh[4];
  const int m = blockIdx.x, lane = threadIdx.x & 63;
  for (int c = threadIdx.x >> 6; c < p.C; c += 4) {
    const float* z = p.z + ((long)c * p.M + m) * p.H2;
    const float* u = p.u + (long)c * p.H2;
    float zz = 0.f, uu = 0.f, zu = 0.f;
    for (int h = lane; h < p.H2; h += 64) { const float a = z[h], b = u[h]; zz += a * a; uu += b * b; zu += a * b; }
    zz = wave_sum(zz); uu = wave_sum(uu); zu = wave_sum(zu);
    const float zi = 1.0f / sqrtf(zz), ui = 1.0f / sqrtf(uu);
    if (lane == 0) {
      p.zinv[(long)m * p.C + c] = zi;
      if (m == 0) p.uinv[c] = ui;
      p.cosine[(long)m * p.C + c] = (zu * zi) * ui;
    }
  }
  __syncthreads();                                  // row m of cosine, written by this workgroup
  const float sc = p.scale[0], lb = p.bias ? p.bias[0] : 0.f;
  const float* cs = p.cosine + (long)m * p.C;
  float mx = -INFINITY;
  // mul_rounded: the product is rounded before the subtraction (no fma contraction), so that the maximum's own term is exp(0)
  // and a single class gives exactly log_softmax = 0; the backward forms the same product
  for (int c = threadIdx.x; c < p.C; c += 256) mx = fmaxf(mx, mul_rounded(sc, cs[c]));
  mx = block_max(mx, sh);
  float s = 0.f;
  for (int c = threadIdx.x; c < p.C; c += 256) s += expf(mul_rounded(sc, cs[c]) - mx);
  s = block_sum(s, sh);
  const float lse = mx + logf(s);
  if (threadIdx.x == 0) p.lse[m] = lse;
  for (int c = threadIdx.x; c < p.C; c += 256) p.logits[(long)m * p.C + c] = (mul_rounded(sc, cs[c]) - lse) + lb;
}

// Memory row m: draw = g - softmax sum_c g;  dcos = draw scale;  dz_c[m] = dcos (u^ - z^ cos) / |z|;  the row's shares of
// dscale (sum_c draw cos) and dbias (sum_c g)
struct MemBwdParams {
  const float* g; const float* cosine; const float* lse; const float* scale;
  const float* z; const float* zinv; const float* u; const float* uinv;
  float* dcos; float* dz; float* part_scale; float* part_bias;
  int M, C, H2;
};

__global__ __launch_bounds__(256) void memory_bwd_rows_kernel(const MemBwdParams p) {
  __shared__ float sh[4];
  const int m = blockIdx.x, lane = threadIdx.x & 63;
  float gs = 0.f;
  for (int c = threadIdx.x; c < p.C; c += 256) gs += p.g[(long)m * p.C + c];
  gs = block_sum(gs, sh);
  const float sc = p.scale[0], lse = p.lse[m];
  float part = 0.f;
  for (int c = threadIdx.x >> 6; c < p.C; c += 4) {
    const long o = (long)m * p.C + c;
    const float cs = p.cosine[o];
    const float draw = p.g[o] - expf(mul_rounded(sc, cs) - lse) * gs;
    const float dcos = draw * sc, zi = p.zinv[o], ui = p.uinv[c];
    if (lane == 0) { p.dcos[o] = dcos; part += draw * cs; }
    const float* z = p.z + ((long)c * p.M + m) * p.H2;
    const float* u = p.u + (long)c * p.H2;
    float* dz = p.dz + ((long)c * p.M + m) * p.H2;
    for (int h = lane; h < p.H2; h += 64) dz[h] = dcos * (u[h] * ui - (z[h] * zi) * cs) * zi;
  }
  part = block_sum(part, sh);
  if (threadIdx.x == 0) { p.part_scale[m] = part; p.part_bias[m] = gs; }
}

// Class c (one wave): du^ = sum_m dcos[m][c] z^_c[m] (m ascending);  du_c = (du^ - u^ <u^, du^>) / |u|
__global__ __launch_bounds__(256) void memory_bwd_text_kernel(const MemBwdParams p, float* du) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= p.C) return;
  const float ui = p.uinv[c];
  const float* u = p.u + (long)c * p.H2;
  float* out = du + (long)c * p.H2;
  float dot = 0.f;
  for (int h = lane; h < p.H2; h += 64) {
    float a = 0.f;
    for (int m = 0; m < p.M; ++m) a += p.dcos[(long)m * p.C + c] * (p.z[((long)c * p.M + m) * p.H2 + h] * p.zinv[(long)m * p.C + c]);
    out[h] = a;                                     // read back below by the lane that wrote it
    dot += a * (u[h] * ui);
  }
  dot = wave_sum(dot);
  for (int h = lane; h < p.H2; h += 64) out[h] = (out[h] - (u[h] * ui) * dot) * ui;
}

// ---- loss terms -------------------------------------------------------------------------------------------------------------------
// softplus and sigmoid that keep their relative accuracy at large |x|
static __device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
static __device__ __forceinline__ float sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

struct SigParams {
  const float* x; long ld; const long long* labels;
  int M, C, focal;
  float alpha, gamma, scale;
  float* per_sample; const float* grad; float* dx; long ldd;
};

// One wave per sample.  With t = +1 at the label and -1 elsewhere, v = -t x:  ce = softplus(v) = -logsigmoid(t x),
// q = sigmoid(v) = 1 - p_t;  term = ce, or alpha_t q^gamma ce with use_focal
__global__ __launch_bounds__(256) void sigmoid_rows_kernel(const SigParams p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.M) return;
  const long long y = p.labels[row];
  float s = 0.f;
  for (int c = lane; c < p.C; c += 64) {
    const bool pos = c == y;
    const float v = pos ? -p.x[row * p.ld + c] : p.x[row * p.ld + c];
    float l = softplus(v);
    if (p.focal) l *= (pos ? p.alpha : 1.0f - p.alpha) * powf(sigmoid(v), p.gamma);
    s += l;
  }
  s = wave_sum(s);
  if (lane == 0) p.per_sample[row] = s * p.scale;
}

// d term / d x = -t q, or with use_focal -t alpha_t q^gamma (gamma (1 - q) ce + q);  times scale * grad / M
__global__ __launch_bounds__(256) void sigmoid_backward_kernel(const SigParams p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.M) return;
  const long long y = p.labels[row];
  const float g = p.grad[0] * p.scale / (float)p.M;
  for (int c = lane; c < p.C; c += 64) {
    const bool pos = c == y;
    const float v = pos ? -p.x[row * p.ld + c] : p.x[row * p.ld + c];
    const float q = sigmoid(v);
    float d = q;
    if (p.focal) d = (pos ? p.alpha : 1.0f - p.alpha) * powf(q, p.gamma) * (p.gamma * sigmoid(-v) * softplus(v) + q);
    p.dx[row * p.ldd + c] = (pos ? -d : d) * g;
  }
}

// loss = -weight * mean_i logits_vm[i][i]: one workgroup
__global__ __launch_bounds__(256) void nte_diag_kernel(const float* lv, int B, float weight, float* loss) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) s += lv[(long)i * B + i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = -weight * (s / (float)B);
}

__global__ __launch_bounds__(256) void nte_diag_backward_kernel(const float* grad, int B, float weight, float* d) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)B * B) return;
  d[t] = t / B == t % B ? -weight * grad[0] / (float)B : 0.f;
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool nte_shape_ok(const gava_nte_head_args* a) {
  return a && a->B > 0 && a->D > 0 && a->E > 0 && a->K > 0 && a->D % 4 == 0 && a->E % 4 == 0 && a->E <= 1024 && a->B <= 32767 &&
         a->summary && a->weight && a->logit_scale && a->sp_norm && a->sp_inv && a->nte_mean && a->valid && a->sim && a->lm &&
         a->row_lse && a->col_lse && al16(a->summary) && al16(a->weight) && al16(a->sp_norm) && al16(a->nte_mean);
}

static bool memory_shape_ok(const gava_memory_head_args* a) {
  return a && a->M > 0 && a->S > 0 && a->C > 0 && a->E > 0 && a->E % 16 == 0 && a->C <= 65535 && a->text_features && a->mem_params &&
         a->tf_w1 && a->tf_b1 && a->tf_w2 && a->tf_b2 && a->logit_scale && a->mem_mean && a->mem_h && a->mem_z && a->mem_inv &&
         a->tf_h && a->tf_u && a->tf_inv && a->cosine && a->lse && al16(a->text_features) && al16(a->tf_w1) && al16(a->tf_w2) &&
         al16(a->mem_mean) && al16(a->mem_h) && al16(a->tf_h);
}

}  // namespace

extern "C" int gava_nte_head(const gava_nte_head_args* a, gava_stream_t stream) {
  if (!nte_shape_ok(a) || !a->video_nte || !a->logits_vm || !al16(a->video_nte)) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int B = a->B, E = a->E;
  hipLaunchKernelGGL(nte_reduce_kernel, dim3(B), dim3(256), 0, s, a->video_nte, a->K, E, a->nte_mean, a->valid);
  LinParams l{};
  l.X = a->summary; l.W = a->weight; l.b = a->bias; l.Y = a->sp_norm; l.R = B; l.N = E; l.K = a->D;
  linear_forward(l, 1, s);
  hipLaunchKernelGGL(nte_sim_kernel, dim3(B), dim3(256), 0, s, a->sp_norm, a->sp_inv, a->nte_mean, a->valid, a->logit_scale, B, E,
                     a->sim, a->lm);
  hipLaunchKernelGGL(nte_lse_kernel, dim3(2 * B), dim3(256), 0, s, a->lm, B, a->row_lse, a->col_lse);
  hipLaunchKernelGGL(nte_out_kernel, dim3((unsigned)(((long)B * B + 255) / 256)), dim3(256), 0, s, a->lm, a->row_lse, a->col_lse, B,
                     a->logits_vm);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" size_t gava_nte_head_backward_workspace_floats(int B, int E) { return (size_t)B * ((size_t)B + E + 3); }

extern "C" int gava_nte_head_backward(const gava_nte_head_args* a, gava_stream_t stream) {
  if (!nte_shape_ok(a)) return GAVA_EINVAL;
  if (!a->dlogits || !a->dsummary || !a->dweight || !a->dbias || !a->dlogit_scale || !a->workspace) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int B = a->B, E = a->E;
  float* gr = a->workspace;
  float* gc = gr + B;
  float* part = gc + B;
  float* dsim = part + B;
  float* dy = dsim + (size_t)B * B;
  hipLaunchKernelGGL(nte_bwd_sums_kernel, dim3(2 * B), dim3(256), 0, s, a->dlogits, B, gr, gc);
  NteBwdParams r{a->dlogits, a->lm, a->sim, a->row_lse, a->col_lse, gr, gc, a->valid, a->logit_scale, a->nte_mean, a->sp_norm,
                 a->sp_inv, dsim, part, dy, B, E};
  hipLaunchKernelGGL(nte_bwd_rows_kernel, dim3(B), dim3(256), 0, s, r);
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, s, part, part, B, 1.0f, a->dlogit_scale, a->dlogit_scale);
  LinParams l{};
  l.X = a->summary; l.W = a->weight; l.dY = dy; l.dX = a->dsummary; l.dW = a->dweight; l.db = a->dbias; l.R = B; l.N = E; l.K = a->D;
  linear_dw(l, 1, s);
  linear_dx(l, 1, s);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_memory_head(const gava_memory_head_args* a, gava_stream_t stream) {
  if (!memory_shape_ok(a) || !a->memory || !a->logits_mt || !al16(a->memory)) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int M = a->M, C = a->C, E = a->E, H1 = E / 4, H2 = E / 8;
  hipLaunchKernelGGL(memory_mean_kernel, dim3((unsigned)(((long)M * (E / 4) + 255) / 256)), dim3(256), 0, s, a->memory, M, a->S, E,
                     a->mem_mean);
  LinParams t1{}, t2{}, m1{}, m2{};
  t1.X = a->text_features; t1.W = a->tf_w1; t1.b = a->tf_b1; t1.Y = a->tf_h; t1.R = C; t1.N = H1; t1.K = E; t1.act = 1;
  t2.X = a->tf_h; t2.W = a->tf_w2; t2.b = a->tf_b2; t2.Y = a->tf_u; t2.R = C; t2.N = H2; t2.K = H1;
  m1.X = a->mem_mean; m1.tab = a->mem_params; m1.w_slot = 0; m1.b_slot = 1; m1.Y = a->mem_h; m1.y_cs = (long)M * H1;
  m1.R = M; m1.N = H1; m1.K = E; m1.act = 1;
  m2.X = a->mem_h; m2.x_cs = (long)M * H1; m2.tab = a->mem_params; m2.w_slot = 2; m2.b_slot = 3; m2.Y = a->mem_z; m2.y_cs = (long)M * H2;
  m2.R = M; m2.N = H2; m2.K = H1;
  linear_forward(t1, 1, s);
  linear_forward(t2, 1, s);
  linear_forward(m1, C, s);
  linear_forward(m2, C, s);
  MemLogitsParams p{a->mem_z, a->tf_u, a->logit_scale, a->logit_bias, a->mem_inv, a->tf_inv, a->cosine, a->lse, a->logits_mt, M, C, H2};
  hipLaunchKernelGGL(memory_logits_kernel, dim3(M), dim3(256), 0, s, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" size_t gava_memory_head_backward_workspace_floats(int M, int C, int E) {
  const size_t H = (size_t)(E / 4 + E / 8);
  return (size_t)M * C + (size_t)C * M * H + (size_t)C * H + 2 * (size_t)M;
}

extern "C" int gava_memory_head_backward(const gava_memory_head_args* a, gava_stream_t stream) {
  if (!memory_shape_ok(a)) return GAVA_EINVAL;
  if (!a->dlogits || !a->dmem_w1 || !a->dmem_b1 || !a->dmem_w2 || !a->dmem_b2 || !a->dtf_w1 || !a->dtf_b1 || !a->dtf_w2 ||
      !a->dtf_b2 || !a->dlogit_scale || !a->workspace || (a->logit_bias && !a->dlogit_bias))
    return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int M = a->M, C = a->C, E = a->E, H1 = E / 4, H2 = E / 8;
  float* dcos = a->workspace;
  float* dz = dcos + (size_t)M * C;
  float* dh = dz + (size_t)C * M * H2;
  float* du = dh + (size_t)C * M * H1;
  float* dth = du + (size_t)C * H2;
  float* part_scale = dth + (size_t)C * H1;
  float* part_bias = part_scale + M;
  MemBwdParams p{a->dlogits, a->cosine, a->lse, a->logit_scale, a->mem_z, a->mem_inv, a->tf_u, a->tf_inv, dcos, dz, part_scale,
                 part_bias, M, C, H2};
  hipLaunchKernelGGL(memory_bwd_rows_kernel, dim3(M), dim3(256), 0, s, p);
  hipLaunchKernelGGL(memory_bwd_text_kernel, dim3((C + 3) / 4), dim3(256), 0, s, p, du);
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(a->dlogit_bias ? 2 : 1), dim3(256), 0, s, part_scale, part_bias, M, 1.0f, a->dlogit_scale,
                     a->dlogit_bias);
  // memory_project[c]: second layer's parameters, back through it and the tanh, first layer's parameters
  LinParams m2{}, m1{}, t2{}, t1{};
  m2.X = a->mem_h; m2.x_cs = (long)M * H1; m2.tab = a->mem_params; m2.w_slot = 2; m2.dY = dz; m2.dy_cs = (long)M * H2;
  m2.H = a->mem_h; m2.dX = dh; m2.dx_cs = (long)M * H1; m2.dW = a->dmem_w2; m2.db = a->dmem_b2; m2.R = M; m2.N = H2; m2.K = H1;
  m1.X = a->mem_mean; m1.dY = dh; m1.dy_cs = (long)M * H1; m1.dW = a->dmem_w1; m1.db = a->dmem_b1; m1.R = M; m1.N = H1; m1.K = E;
  linear_dw(m2, C, s);
  linear_dx(m2, C, s);
  linear_dw(m1, C, s);
  // tf_project: its rows are the classes, so the sums over r are the sums over the classes in class order
  t2.X = a->tf_h; t2.W = a->tf_w2; t2.dY = du; t2.H = a->tf_h; t2.dX = dth; t2.dW = a->dtf_w2; t2.db = a->dtf_b2;
  t2.R = C; t2.N = H2; t2.K = H1;
  t1.X = a->text_features; t1.W = a->tf_w1; t1.dY = dth; t1.dX = a->dtext_features; t1.dW = a->dtf_w1; t1.db = a->dtf_b1;
  t1.R = C; t1.N = H1; t1.K = E;
  linear_dw(t2, 1, s);
  linear_dx(t2, 1, s);
  linear_dw(t1, 1, s);
  if (a->dtext_features) linear_dx(t1, 1, s);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

static bool sigmoid_ok(const gava_sigmoid_criterion_args* a) {
  return a && a->M > 0 && a->C > 0 && a->logits && a->labels && a->ld_logits >= a->C && !(a->use_focal && !(a->gamma >= 1.0f));
}

extern "C" int gava_sigmoid_criterion(const gava_sigmoid_criterion_args* a, gava_stream_t stream) {
  if (!sigmoid_ok(a) || !a->loss || !a->per_sample) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  SigParams p{a->logits, (long)a->ld_logits, (const long long*)a->labels, a->M, a->C, a->use_focal, a->alpha, a->gamma, a->scale,
              a->per_sample, nullptr, nullptr, 0};
  hipLaunchKernelGGL(sigmoid_rows_kernel, dim3((a->M + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, s, a->per_sample, a->per_sample, a->M, 1.0f / (float)a->M, a->loss, a->loss);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_sigmoid_criterion_backward(const gava_sigmoid_criterion_args* a, gava_stream_t stream) {
  if (!sigmoid_ok(a) || !a->grad_loss || !a->dlogits || a->ld_dlogits < a->C) return GAVA_EINVAL;
  SigParams p{a->logits, (long)a->ld_logits, (const long long*)a->labels, a->M, a->C, a->use_focal, a->alpha, a->gamma, a->scale,
              nullptr, a->grad_loss, a->dlogits, (long)a->ld_dlogits};
  hipLaunchKernelGGL(sigmoid_backward_kernel, dim3((a->M + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_nte_diag_loss(const gava_nte_diag_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->B > 32767 || !a->logits_vm || !a->loss) return GAVA_EINVAL;
  hipLaunchKernelGGL(nte_diag_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->logits_vm, a->B, a->weight, a->loss);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_nte_diag_loss_backward(const gava_nte_diag_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->B > 32767 || !a->grad_loss || !a->dlogits_vm) return GAVA_EINVAL;
  hipLaunchKernelGGL(nte_diag_backward_kernel, dim3((unsigned)(((long)a->B * a->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     a->grad_loss, a->B, a->weight, a->dlogits_vm);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_aux_struct_sizes(size_t* out, int cap) {
  const size_t v[] = {sizeof(gava_nte_head_args), sizeof(gava_memory_head_args), sizeof(gava_sigmoid_criterion_args),
                      sizeof(gava_nte_diag_args)};
  for (int i = 0; out && i < 4 && i < cap; ++i) out[i] = v[i];
  return 4;
}
