// optimizer.hip — fused multi-tensor AdamW step that also refreshes the 16-bit weight copies (gava_adamw_step).
//
// One workgroup per chunk of at most 4096 elements of one tensor; a thread owns two groups of 8 consecutive elements.  The
// kernel is a stream over p, g, m, v (in) and p, m, v plus the copies (out): everything is loaded first, the scalar
// coefficients (double precision, thread 0) are computed while the loads fly, and every group moves 16 bytes per lane per
// instruction where its addresses allow.  A tensor with a transposed copy is cut into 64 x 64 tiles instead of linear ranges:
// rows of the tile are read 256 bytes at a time, the bf16 values cross an LDS tile, and columns are written 128 bytes at a time.
//
// gava_grad_norm walks the same chunk list with the same lane geometry (lane_groups) and reads g alone: one double partial per
// chunk, then one workgroup adds the partials per tensor and the tensors in table order.  gava_adamw_step_clipped is the step
// kernel's second instantiation: it multiplies the unscaled gradient by stats[1] and leaves when stats[2] is set.
#include "common.h"
#include <math.h>

namespace {

constexpr int kChunk = 4096;     // elements per linear chunk
constexpr int kTile = 64;        // tile edge of a tensor with a transposed copy (kTile * kTile == kChunk)
constexpr int kThreads = 256;
constexpr int kGroup = 8;        // consecutive elements per lane and pass
constexpr int kPasses = kChunk / (kThreads * kGroup);
static_assert(kTile * kTile == kChunk && kPasses == 2 && kTile / kGroup * (kTile / kPasses) == kThreads, "chunk geometry");

struct Groups { gava_adamw_group g[GAVA_ADAMW_MAX_GROUPS]; };

struct Coef { float inv_scale, decay, w1, beta2, w2, step_size, bc2_sqrt, eps; };

__device__ __forceinline__ bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// 8 consecutive floats, `cnt` of them valid
__device__ __forceinline__ void load8(const float* q, int cnt, float (&x)[kGroup]) {
  if (cnt == kGroup && aligned16(q)) {
    const float4 a = ((const float4*)q)[0], b = ((const float4*)q)[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kGroup; ++j) x[j] = j < cnt ? q[j] : 0.0f;
  }
}

__device__ __forceinline__ void store8(float* q, int cnt, const float (&x)[kGroup]) {
  if (cnt == kGroup && aligned16(q)) {
    ((float4*)q)[0] = make_float4(x[0], x[1], x[2], x[3]);
    ((float4*)q)[1] = make_float4(x[4], x[5], x[6], x[7]);
  } else {
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
      if (j < cnt) q[j] = x[j];
  }
}

__device__ __forceinline__ void store8_h16(unsigned short* q, int cnt, const unsigned short (&h)[kGroup]) {
  if (cnt == kGroup && aligned16(q)) {
    uint4 u;
    u.x = h[0] | (unsigned)h[1] << 16; u.y = h[2] | (unsigned)h[3] << 16;
    u.z = h[4] | (unsigned)h[5] << 16; u.w = h[6] | (unsigned)h[7] << 16;
    *(uint4*)q = u;
  } else {
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
      if (j < cnt) q[j] = h[j];
  }
}

// 1 / *grad_scale as every kernel here forms it (NULL: 1)
__device__ __forceinline__ float inv_scale_of(const float* grad_scale) { return grad_scale ? 1.0f / *grad_scale : 1.0f; }

// Where lane `tid`'s two groups of chunk `ch` sit: first element, number of valid elements, and (row, column) of the first one
// (row and column of a linear chunk are filled in only when the tensor has copies).
__device__ __forceinline__ void lane_groups(const gava_adamw_chunk& ch, const gava_adamw_tensor& t, bool tiled, bool copies, int tid,
                                            int (&e0)[kPasses], int (&cnt)[kPasses], int (&row)[kPasses], int (&col)[kPasses]) {
#pragma unroll
  for (int k = 0; k < kPasses; ++k) {
    if (tiled) {
      row[k] = ch.a + k * (kTile / kPasses) + tid / (kTile / kGroup);
      col[k] = ch.b + tid % (kTile / kGroup) * kGroup;
      const int left = row[k] >= 0 && row[k] < t.rows && col[k] >= 0 ? t.cols - col[k] : 0;
      cnt[k] = left < 0 ? 0 : left > kGroup ? kGroup : left;
      e0[k] = row[k] * t.cols + col[k];
    } else {
      const int len = ch.a < 0 || ch.b < 0 ? 0 : ch.b > kChunk ? kChunk : ch.b;
      const long end = (long)ch.a + len < t.n ? (long)ch.a + len : (long)t.n;
      const long first = (long)ch.a + (k * kThreads + tid) * kGroup;
      const long left = end - first;
      cnt[k] = left < 0 ? 0 : left > kGroup ? kGroup : (int)left;
      e0[k] = cnt[k] > 0 ? (int)first : 0;
      row[k] = col[k] = 0;
      if (copies && cnt[k] > 0) { row[k] = e0[k] / t.cols; col[k] = e0[k] - row[k] * t.cols; }
    }
  }
}

// kClip: the gradient is also multiplied by clip_stats[1] and the step is skipped when clip_stats[2] != 0 (gava_grad_norm's
// stats).  A template flag and not a test of the pointer: device code is compiled with floating-point contraction, so a run-time
// select between g * inv_scale and its clipped form would change how the first product fuses into the updates that follow, and
// the plain step would lose the bits it has.  The <false> instantiation is the kernel as it was.
template <bool kClip>
__global__ __launch_bounds__(kThreads) void adamw_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors,
                                                         const gava_adamw_chunk* __restrict__ chunks, Groups groups, int n_groups,
                                                         const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                         const float* __restrict__ clip_stats) {
  __shared__ Coef coef_s;
  __shared__ unsigned short tile[kTile][kTile + 2];   // row stride 33 dwords: the column reads of the transposed pass spread over the banks
  if (found_inf && *found_inf != 0.0f) return;        // a skipped step changes nothing (uniform: every workgroup leaves)
  if (kClip && clip_stats[2] != 0.0f) return;         // a non-finite gradient norm: skipped the same way
  const gava_adamw_chunk ch = chunks[blockIdx.x];
  if ((unsigned)ch.tensor >= (unsigned)n_tensors) return;
  const gava_adamw_tensor t = table[ch.tensor];
  if (!t.g || (unsigned)t.group >= (unsigned)n_groups) return;
  const bool tiled = t.copy_bf16_t != nullptr;
  const bool copies = t.copy_f32 || t.copy16 || t.copy_bf16;
  const int tid = threadIdx.x;

  int e0[kPasses], cnt[kPasses], row[kPasses], col[kPasses];
  lane_groups(ch, t, tiled, copies, tid, e0, cnt, row, col);

  float p[kPasses][kGroup], g[kPasses][kGroup], m[kPasses][kGroup], v[kPasses][kGroup];
#pragma unroll
  for (int k = 0; k < kPasses; ++k) {
    const int c = cnt[k];
    const long e = c > 0 ? e0[k] : 0;
    load8(t.p + e, c, p[k]); load8(t.g + e, c, g[k]); load8(t.m + e, c, m[k]); load8(t.v + e, c, v[k]);
  }

  if (tid == 0) {   // once per workgroup, in double, from the step count every chunk of the tensor still sees unchanged
    const gava_adamw_group h = groups.g[t.group];
    const double step = (double)*t.step + 1.0;
    const double bc1 = 1.0 - pow(h.beta1, step), bc2 = 1.0 - pow(h.beta2, step);
    Coef c;
    c.inv_scale = inv_scale_of(grad_scale);
    c.decay = (float)(1.0 - h.lr * h.weight_decay);
    c.w1 = (float)(1.0 - h.beta1);
    c.beta2 = (float)h.beta2;
    c.w2 = (float)(1.0 - h.beta2);
    c.step_size = (float)(h.lr / bc1);
    c.bc2_sqrt = (float)sqrt(bc2);
    c.eps = (float)h.eps;
    coef_s = c;
  }
  __syncthreads();
  const Coef c = coef_s;
  const float clip = kClip ? clip_stats[1] : 1.0f;

#pragma unroll
  for (int k = 0; k < kPasses; ++k) {
    unsigned short h16[kGroup], hb[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      float gj = g[k][j] * c.inv_scale;
      if (kClip) {   // fl32(fl32(g * inv_scale) * coef), the two roundings of unscale-then-clip: each product lands in a register
        asm volatile("" : "+v"(gj));   // before it is used, so neither is contracted into a neighbour
        gj *= clip;
        asm volatile("" : "+v"(gj));
      }
      float pj = p[k][j] * c.decay;
      const float mj = m[k][j] + (gj - m[k][j]) * c.w1;
      const float vj = v[k][j] * c.beta2 + c.w2 * gj * gj;
      pj = pj - c.step_size * (mj / (sqrtf(vj) / c.bc2_sqrt + c.eps));
      p[k][j] = pj; m[k][j] = mj; v[k][j] = vj;
      hb[j] = PrecBF16::cvt(pj);
      h16[j] = t.prec16 == GAVA_PREC_F16 ? PrecF16::cvt(pj) : hb[j];
    }
    const int n = cnt[k];
    if (n > 0) {
      const long e = e0[k];
      store8(t.p + e, n, p[k]); store8(t.m + e, n, m[k]); store8(t.v + e, n, v[k]);
      if (copies) {
        if (col[k] + n <= t.cols) {   // the group stays inside one row of the matrix
          if (t.copy_f32) store8(t.copy_f32 + row[k] * t.ld_f32 + col[k], n, p[k]);
          if (t.copy16) store8_h16((unsigned short*)t.copy16 + row[k] * t.ld16 + col[k], n, h16);
          if (t.copy_bf16) store8_h16((unsigned short*)t.copy_bf16 + row[k] * t.ld_bf16 + col[k], n, hb);
        } else {
          for (int j = 0; j < n; ++j) {
            const int r = (int)((e + j) / t.cols), cc = (int)((e + j) - (long)r * t.cols);
            if (t.copy_f32) t.copy_f32[r * t.ld_f32 + cc] = p[k][j];
            if (t.copy16) ((unsigned short*)t.copy16)[r * t.ld16 + cc] = h16[j];
            if (t.copy_bf16) ((unsigned short*)t.copy_bf16)[r * t.ld_bf16 + cc] = hb[j];
          }
        }
      }
      if (tiled) {
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
          if (j < n) tile[row[k] - ch.a][col[k] - ch.b + j] = hb[j];
      }
    }
  }

  if (tiled) {   // uniform per workgroup
    __syncthreads();
    unsigned short* out = (unsigned short*)t.copy_bf16_t;
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int lc = k * (kTile / kPasses) + tid / (kTile / kGroup), lr = tid % (kTile / kGroup) * kGroup;
      const int cc = ch.b + lc, r0 = ch.a + lr;
      if (ch.a < 0 || ch.b < 0 || cc >= t.cols) continue;
      const int left = t.rows - r0, n = left < 0 ? 0 : left > kGroup ? kGroup : left;
      if (n == 0) continue;
      unsigned short hb[kGroup];
#pragma unroll
      for (int j = 0; j < kGroup; ++j) hb[j] = tile[lr + j][lc];   // entries past n were never written and are never stored
      store8_h16(out + cc * t.ld_bf16_t + r0, n, hb);
    }
  }
}

__global__ void adamw_count_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors, const float* __restrict__ found_inf,
                                   const float* __restrict__ clip_stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tensors || (found_inf && *found_inf != 0.0f) || (clip_stats && clip_stats[2] != 0.0f)) return;
  if (table[i].g) *table[i].step += 1.0f;
}

// ---- the gradient norm ---------------------------------------------------------------------------------------------------
//
// Stage 1, one workgroup per chunk: partial[chunk] = sum of fl32(g * inv_scale)^2 over the chunk, in double.  The order is fixed:
// a lane adds its (at most) 16 squares in element order, a wave folds its 64 lanes through the halving tree 32, 16, ... 1, and
// thread 0 adds the four wave sums as (w0 + w1) + (w2 + w3).  The square of an fp32 value is exact in double.  Every
// workgroup writes its word, whatever its chunk names.
constexpr int kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors,
                                                              const gava_adamw_chunk* __restrict__ chunks,
                                                              const float* __restrict__ grad_scale, double* __restrict__ partial) {
  __shared__ double wave_s[kWaves];
  const int tid = threadIdx.x;
  const gava_adamw_chunk ch = chunks[blockIdx.x];
  double acc = 0.0;
  if ((unsigned)ch.tensor < (unsigned)n_tensors) {   // uniform per workgroup, like every test below
    const gava_adamw_tensor t = table[ch.tensor];
    if (t.g) {
      int e0[kPasses], cnt[kPasses], row[kPasses], col[kPasses];
      lane_groups(ch, t, t.copy_bf16_t != nullptr, false, tid, e0, cnt, row, col);
      float g[kPasses][kGroup];
#pragma unroll
      for (int k = 0; k < kPasses; ++k) load8(t.g + (cnt[k] > 0 ? e0[k] : 0), cnt[k], g[k]);
      const float inv_scale = inv_scale_of(grad_scale);
#pragma unroll
      for (int k = 0; k < kPasses; ++k)
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
          if (j < cnt[k]) {
            const double x = (double)(g[k][j] * inv_scale);   // the product adamw_kernel forms, rounded to fp32
            acc += x * x;
          }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) wave_s[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (wave_s[0] + wave_s[1]) + (wave_s[2] + wave_s[3]);
}

// Stage 2, one workgroup.  The chunk list is in table order (gava_adamw_plan writes it so), so the chunks of a tensor are one
// range: every lane looks at chunks and marks where a tensor's range starts and ends, in that tensor's workspace slot.  Then a
// lane per tensor adds the tensor's partials in chunk order, sixteen loads in flight at a time, and puts the sum into its slot
// (and into LDS); thread 0 adds the sums of each round of 1024 tensors from LDS in table order and writes the four stats.
// tensor_sum == NULL: there are no chunks and every sum is zero.  A list that is not in table order gives ranges that are wrong
// but inside the list: the sums are then meaningless, nothing is read out of bounds.
constexpr int kFinalThreads = 1024;
constexpr int kInFlight = 16;

__global__ __launch_bounds__(kFinalThreads) void grad_norm_final_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors,
                                                                        const gava_adamw_chunk* __restrict__ chunks, int n_chunks,
                                                                        const double* __restrict__ partial, double* tensor_sum,
                                                                        double max_norm, float* __restrict__ tensor_norm,
                                                                        float* __restrict__ stats) {
  __shared__ double sum_s[kFinalThreads];
  static_assert(sizeof(int2) == sizeof(double), "a tensor's chunk range lives in its sum's slot until the sum is known");
  int2* range = reinterpret_cast<int2*>(tensor_sum);
  const int tid = threadIdx.x;
  if (tensor_sum) {
    for (int i = tid; i < n_tensors; i += kFinalThreads) range[i] = make_int2(0, 0);
    __syncthreads();
    for (int c = tid; c < n_chunks; c += kFinalThreads) {
      const int t = chunks[c].tensor;
      if ((unsigned)t >= (unsigned)n_tensors) continue;
      if (c == 0 || chunks[c - 1].tensor != t) range[t].x = c;
      if (c == n_chunks - 1 || chunks[c + 1].tensor != t) range[t].y = c + 1;
    }
    __syncthreads();
  }
  double total = 0.0;   // thread 0's
  for (int base = 0; base < n_tensors; base += kFinalThreads) {   // uniform
    const int i = base + tid;
    double s = 0.0;
    if (i < n_tensors) {
      if (tensor_sum) {
        const int2 r = range[i];
        if (table[i].g) {
          int c = r.x;
          for (; c + kInFlight <= r.y; c += kInFlight) {
            double v[kInFlight];
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) v[j] = partial[c + j];
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) s += v[j];
          }
          for (; c < r.y; ++c) s += partial[c];
        }
        tensor_sum[i] = s;
      }
      if (tensor_norm) tensor_norm[i] = (float)sqrt(s);
    }
    sum_s[tid] = s;
    __syncthreads();
    if (tid == 0) {
      const int cnt = n_tensors - base < kFinalThreads ? n_tensors - base : kFinalThreads;
      for (int j = 0; j < cnt; ++j) total += sum_s[j];
    }
    __syncthreads();
  }
  if (tid == 0 && stats) {
    const double norm = sqrt(total);
    const bool bad = !isfinite(total);   // an inf or a NaN anywhere
    stats[0] = (float)norm;
    stats[1] = bad ? 1.0f : (float)fmin(1.0, max_norm / (norm + 1e-6));
    stats[2] = bad ? 1.0f : 0.0f;
    stats[3] = 0.0f;
  }
}

bool valid_tensor(const gava_adamw_tensor& t, int n_groups) {
  if (!t.g) return true;   // skipped entirely
  if (!t.p || !t.m || !t.v || !t.step || t.n < 0) return false;
  if (t.group < 0 || t.group >= n_groups) return false;
  if (t.copy16 && t.prec16 != GAVA_PREC_F16 && t.prec16 != GAVA_PREC_BF16) return false;
  if (t.copy_f32 || t.copy16 || t.copy_bf16 || t.copy_bf16_t) {
    if (t.rows < 0 || t.cols < 0 || (int64_t)t.rows * t.cols != t.n) return false;
    if ((t.copy_f32 && t.ld_f32 < t.cols) || (t.copy16 && t.ld16 < t.cols) || (t.copy_bf16 && t.ld_bf16 < t.cols) ||
        (t.copy_bf16_t && t.ld_bf16_t < t.rows))
      return false;
  }
  return true;
}

bool valid_table(const gava_adamw_tensor* table, int n_tensors, int n_groups) {
  if (n_tensors < 0 || n_groups < 1 || n_groups > GAVA_ADAMW_MAX_GROUPS || (n_tensors > 0 && !table)) return false;
  for (int i = 0; i < n_tensors; ++i)
    if (!valid_tensor(table[i], n_groups)) return false;
  return true;
}

}  // namespace

extern "C" int gava_adamw_plan(const gava_adamw_tensor* table_host, int n_tensors, int n_groups, gava_adamw_chunk* out, int cap) {
  if (!valid_table(table_host, n_tensors, n_groups) || cap < 0 || (cap > 0 && !out)) return GAVA_EINVAL;
  long count = 0;
  auto emit = [&](int tensor, int a, int b) {
    if (count < cap) out[count] = gava_adamw_chunk{tensor, a, b, 0};
    ++count;
  };
  for (int i = 0; i < n_tensors; ++i) {
    const gava_adamw_tensor& t = table_host[i];
    if (!t.g || t.n == 0) continue;
    if (t.copy_bf16_t) {
      for (int r = 0; r < t.rows; r += kTile)
        for (int c = 0; c < t.cols; c += kTile) emit(i, r, c);
    } else {
      for (long e = 0; e < t.n; e += kChunk) emit(i, (int)e, (int)(t.n - e < kChunk ? t.n - e : kChunk));
    }
  }
  return count > 0x7fffffffL ? GAVA_EINVAL : (int)count;
}

namespace {

// clip_stats == NULL: the plain step
int adamw_step(const gava_adamw_args* a, const float* clip_stats, gava_stream_t stream) {
  if (!a) return GAVA_EINVAL;
  if (a->n_tensors > 0 && !a->table) return GAVA_EINVAL;
  if (!valid_table(a->table_host, a->n_tensors, a->n_groups)) return GAVA_EINVAL;
  if (a->n_chunks < 0 || (a->n_chunks > 0 && !a->chunks)) return GAVA_EINVAL;
  if (a->n_tensors == 0) return GAVA_OK;
  hipStream_t s = (hipStream_t)stream;
  if (a->n_chunks > 0) {
    Groups groups;
    for (int i = 0; i < GAVA_ADAMW_MAX_GROUPS; ++i) groups.g[i] = a->groups[i];
    if (clip_stats)
      hipLaunchKernelGGL(adamw_kernel<true>, dim3(a->n_chunks), dim3(kThreads), 0, s, a->table, a->n_tensors, a->chunks, groups,
                         a->n_groups, a->grad_scale, a->found_inf, clip_stats);
    else
      hipLaunchKernelGGL(adamw_kernel<false>, dim3(a->n_chunks), dim3(kThreads), 0, s, a->table, a->n_tensors, a->chunks, groups,
                         a->n_groups, a->grad_scale, a->found_inf, clip_stats);
    GAVA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(adamw_count_kernel, dim3((a->n_tensors + 255) / 256), dim3(256), 0, s, a->table, a->n_tensors, a->found_inf,
                     clip_stats);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

}  // namespace

extern "C" int gava_adamw_step(const gava_adamw_args* a, gava_stream_t stream) { return adamw_step(a, nullptr, stream); }

extern "C" int gava_adamw_step_clipped(const gava_adamw_args* a, const float* stats, gava_stream_t stream) {
  if (!stats) return GAVA_EINVAL;
  return adamw_step(a, stats, stream);
}

extern "C" int gava_grad_norm(const gava_grad_norm_args* a, gava_stream_t stream) {
  if (!a) return GAVA_EINVAL;
  if (a->n_tensors > 0 && !a->table) return GAVA_EINVAL;
  if (!valid_table(a->table_host, a->n_tensors, a->n_groups)) return GAVA_EINVAL;
  if (!(a->max_norm > 0.0)) return GAVA_EINVAL;   // zero, negative, NaN
  if (a->n_chunks < 0 || (a->n_chunks > 0 && (!a->chunks || !a->stats || !a->workspace))) return GAVA_EINVAL;
  if ((uintptr_t)a->workspace % sizeof(double) || (uintptr_t)a->stats % sizeof(float) || (uintptr_t)a->tensor_norm % sizeof(float))
    return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  double* partial = a->n_chunks > 0 ? (double*)a->workspace : nullptr;
  if (a->n_chunks > 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(a->n_chunks), dim3(kThreads), 0, s, a->table, a->n_tensors, a->chunks, a->grad_scale,
                       partial);
    GAVA_CHECK_LAUNCH();
  }
  if (a->stats || (a->tensor_norm && a->n_tensors > 0)) {
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, a->table, a->n_tensors, a->chunks, a->n_chunks,
                       partial, partial ? partial + a->n_chunks : nullptr, a->max_norm, a->tensor_norm, a->stats);
    GAVA_CHECK_LAUNCH();
  }
  return GAVA_OK;
}

extern "C" int gava_grad_clip_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_grad_norm_args)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}

extern "C" int gava_optim_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_adamw_tensor), sizeof(gava_adamw_args), sizeof(gava_adamw_chunk)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
