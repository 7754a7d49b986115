// optimizer.hip — fused multi-tensor AdamW step that also refreshes the 16-bit weight copies (gava_adamw_step).
//
// One workgroup per chunk of at most 4096 elements of one tensor; a thread owns two groups of 8 consecutive elements.  The
// kernel is a stream over p, g, m, v (in) and p, m, v plus the copies (out): everything is loaded first, the scalar
// coefficients (double precision, thread 0) are computed while the loads fly, and every group moves 16 bytes per lane per
// instruction where its addresses allow.  A tensor with a transposed copy is cut into 64 x 64 tiles instead of linear ranges:
// rows of the tile are read 256 bytes at a time, the bf16 values cross an LDS tile, and columns are written 128 bytes at a time.
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

__global__ __launch_bounds__(kThreads) void adamw_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors,
                                                         const gava_adamw_chunk* __restrict__ chunks, Groups groups, int n_groups,
                                                         const float* __restrict__ grad_scale, const float* __restrict__ found_inf) {
  __shared__ Coef coef_s;
  __shared__ unsigned short tile[kTile][kTile + 2];   // row stride 33 dwords: the column reads of the transposed pass spread over the banks
  if (found_inf && *found_inf != 0.0f) return;        // a skipped step changes nothing (uniform: every workgroup leaves)
  const gava_adamw_chunk ch = chunks[blockIdx.x];
  if ((unsigned)ch.tensor >= (unsigned)n_tensors) return;
  const gava_adamw_tensor t = table[ch.tensor];
  if (!t.g || (unsigned)t.group >= (unsigned)n_groups) return;
  const bool tiled = t.copy_bf16_t != nullptr;
  const bool copies = t.copy_f32 || t.copy16 || t.copy_bf16;
  const int tid = threadIdx.x;

  // where this lane's two groups sit: first element, number of valid elements, and (row, column) of the first one
  int e0[kPasses], cnt[kPasses], row[kPasses], col[kPasses];
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
    c.inv_scale = grad_scale ? 1.0f / *grad_scale : 1.0f;
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

#pragma unroll
  for (int k = 0; k < kPasses; ++k) {
    unsigned short h16[kGroup], hb[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const float gj = g[k][j] * c.inv_scale;
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

__global__ void adamw_count_kernel(const gava_adamw_tensor* __restrict__ table, int n_tensors, const float* __restrict__ found_inf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tensors || (found_inf && *found_inf != 0.0f)) return;
  if (table[i].g) *table[i].step += 1.0f;
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

extern "C" int gava_adamw_step(const gava_adamw_args* a, gava_stream_t stream) {
  if (!a) return GAVA_EINVAL;
  if (a->n_tensors > 0 && !a->table) return GAVA_EINVAL;
  if (!valid_table(a->table_host, a->n_tensors, a->n_groups)) return GAVA_EINVAL;
  if (a->n_chunks < 0 || (a->n_chunks > 0 && !a->chunks)) return GAVA_EINVAL;
  if (a->n_tensors == 0) return GAVA_OK;
  hipStream_t s = (hipStream_t)stream;
  if (a->n_chunks > 0) {
    Groups groups;
    for (int i = 0; i < GAVA_ADAMW_MAX_GROUPS; ++i) groups.g[i] = a->groups[i];
    hipLaunchKernelGGL(adamw_kernel, dim3(a->n_chunks), dim3(kThreads), 0, s, a->table, a->n_tensors, a->chunks, groups,
                       a->n_groups, a->grad_scale, a->found_inf);
    GAVA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(adamw_count_kernel, dim3((a->n_tensors + 255) / 256), dim3(256), 0, s, a->table, a->n_tensors, a->found_inf);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_optim_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_adamw_tensor), sizeof(gava_adamw_args), sizeof(gava_adamw_chunk)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
