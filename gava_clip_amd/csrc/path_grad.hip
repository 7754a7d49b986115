// path_grad.hip — integrated gradients and SmoothGrad: m gradients of near-copies of a clip, reduced to one map (see the
// "path gradients" section of gava_hip.h).  gava_path_clips writes the m copies (the straight line from a baseline, or the clip
// plus counter-based Gaussian noise), gava_clip_range gives the noise its scale, gava_unpatchify_path is gava_unpatchify with
// the weighted sum over the m copies folded in - the m gradients are never in memory - and gava_path_delta is the completeness
// residual of integrated gradients.  All HBM-bound passes: no atomics, fixed summation orders, 64-bit offsets.
#include "common.h"

namespace {

// (Vec / load / store are input_grad.hip's, restated: that file is not this change's to touch; they belong in common.h.)
template <int VEC>
struct Vec {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> load(const float* p) {
  Vec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else if constexpr (VEC == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    r.v[0] = q.x; r.v[1] = q.y;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void store(float* p, const Vec<VEC>& r) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else if constexpr (VEC == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  else *p = r.v[0];
}

// ---- the copies --------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): ten rounds, the key bumped between them.
struct Philox {
  unsigned c[4];
};

static __device__ __forceinline__ Philox philox4x32_10(Philox ctr, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, ctr.c[0]), lo0 = 0xD2511F53u * ctr.c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, ctr.c[2]), lo1 = 0xCD9E8D57u * ctr.c[2];
    ctr.c[0] = hi1 ^ ctr.c[1] ^ k0; ctr.c[1] = lo1;
    ctr.c[2] = hi0 ^ ctr.c[3] ^ k1; ctr.c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return ctr;
}

// two words -> two standard normals (Box-Muller on exact 24-bit uniforms; u1 in (0, 1], u2 in [0, 1))
static __device__ __forceinline__ void box_muller(unsigned ra, unsigned rb, float& za, float& zb) {
  const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f, u2 = (float)(rb >> 8) * 0x1p-24f;
  const float radius = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  za = radius * cs; zb = radius * sn;
}

struct PathClipsParams {
  const float* x; const float* baseline; const float* sigma; float* out;
  long items;            // nb * 3 * T * size * size / VEC
  int T, size, kind, m, clip0;
  unsigned seed_lo, seed_hi;
  float alpha[GAVA_PATH_MAX_STEPS], beta[GAVA_PATH_MAX_STEPS];
};

constexpr int PC_THREADS = 256;

// A work item is VEC consecutive floats of a clip: read x (and the baseline, or sigma) once, write the m copies.
// Noise: a Philox block serves a group of four floats, so VEC = 4 draws it once per group, VEC = 2 (P = 14) twice - each item
// its own Box-Muller pair - and VEC = 1 (an odd patch with an even size) four times, with a pair of which one value is used:
// four times the generator work at a shape no model here has, accepted for one code path.
template <int VEC, bool NOISE>
__global__ __launch_bounds__(PC_THREADS) void path_clips_kernel(const PathClipsParams p) {
  const long plane = (long)p.size * p.size;
  const long clip = 3 * (long)p.T * plane;                 // floats per clip
  const long clip_items = clip / VEC;
  const long stride = (long)gridDim.x * PC_THREADS;
  for (long it = (long)blockIdx.x * PC_THREADS + threadIdx.x; it < p.items; it += stride) {
    const long b = it / clip_items;
    const long e = (it - b * clip_items) * VEC;            // float offset inside the clip
    const Vec<VEC> xv = load<VEC>(p.x + b * clip + e);
    float* dst = p.out + b * p.m * clip + e;
    if constexpr (NOISE) {
      const float sg = p.sigma[b];
      const unsigned long long e4 = (unsigned long long)e >> 2;       // the group of four floats this item lies in
      const int first = (int)(e & 3);
      for (int k = 0; k < p.m; ++k) {
        Philox ctr;
        ctr.c[0] = (unsigned)e4; ctr.c[1] = (unsigned)(e4 >> 32); ctr.c[2] = (unsigned)k; ctr.c[3] = (unsigned)(p.clip0 + (int)b);
        const Philox r = philox4x32_10(ctr, p.seed_lo, p.seed_hi);
        float z[4];
        if (VEC == 4 || first < 2) box_muller(r.c[0], r.c[1], z[0], z[1]);
        if (VEC == 4 || first >= 2) box_muller(r.c[2], r.c[3], z[2], z[3]);
        Vec<VEC> o;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o.v[j] = __fmaf_rn(sg, VEC == 4 ? z[j] : z[first + j], xv.v[j]);
        store<VEC>(dst + k * clip, o);
      }
    } else {
      Vec<VEC> bv;
      if (p.kind == GAVA_BASELINE_TENSOR) {
        bv = load<VEC>(p.baseline + b * clip + e);
      } else {
        const float word = p.kind == GAVA_BASELINE_CHANNEL ? p.baseline[e / ((long)p.T * plane)] : 0.0f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) bv.v[j] = word;
      }
      for (int k = 0; k < p.m; ++k) {
        const float al = p.alpha[k], be = p.beta[k];
        Vec<VEC> o;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o.v[j] = __fmaf_rn(al, xv.v[j], __fmul_rn(be, bv.v[j]));
        store<VEC>(dst + k * clip, o);
      }
    }
  }
}

template <int VEC>
void launch_path_clips(const PathClipsParams& p, bool noise, hipStream_t s) {
  const long blocks = (p.items + PC_THREADS - 1) / PC_THREADS;
  const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
  if (noise) hipLaunchKernelGGL((path_clips_kernel<VEC, true>), grid, dim3(PC_THREADS), 0, s, p);
  else hipLaunchKernelGGL((path_clips_kernel<VEC, false>), grid, dim3(PC_THREADS), 0, s, p);
}

// ---- range -------------------------------------------------------------------------------------------------------------
// min / max that keep a NaN: any NaN in a clip makes both results NaN, in whatever order the tree runs.
static __device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : b != b ? b : fminf(a, b); }
static __device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }

constexpr int CR_THREADS = 256;

// -> (min, max) of the workgroup's values in thread 0
static __device__ __forceinline__ void block_min_max(float& lo, float& hi) {
  __shared__ float s_lo[CR_THREADS / 64], s_hi[CR_THREADS / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = nan_min(lo, __shfl_xor(lo, o, 64));
    hi = nan_max(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < CR_THREADS / 64; ++w) { lo = nan_min(lo, s_lo[w]); hi = nan_max(hi, s_hi[w]); }
  }
}

// launch 1: workgroup (part, b) reduces its share of clip b into partial[b][part][0..1]
template <int VEC>
__global__ __launch_bounds__(CR_THREADS) void clip_range_parts_kernel(const float* __restrict__ x, float* __restrict__ partial, long clip) {
  const long b = blockIdx.y;
  const float* src = x + b * clip;
  float lo = INFINITY, hi = -INFINITY;
  const long items = clip / VEC, stride = (long)gridDim.x * CR_THREADS;
  for (long it = (long)blockIdx.x * CR_THREADS + threadIdx.x; it < items; it += stride) {
    const Vec<VEC> v = load<VEC>(src + it * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) { lo = nan_min(lo, v.v[j]); hi = nan_max(hi, v.v[j]); }
  }
  block_min_max(lo, hi);
  if (threadIdx.x == 0) {
    float* dst = partial + (b * gridDim.x + blockIdx.x) * 2;
    dst[0] = lo; dst[1] = hi;
  }
}

// launch 2: one workgroup per clip over its parts
__global__ __launch_bounds__(CR_THREADS) void clip_range_final_kernel(const float* __restrict__ partial, int parts, float rel,
                                                                      float* __restrict__ mn, float* __restrict__ mx,
                                                                      float* __restrict__ sigma) {
  const long b = blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < parts; i += CR_THREADS) {
    lo = nan_min(lo, partial[(b * parts + i) * 2]);
    hi = nan_max(hi, partial[(b * parts + i) * 2 + 1]);
  }
  block_min_max(lo, hi);
  if (threadIdx.x == 0) {
    mn[b] = lo; mx[b] = hi;
    sigma[b] = __fmul_rn(rel, __fsub_rn(hi, lo));
  }
}

// ---- the accumulating fold -----------------------------------------------------------------------------------------------
struct PathFoldParams {
  const float* dpatch; long ld;
  const float* x; const float* baseline;
  float* out;
  int T, size, P, g, frame_rows, row_offset, kind, m;
  float w[GAVA_PATH_MAX_STEPS];
};

template <int MODE>
constexpr bool per_channel() { return MODE == GAVA_PATH_GRAD || MODE == GAVA_PATH_ATTR; }
template <int MODE>
constexpr bool attribution() { return MODE == GAVA_PATH_ATTR || MODE == GAVA_PATH_ATTR_SUM || MODE == GAVA_PATH_ATTR_ABS; }

// One workgroup per (frame f of the OUTPUT, patch row gy [, channel c in the per-channel modes]), the geometry of
// unpatchify_kernel; the frame's gradient is the chain G = fma(w[k], g(b*m + k), G) over the m copies of its clip.
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void unpatchify_path_kernel(const PathFoldParams p) {
  constexpr int NC = per_channel<MODE>() ? 1 : 3;
  const long f = blockIdx.x;
  const int gy = blockIdx.y;
  const long b = f / p.T, t = f - b * p.T;
  const int n_vec = p.P * p.size / VEC, PP = p.P * p.P;
  const int c0 = per_channel<MODE>() ? (int)blockIdx.z : 0;
  const long plane = (long)p.size * p.size, rows0 = (long)gy * p.P * p.size;
  const long copy_rows = (long)p.T * p.frame_rows * p.ld;                    // floats between two copies' frame t
  // first patch row of this workgroup in copy 0 of clip b: row (b*m*T + t, gy*g) of dpatch
  const float* src = p.dpatch + ((b * p.m * p.T + t) * p.frame_rows + p.row_offset + (long)gy * p.g) * p.ld + c0 * PP;
  for (int i = threadIdx.x; i < n_vec; i += 256) {
    const int e0 = i * VEC, iy = e0 / p.size, x0 = e0 - iy * p.size;
    const int px = x0 / p.P, ix = x0 - px * p.P;
    const float* s = src + (long)px * p.ld + iy * p.P + ix;
    Vec<VEC> G[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < VEC; ++e) G[c].v[e] = 0.0f;
    for (int k = 0; k < p.m; ++k) {
      const float wk = p.w[k];
      if (wk == 0.0f) continue;                            // uniform over the launch
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const Vec<VEC> gv = load<VEC>(s + k * copy_rows + c * PP);
#pragma unroll
        for (int e = 0; e < VEC; ++e) G[c].v[e] = __fmaf_rn(wk, gv.v[e], G[c].v[e]);
      }
    }
    if constexpr (attribution<MODE>()) {                   // G_c <- a_c = (x_c - x0_c) * G_c
      const long chan = (long)p.T * plane;
      const long at = (b * 3 * p.T + t) * plane + rows0 + e0;                // channel 0
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int cc = c0 + c;
        const Vec<VEC> xv = load<VEC>(p.x + at + cc * chan);
        Vec<VEC> bv;
        if (p.kind == GAVA_BASELINE_TENSOR) {
          bv = load<VEC>(p.baseline + at + cc * chan);
        } else {
          const float word = p.kind == GAVA_BASELINE_CHANNEL ? p.baseline[cc] : 0.0f;
#pragma unroll
          for (int e = 0; e < VEC; ++e) bv.v[e] = word;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) G[c].v[e] = __fmul_rn(__fsub_rn(xv.v[e], bv.v[e]), G[c].v[e]);
      }
    }
    if constexpr (per_channel<MODE>()) {
      store<VEC>(p.out + ((b * 3 + c0) * p.T + t) * plane + rows0 + e0, G[0]);
    } else {
      Vec<VEC> r;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float a0 = G[0].v[e], a1 = G[NC - 2].v[e], a2 = G[NC - 1].v[e];
        if constexpr (MODE == GAVA_PATH_ABSMAX) r.v[e] = fmaxf(fmaxf(fabsf(a0), fabsf(a1)), fabsf(a2));
        else if constexpr (MODE == GAVA_PATH_L2) r.v[e] = __fsqrt_rn(__fmaf_rn(a2, a2, __fmaf_rn(a1, a1, a0 * a0)));
        else if constexpr (MODE == GAVA_PATH_ATTR_SUM) r.v[e] = __fadd_rn(__fadd_rn(a0, a1), a2);
        else r.v[e] = __fadd_rn(__fadd_rn(fabsf(a0), fabsf(a1)), fabsf(a2));
      }
      store<VEC>(p.out + f * plane + rows0 + e0, r);
    }
  }
}

template <int MODE>
void launch_fold(const PathFoldParams& p, int vec, dim3 grid, hipStream_t s) {
  if (vec == 4) hipLaunchKernelGGL((unpatchify_path_kernel<MODE, 4>), grid, dim3(256), 0, s, p);
  else if (vec == 2) hipLaunchKernelGGL((unpatchify_path_kernel<MODE, 2>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((unpatchify_path_kernel<MODE, 1>), grid, dim3(256), 0, s, p);
}

// ---- the completeness residual -------------------------------------------------------------------------------------------
constexpr int PD_THREADS = 256;

struct PathDeltaParams {
  const float* map; const float* logits; long ld; const long long* target;
  float* sum_attr; float* f_diff; float* delta;
  long n;                // T * size * size
  int m, C, k_lo, k_hi;
};

__global__ __launch_bounds__(PD_THREADS) void path_delta_kernel(const PathDeltaParams p) {
  __shared__ double part[PD_THREADS / 64];
  const long b = blockIdx.x;
  const float* a = p.map + b * p.n;
  double acc = 0.0;
  for (long i = threadIdx.x; i < p.n; i += PD_THREADS) acc += (double)a[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = part[0];
    for (int w = 1; w < PD_THREADS / 64; ++w) total += part[w];
    const long long tg = p.target[b];
    const float nan = __builtin_nanf("");
    float sum = nan, diff = nan, d = nan;
    if (tg >= 0 && tg < p.C) {
      const float* rows = p.logits + b * p.m * p.ld;
      sum = (float)total;
      diff = __fsub_rn(rows[p.k_hi * p.ld + tg], rows[p.k_lo * p.ld + tg]);
      d = __fsub_rn(sum, diff);
    }
    p.sum_attr[b] = sum; p.f_diff[b] = diff; p.delta[b] = d;
  }
}

bool known_kind(int kind) { return kind == GAVA_BASELINE_ZERO || kind == GAVA_BASELINE_CHANNEL || kind == GAVA_BASELINE_TENSOR; }

}  // namespace

extern "C" int gava_path_clips(const gava_path_clips_args* a, gava_stream_t stream) {
  if (!a || !a->x || !a->out) return GAVA_EINVAL;
  if (a->nb < 1 || a->T < 1 || a->size < 1 || a->patch < 1 || a->size % a->patch) return GAVA_EINVAL;
  if (a->m < 1 || a->m > GAVA_PATH_MAX_STEPS) return GAVA_EINVAL;
  if (a->mode != GAVA_PATH_LINE && a->mode != GAVA_PATH_NOISE) return GAVA_EINVAL;
  if (((uintptr_t)a->x | (uintptr_t)a->out) & 15) return GAVA_EINVAL;
  const bool noise = a->mode == GAVA_PATH_NOISE;
  if (noise) {
    if (!a->sigma || ((uintptr_t)a->sigma & 3) || a->baseline || a->baseline_kind != GAVA_BASELINE_ZERO) return GAVA_EINVAL;
    if (a->size % 2 || a->clip0 < 0 || (long)a->clip0 + a->nb > 0x7fffffffL) return GAVA_EINVAL;
  } else {
    if (a->sigma || !known_kind(a->baseline_kind)) return GAVA_EINVAL;
    if ((a->baseline_kind == GAVA_BASELINE_ZERO) != (a->baseline == nullptr)) return GAVA_EINVAL;
    if ((uintptr_t)a->baseline & (a->baseline_kind == GAVA_BASELINE_TENSOR ? 15 : 3)) return GAVA_EINVAL;
    for (int k = 0; k < a->m; ++k)
      if (!(a->alpha[k] >= 0.0f && a->alpha[k] <= 1.0f) || !(a->beta[k] >= 0.0f && a->beta[k] <= 1.0f)) return GAVA_EINVAL;
  }
  PathClipsParams p;
  p.x = a->x; p.baseline = a->baseline; p.sigma = a->sigma; p.out = a->out;
  p.T = a->T; p.size = a->size; p.kind = a->baseline_kind; p.m = a->m; p.clip0 = a->clip0;
  p.seed_lo = (unsigned)(a->seed & 0xffffffffu); p.seed_hi = (unsigned)(a->seed >> 32);
  for (int k = 0; k < GAVA_PATH_MAX_STEPS; ++k) {
    p.alpha[k] = (!noise && k < a->m) ? a->alpha[k] : 0.0f;
    p.beta[k] = (!noise && k < a->m) ? a->beta[k] : 0.0f;
  }
  const long floats = 3L * a->nb * a->T * a->size * a->size;
  // every row (size floats) starts on a vector boundary when VEC | patch; a noise group of four is then whole vectors
  const int vec = a->patch % 4 == 0 ? 4 : a->patch % 2 == 0 ? 2 : 1;
  p.items = floats / vec;
  hipStream_t s = (hipStream_t)stream;
  if (vec == 4) launch_path_clips<4>(p, noise, s);
  else if (vec == 2) launch_path_clips<2>(p, noise, s);
  else launch_path_clips<1>(p, noise, s);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_clip_range(const gava_clip_range_args* a, gava_stream_t stream) {
  if (!a || !a->x || !a->min || !a->max || !a->sigma || !a->workspace) return GAVA_EINVAL;
  if (a->nb < 1 || a->nb > 65535 || a->T < 1 || a->size < 1) return GAVA_EINVAL;
  if (((uintptr_t)a->x | (uintptr_t)a->min | (uintptr_t)a->max | (uintptr_t)a->sigma | (uintptr_t)a->workspace) & 3) return GAVA_EINVAL;
  const long clip = 3L * a->T * a->size * a->size;
  const bool wide = clip % 4 == 0 && ((uintptr_t)a->x & 15) == 0;
  const dim3 grid(GAVA_CLIP_RANGE_PARTS, (unsigned)a->nb);
  hipStream_t s = (hipStream_t)stream;
  if (wide) hipLaunchKernelGGL((clip_range_parts_kernel<4>), grid, dim3(CR_THREADS), 0, s, a->x, a->workspace, clip);
  else hipLaunchKernelGGL((clip_range_parts_kernel<1>), grid, dim3(CR_THREADS), 0, s, a->x, a->workspace, clip);
  GAVA_CHECK_LAUNCH();
  hipLaunchKernelGGL(clip_range_final_kernel, dim3((unsigned)a->nb), dim3(CR_THREADS), 0, s, (const float*)a->workspace, GAVA_CLIP_RANGE_PARTS,
                     a->rel, a->min, a->max, a->sigma);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_unpatchify_path(const gava_unpatchify_path_args* a, gava_stream_t stream) {
  if (!a || !a->dpatch || !a->out) return GAVA_EINVAL;
  if (a->mode < GAVA_PATH_GRAD || a->mode > GAVA_PATH_ATTR_ABS || !known_kind(a->baseline_kind)) return GAVA_EINVAL;
  const bool attr = a->mode >= GAVA_PATH_ATTR;
  if (attr != (a->x != nullptr)) return GAVA_EINVAL;
  if (!attr && (a->baseline || a->baseline_kind != GAVA_BASELINE_ZERO)) return GAVA_EINVAL;
  if ((a->baseline_kind == GAVA_BASELINE_ZERO) != (a->baseline == nullptr)) return GAVA_EINVAL;
  if (((uintptr_t)a->dpatch | (uintptr_t)a->out | (uintptr_t)a->x) & 15) return GAVA_EINVAL;
  if ((uintptr_t)a->baseline & (a->baseline_kind == GAVA_BASELINE_TENSOR ? 15 : 3)) return GAVA_EINVAL;
  if (a->B <= 0 || a->T <= 0 || a->size <= 0 || a->patch <= 0 || a->size % a->patch) return GAVA_EINVAL;
  if (a->m < 1 || a->m > GAVA_PATH_MAX_STEPS) return GAVA_EINVAL;
  if ((long)a->B * a->T * a->m > 0x7fffffffL) return GAVA_EINVAL;
  const long g = a->size / a->patch, n = g * g;
  if (g > 65535 || a->ld < 3L * a->patch * a->patch) return GAVA_EINVAL;
  if (a->row_offset < 0 || a->row_offset + n > a->frame_rows) return GAVA_EINVAL;
  for (int k = 0; k < a->m; ++k)
    if (!(a->w[k] - a->w[k] == 0.0f)) return GAVA_EINVAL;                 // a weight that is not finite
  PathFoldParams p;
  p.dpatch = a->dpatch; p.ld = a->ld; p.x = a->x; p.baseline = a->baseline; p.out = a->out;
  p.T = a->T; p.size = a->size; p.P = a->patch; p.g = (int)g; p.frame_rows = a->frame_rows; p.row_offset = a->row_offset;
  p.kind = a->baseline_kind; p.m = a->m;
  for (int k = 0; k < GAVA_PATH_MAX_STEPS; ++k) p.w[k] = k < a->m ? a->w[k] : 0.0f;
  // every address is base + a multiple of (ld, P) floats: the vector width follows from those two (the bases are 16-byte aligned)
  const int vec = (a->patch % 4 == 0 && a->ld % 4 == 0) ? 4 : (a->patch % 2 == 0 && a->ld % 2 == 0) ? 2 : 1;
  const bool chan = a->mode == GAVA_PATH_GRAD || a->mode == GAVA_PATH_ATTR;
  dim3 grid((unsigned)((long)a->B * a->T), (unsigned)g, chan ? 3 : 1);
  hipStream_t s = (hipStream_t)stream;
  switch (a->mode) {
    case GAVA_PATH_GRAD: launch_fold<GAVA_PATH_GRAD>(p, vec, grid, s); break;
    case GAVA_PATH_ABSMAX: launch_fold<GAVA_PATH_ABSMAX>(p, vec, grid, s); break;
    case GAVA_PATH_L2: launch_fold<GAVA_PATH_L2>(p, vec, grid, s); break;
    case GAVA_PATH_ATTR: launch_fold<GAVA_PATH_ATTR>(p, vec, grid, s); break;
    case GAVA_PATH_ATTR_SUM: launch_fold<GAVA_PATH_ATTR_SUM>(p, vec, grid, s); break;
    default: launch_fold<GAVA_PATH_ATTR_ABS>(p, vec, grid, s); break;
  }
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_path_delta(const gava_path_delta_args* a, gava_stream_t stream) {
  if (!a || !a->map || !a->logits || !a->target || !a->sum_attr || !a->f_diff || !a->delta) return GAVA_EINVAL;
  if (a->B < 1 || a->T < 1 || a->size < 1 || a->C < 1 || a->ld < a->C) return GAVA_EINVAL;
  if (a->m < 1 || a->m > GAVA_PATH_MAX_STEPS || a->k_lo < 0 || a->k_lo >= a->m || a->k_hi < 0 || a->k_hi >= a->m) return GAVA_EINVAL;
  if (((uintptr_t)a->map | (uintptr_t)a->logits | (uintptr_t)a->sum_attr | (uintptr_t)a->f_diff | (uintptr_t)a->delta) & 3) return GAVA_EINVAL;
  if ((uintptr_t)a->target & 7) return GAVA_EINVAL;
  PathDeltaParams p;
  p.map = a->map; p.logits = a->logits; p.ld = (long)a->ld; p.target = (const long long*)a->target;
  p.sum_attr = a->sum_attr; p.f_diff = a->f_diff; p.delta = a->delta;
  p.n = (long)a->T * a->size * a->size; p.m = a->m; p.C = a->C; p.k_lo = a->k_lo; p.k_hi = a->k_hi;
  hipLaunchKernelGGL(path_delta_kernel, dim3((unsigned)a->B), dim3(PD_THREADS), 0, (hipStream_t)stream, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_path_grad_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_path_clips_args), sizeof(gava_clip_range_args), sizeof(gava_unpatchify_path_args),
                          sizeof(gava_path_delta_args)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
