// The last stage of the gradient with respect to the input clip: the fold half of ImagePatchEmbed2D (see gava_unpatchify_args).
// One workgroup per (frame f, patch row gy [, channel c in GRAD mode]): it owns the P image rows gy*P ... gy*P + P - 1 of the
// frame, P * size contiguous floats of an output plane.  A thread takes VEC consecutive pixels of one row - a vector never
// straddles a patch, VEC divides P - so consecutive threads store consecutive addresses (whole rows) and load P-float segments
// of the g patch rows.  HBM-bound: 12 B in per pixel (24 with x), 12 or 4 B out; no LDS, no atomics.
#include "common.h"

namespace {

struct UnpatchParams {
  const float* dpatch; long ld;
  const float* x;
  float* out;
  int T, size, P, g, frame_rows, row_offset;
};

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

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void unpatchify_kernel(const UnpatchParams p) {
  const long f = blockIdx.x;
  const int gy = blockIdx.y;
  const long b = f / p.T, t = f - b * p.T;
  const int n_vec = p.P * p.size / VEC, PP = p.P * p.P;
  const long plane = (long)p.size * p.size, rows0 = (long)gy * p.P * p.size;
  // first patch row of this workgroup: row (f, gy*g) of dpatch
  const float* src = p.dpatch + (f * p.frame_rows + p.row_offset + (long)gy * p.g) * p.ld;
  for (int i = threadIdx.x; i < n_vec; i += 256) {
    const int e0 = i * VEC, iy = e0 / p.size, x0 = e0 - iy * p.size;
    const int px = x0 / p.P, ix = x0 - px * p.P;
    const float* s = src + (long)px * p.ld + iy * p.P + ix;
    if constexpr (MODE == GAVA_UNPATCH_GRAD) {
      const int c = blockIdx.z;
      store<VEC>(p.out + ((b * 3 + c) * p.T + t) * plane + rows0 + e0, load<VEC>(s + c * PP));
    } else {
      const Vec<VEC> g0 = load<VEC>(s), g1 = load<VEC>(s + PP), g2 = load<VEC>(s + 2 * PP);
      Vec<VEC> r;
      if constexpr (MODE == GAVA_UNPATCH_ABSMAX) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) r.v[e] = fmaxf(fmaxf(fabsf(g0.v[e]), fabsf(g1.v[e])), fabsf(g2.v[e]));
      } else if constexpr (MODE == GAVA_UNPATCH_L2) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          r.v[e] = __fsqrt_rn(__fmaf_rn(g2.v[e], g2.v[e], __fmaf_rn(g1.v[e], g1.v[e], g0.v[e] * g0.v[e])));
      } else {
        const float* xs = p.x + (b * 3 * p.T + t) * plane + rows0 + e0;      // channel 0; channels are T planes apart
        const Vec<VEC> x0v = load<VEC>(xs), x1v = load<VEC>(xs + p.T * plane), x2v = load<VEC>(xs + 2 * p.T * plane);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          r.v[e] = __fmaf_rn(g2.v[e], x2v.v[e], __fmaf_rn(g1.v[e], x1v.v[e], g0.v[e] * x0v.v[e]));
      }
      store<VEC>(p.out + f * plane + rows0 + e0, r);
    }
  }
}

template <int MODE>
void launch(const UnpatchParams& p, int vec, dim3 grid, hipStream_t s) {
  if (vec == 4) hipLaunchKernelGGL((unpatchify_kernel<MODE, 4>), grid, dim3(256), 0, s, p);
  else if (vec == 2) hipLaunchKernelGGL((unpatchify_kernel<MODE, 2>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((unpatchify_kernel<MODE, 1>), grid, dim3(256), 0, s, p);
}

}  // namespace

extern "C" int gava_unpatchify(const gava_unpatchify_args* a, gava_stream_t stream) {
  if (!a || !a->dpatch || !a->out) return GAVA_EINVAL;
  if (a->mode < GAVA_UNPATCH_GRAD || a->mode > GAVA_UNPATCH_GRAD_X_INPUT) return GAVA_EINVAL;
  if ((a->mode == GAVA_UNPATCH_GRAD_X_INPUT) != (a->x != nullptr)) return GAVA_EINVAL;
  if (((uintptr_t)a->dpatch | (uintptr_t)a->out | (uintptr_t)a->x) & 15) return GAVA_EINVAL;
  if (a->B <= 0 || a->T <= 0 || a->size <= 0 || a->patch <= 0 || a->size % a->patch) return GAVA_EINVAL;
  if ((long)a->B * a->T > 0x7fffffffL) return GAVA_EINVAL;
  const long g = a->size / a->patch, n = g * g;
  if (g > 65535 || a->ld < 3L * a->patch * a->patch) return GAVA_EINVAL;
  if (a->row_offset < 0 || a->row_offset + n > a->frame_rows) return GAVA_EINVAL;
  UnpatchParams p;
  p.dpatch = a->dpatch; p.ld = a->ld; p.x = a->x; p.out = a->out;
  p.T = a->T; p.size = a->size; p.P = a->patch; p.g = (int)g; p.frame_rows = a->frame_rows; p.row_offset = a->row_offset;
  // every address is base + a multiple of (ld, P) floats: the vector width follows from those two (the bases are 16-byte aligned)
  const int vec = (a->patch % 4 == 0 && a->ld % 4 == 0) ? 4 : (a->patch % 2 == 0 && a->ld % 2 == 0) ? 2 : 1;
  dim3 grid((unsigned)((long)a->B * a->T), (unsigned)g, a->mode == GAVA_UNPATCH_GRAD ? 3 : 1);
  hipStream_t s = (hipStream_t)stream;
  switch (a->mode) {
    case GAVA_UNPATCH_GRAD: launch<GAVA_UNPATCH_GRAD>(p, vec, grid, s); break;
    case GAVA_UNPATCH_ABSMAX: launch<GAVA_UNPATCH_ABSMAX>(p, vec, grid, s); break;
    case GAVA_UNPATCH_L2: launch<GAVA_UNPATCH_L2>(p, vec, grid, s); break;
    default: launch<GAVA_UNPATCH_GRAD_X_INPUT>(p, vec, grid, s); break;
  }
  if (hipGetLastError() != hipSuccess) return GAVA_ELAUNCH;
  return GAVA_OK;
}

extern "C" int gava_input_grad_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_unpatchify_args)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
