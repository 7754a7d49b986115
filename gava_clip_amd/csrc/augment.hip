// augment.hip — the reference's RandAugment step (video_dataset/rand_augment.py under Pillow) on packed uint8 RGB frames: one
// layer of the policy per call, every frame of every clip of the layer in the same launches.  Three kernels: the histograms of
// the frames whose op needs statistics, the 3 x 256 byte table of every table op, and the pixels.  The results are Pillow's,
// byte for byte: fp64 where Python floats or Geometry.c's doubles are at work, fp32 for Image.blend and the SMOOTH filter,
// integers for the tables; integer atomics only.  The formulas are in include/gava_hip.h.
#include "common.h"

// Pillow's CPU builds round every product before the add that follows it; hipcc would fuse them (and has done so differently
// between two kernels before, see cp_mul in clip_pixel.h).  Nothing in this file may contract.
#pragma clang fp contract(off)

namespace {

static __device__ __forceinline__ bool aug_needs_hist(const gava_augment_desc& d) {
  return d.kind == GAVA_AUG_TABLE && d.op >= GAVA_AUG_CONTRAST;
}

// Image.blend(a, b, f): fp32 a + f (b - a); truncated for 0 <= f <= 1 (the value lies between a and b), else clipped, then truncated
static __device__ __forceinline__ unsigned blend_u8(int a, int b, float f, bool inside) {
  float t = (float)a + f * (float)(b - a);
  if (!inside) t = fminf(fmaxf(t, 0.0f), 255.0f);
  return (unsigned)(int)t;
}

// ImageMode conversion RGB -> L
static __device__ __forceinline__ int luma_u8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// The three bytes of pixel p of a frame of npix pixels, in the low 24 bits (R lowest).  One 4-byte access - gfx950 takes global
// accesses at any alignment - wherever its fourth byte is still the frame's; the frame's last pixel byte by byte.
static __device__ __forceinline__ unsigned load_rgb(const uint8_t* frame, int p, int npix) {
  const uint8_t* s = frame + (long)p * 3;
  if (p + 1 < npix) {
    unsigned w;
    __builtin_memcpy(&w, s, 4);
    return w & 0xffffffu;
  }
  return (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
}

static __device__ __forceinline__ int chan(unsigned rgb, int c) { return (int)((rgb >> (8 * c)) & 255u); }

// ---- histograms ---------------------------------------------------------------------------------------------------------------
// grid (x: frame of the layer, y: slabs of the frame).  Every wave counts into LDS histograms of its own (a low-contrast frame
// puts most pixels into a few bins: one shared histogram would serialise on them), the workgroup adds its non-empty bins to the
// frame's slot with integer atomics.  Contrast needs the L histogram only, AutoContrast and Equalize R, G and B only.
__global__ __launch_bounds__(256) void augment_hist_kernel(const gava_augment_desc* desc, unsigned* hist) {
  const gava_augment_desc d = desc[blockIdx.x];
  if (!aug_needs_hist(d)) return;
  __shared__ unsigned h[4][4][256];                    // [wave][R, G, B, L][bin]
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int e = tid; e < 4 * 4 * 256; e += 256) (&h[0][0][0])[e] = 0;
  __syncthreads();
  const int npix = d.H * d.W;
  const bool luma = d.op == GAVA_AUG_CONTRAST;
  for (int p = blockIdx.y * 256 + tid; p < npix; p += gridDim.y * 256) {
    const unsigned v = load_rgb(d.src, p, npix);
    const int r = chan(v, 0), g = chan(v, 1), b = chan(v, 2);
    if (luma) {
      atomicAdd(&h[wave][3][luma_u8(r, g, b)], 1u);
    } else {
      atomicAdd(&h[wave][0][r], 1u);
      atomicAdd(&h[wave][1][g], 1u);
      atomicAdd(&h[wave][2][b], 1u);
    }
  }
  __syncthreads();
  unsigned* out = hist + (long)d.hist_slot * 1024;
  for (int e = tid; e < 1024; e += 256) {
    const unsigned s = (&h[0][0][0])[e] + (&h[1][0][0])[e] + (&h[2][0][0])[e] + (&h[3][0][0])[e];
    if (s) atomicAdd(out + e, s);
  }
}

// ---- tables -------------------------------------------------------------------------------------------------------------------
// One workgroup per frame, thread i owns entry i of the three channel tables.  The statistics ops read the frame's histogram
// slot and leave it zero for the next layer.
__global__ __launch_bounds__(256) void augment_luts_kernel(const gava_augment_desc* desc, unsigned* hist, uint8_t* luts) {
  const gava_augment_desc d = desc[blockIdx.x];
  if (d.kind != GAVA_AUG_TABLE) return;
  __shared__ unsigned h[4][256];
  __shared__ unsigned scan[3][256];
  __shared__ unsigned long long wsum[256], csum[256];
  __shared__ int lo[3], hi[3], nz[3];
  const int i = threadIdx.x;
  uint8_t* out = luts + (long)d.lut_slot * 768;
  const float f = d.factor;
  const bool inside = f >= 0.0f && f <= 1.0f;
  unsigned v[3] = {(unsigned)i, (unsigned)i, (unsigned)i};
  if (aug_needs_hist(d)) {
    unsigned* hs = hist + (long)d.hist_slot * 1024;
    for (int c = 0; c < 4; ++c) {
      h[c][i] = hs[c * 256 + i];
      hs[c * 256 + i] = 0;                             // this thread's own entries: the slot is clean for the next layer
    }
    if (i < 3) { lo[i] = 256; hi[i] = -1; nz[i] = 0; }
    __syncthreads();
  }
  switch (d.op) {
    case GAVA_AUG_INVERT: v[0] = v[1] = v[2] = 255 - i; break;
    case GAVA_AUG_POSTERIZE: {
      const unsigned mask = d.iarg >= 8 ? 0xffu : (~((1u << (8 - d.iarg)) - 1u) & 0xffu);
      v[0] = v[1] = v[2] = i & mask;
    } break;
    case GAVA_AUG_SOLARIZE: v[0] = v[1] = v[2] = i < d.iarg ? i : 255 - i; break;
    case GAVA_AUG_SOLARIZE_ADD: v[0] = v[1] = v[2] = i < 128 ? (i + d.iarg > 255 ? 255 : i + d.iarg) : i; break;
    case GAVA_AUG_BRIGHTNESS: v[0] = v[1] = v[2] = blend_u8(0, i, f, inside); break;
    case GAVA_AUG_CONTRAST: {
      // mean = int(sum_i i hL[i] / sum_i hL[i] + 0.5) in fp64, as ImageStat and ImageEnhance.Contrast form it
      wsum[i] = (unsigned long long)i * h[3][i];
      csum[i] = h[3][i];
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (i < o) { wsum[i] += wsum[i + o]; csum[i] += csum[i + o]; }
        __syncthreads();
      }
      const int mean = csum[0] ? (int)((double)wsum[0] / (double)csum[0] + 0.5) : 0;
      v[0] = v[1] = v[2] = blend_u8(mean, i, f, inside);
    } break;
    case GAVA_AUG_AUTOCONTRAST: {
      for (int c = 0; c < 3; ++c)
        if (h[c][i]) { atomicMin(&lo[c], i); atomicMax(&hi[c], i); }
      __syncthreads();
      for (int c = 0; c < 3; ++c) {
        if (hi[c] <= lo[c]) continue;
        const double scale = 255.0 / (double)(hi[c] - lo[c]);
        const double offset = (double)(-lo[c]) * scale;
        const int ix = (int)((double)i * scale + offset);
        v[c] = ix < 0 ? 0 : (ix > 255 ? 255 : ix);
      }
    } break;
    case GAVA_AUG_EQUALIZE: {
      for (int c = 0; c < 3; ++c) {
        scan[c][i] = h[c][i];
        if (h[c][i]) { atomicAdd(&nz[c], 1); atomicMax(&hi[c], i); }
      }
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {              // inclusive prefix sums of the three histograms
        unsigned t[3];
        for (int c = 0; c < 3; ++c) t[c] = i >= o ? scan[c][i - o] : 0;
        __syncthreads();
        for (int c = 0; c < 3; ++c) scan[c][i] += t[c];
        __syncthreads();
      }
      for (int c = 0; c < 3; ++c) {
        if (nz[c] <= 1) continue;
        const unsigned step = (scan[c][255] - h[c][hi[c]]) / 255u;
        if (!step) continue;
        const unsigned n = step / 2 + (scan[c][i] - h[c][i]);
        const unsigned q = n / step;
        v[c] = q > 255 ? 255 : q;                      // Image.point clips the table to a byte
      }
    } break;
    default: break;
  }
  for (int c = 0; c < 3; ++c) out[c * 256 + i] = (uint8_t)v[c];
}

// ---- pixels -------------------------------------------------------------------------------------------------------------------
// grid (x: frame of the layer, y: strides the frame).  The kind is the frame's, so every branch on it is uniform in a workgroup.
// Frames are packed RGB: rows of 3 W bytes, in general at no alignment.  No address outside a frame is formed: every index is
// bounded by the frame's byte or pixel count, every sampled coordinate is clipped first.

static __device__ void apply_table(const gava_augment_desc& d, const uint8_t* luts) {
  __shared__ uint8_t lut[768];
  const int tid = threadIdx.x;
  for (int e = tid; e < 768; e += 256) lut[e] = luts[(long)d.lut_slot * 768 + e];
  __syncthreads();
  const int n = d.H * d.W * 3;
  if ((((uintptr_t)d.src | (uintptr_t)d.dst) & 15) == 0) {
    // 16 bytes per access; 16 = 1 mod 3, so the channel of the first byte of vector i is i % 3
    const int nv = n >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(d.src);
    uint4* d4 = reinterpret_cast<uint4*>(d.dst);
    for (int i = blockIdx.y * 256 + tid; i < nv; i += gridDim.y * 256) {
      const uint4 q = s4[i];
      unsigned w[4] = {q.x, q.y, q.z, q.w};
      int c = i % 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          r |= (unsigned)lut[c * 256 + ((w[j] >> (8 * k)) & 255u)] << (8 * k);
          c = c == 2 ? 0 : c + 1;
        }
        w[j] = r;
      }
      d4[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (blockIdx.y == 0) {
      const int i = (nv << 4) + tid;                   // the last n % 16 bytes
      if (tid < 16 && i < n) d.dst[i] = lut[(i % 3) * 256 + d.src[i]];
    }
  } else {
    for (int i = blockIdx.y * 256 + tid; i < n; i += gridDim.y * 256) d.dst[i] = lut[(i % 3) * 256 + d.src[i]];
  }
}

// A thread owns four consecutive pixels: twelve bytes, stored as three dwords (a wave writes 768 contiguous bytes); the last
// pixels of a frame whose count is no multiple of four go out byte by byte.  f(p) is pixel p's result, packed like load_rgb's.
template <class F>
static __device__ __forceinline__ void for_each_quad(const gava_augment_desc& d, F f) {
  const int npix = d.H * d.W, nq = (npix + 3) >> 2;
  for (int q = blockIdx.y * 256 + threadIdx.x; q < nq; q += gridDim.y * 256) {
    const int p0 = q * 4;
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = p0 + k < npix ? f(p0 + k) : 0u;
    uint8_t* o = d.dst + (long)p0 * 3;
    if (p0 + 4 <= npix) {
      const unsigned w[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
      __builtin_memcpy(o, w, 12);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (p0 + k < npix) {
          o[3 * k] = (uint8_t)px[k]; o[3 * k + 1] = (uint8_t)(px[k] >> 8); o[3 * k + 2] = (uint8_t)(px[k] >> 16);
        }
    }
  }
}

// ImageEnhance.Color: blend(L, v, f) per channel
static __device__ void apply_color(const gava_augment_desc& d) {
  const int npix = d.H * d.W;
  const float f = d.factor;
  const bool inside = f >= 0.0f && f <= 1.0f;
  for_each_quad(d, [&](int p) {
    const unsigned v = load_rgb(d.src, p, npix);
    const int L = luma_u8(chan(v, 0), chan(v, 1), chan(v, 2));
    return blend_u8(L, chan(v, 0), f, inside) | (blend_u8(L, chan(v, 1), f, inside) << 8) | (blend_u8(L, chan(v, 2), f, inside) << 16);
  });
}

// ImageEnhance.Sharpness: blend(SMOOTH(v), v, f).  The filter accumulates in fp32 from 0.5, row-major, each pixel times
// fl32(k / 13), clips and truncates; it copies the one-pixel border, where the blend of a pixel with itself is the pixel.
static __device__ void apply_sharpness(const gava_augment_desc& d) {
  const int npix = d.H * d.W, W = d.W, H = d.H;
  const float f = d.factor;
  const bool inside = f >= 0.0f && f <= 1.0f;
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  for_each_quad(d, [&](int p) {
    const int y = p / W, x = p - y * W;
    const unsigned own = load_rgb(d.src, p, npix);
    if (y == 0 || x == 0 || y == H - 1 || x == W - 1) return own;
    float acc[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const unsigned v = (dy == 0 && dx == 0) ? own : load_rgb(d.src, p + dy * W + dx, npix);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (float)chan(v, c) * ((dy == 0 && dx == 0) ? k5 : k1);
      }
    unsigned r = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) r |= blend_u8((int)fminf(fmaxf(acc[c], 0.0f), 255.0f), chan(own, c), f, inside) << (8 * c);
    return r;
  });
}

static __device__ __forceinline__ int clipi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

static __device__ __forceinline__ double lerp64(double a, double b, double t) { return a + (b - a) * t; }

static __device__ __forceinline__ double cubic64(double v1, double v2, double v3, double v4, double t) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + t * (p2 + t * (p3 + t * p4));
}

// Image.transform(size, AFFINE, m, resample, fillcolor = 128): Geometry.c's affine_transform and its bilinear / bicubic filters
template <int FILTER>
static __device__ void apply_affine(const gava_augment_desc& d) {
  const int npix = d.H * d.W, W = d.W, H = d.H;
  const double a0 = d.m[0], a1 = d.m[1], a2 = d.m[2], a3 = d.m[3], a4 = d.m[4], a5 = d.m[5];
  for_each_quad(d, [&](int p) {
    const int yo = p / W, xo = p - yo * W;
    const double xc = (double)xo + 0.5, yc = (double)yo + 0.5;
    double xin = a0 * xc + a1 * yc + a2;
    double yin = a3 * xc + a4 * yc + a5;
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return 0x808080u;
    xin -= 0.5; yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const int x = (int)fx, y = (int)fy;
    const double dx = xin - fx, dy = yin - fy;
    unsigned r = 0;
    if (FILTER == GAVA_AUG_BILINEAR) {
      const int y0 = clipi(y, H) * W, y1 = clipi(y + 1, H) * W, x0 = clipi(x, W), x1 = clipi(x + 1, W);
      const unsigned p00 = load_rgb(d.src, y0 + x0, npix), p01 = load_rgb(d.src, y0 + x1, npix);
      const unsigned p10 = load_rgb(d.src, y1 + x0, npix), p11 = load_rgb(d.src, y1 + x1, npix);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v1 = lerp64((double)chan(p00, c), (double)chan(p01, c), dx);
        const double v2 = lerp64((double)chan(p10, c), (double)chan(p11, c), dx);
        r |= (unsigned)(int)lerp64(v1, v2, dy) << (8 * c);
      }
    } else {
      int xs[4];
      unsigned px[4][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[k] = clipi(x - 1 + k, W);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int yk = clipi(y - 1 + k, H) * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) px[k][j] = load_rgb(d.src, yk + xs[j], npix);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          v[k] = cubic64((double)chan(px[k][0], c), (double)chan(px[k][1], c), (double)chan(px[k][2], c), (double)chan(px[k][3], c), dx);
        const double t = cubic64(v[0], v[1], v[2], v[3], dy);
        r |= (t <= 0.0 ? 0u : (t >= 255.0 ? 255u : (unsigned)(int)t)) << (8 * c);
      }
    }
    return r;
  });
}

__global__ __launch_bounds__(256) void augment_apply_kernel(const gava_augment_desc* desc, const uint8_t* luts) {
  const gava_augment_desc d = desc[blockIdx.x];
  switch (d.kind) {
    case GAVA_AUG_TABLE: apply_table(d, luts); break;
    case GAVA_AUG_COLOR: apply_color(d); break;
    case GAVA_AUG_SHARPNESS: apply_sharpness(d); break;
    case GAVA_AUG_AFFINE:
      if (d.filter == GAVA_AUG_BILINEAR) apply_affine<GAVA_AUG_BILINEAR>(d);
      else apply_affine<GAVA_AUG_BICUBIC>(d);
      break;
    default: break;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct LayerShape { int max_pixels, n_hist, n_table; };

// the host copy of the table, before any launch
static bool augment_args_ok(const gava_augment_args* a, LayerShape* shape) {
  if (!a || !a->desc_host || !a->desc || a->n < 1 || a->n_hist < 0 || a->n_luts < 0) return false;
  LayerShape s{0, 0, 0};
  for (int i = 0; i < a->n; ++i) {
    const gava_augment_desc& d = a->desc_host[i];
    if (!d.src || !d.dst || d.H < 1 || d.W < 1) return false;
    const long bytes = (long)d.H * d.W * 3;
    if (bytes > 0x7fffffffL) return false;
    const uintptr_t s0 = (uintptr_t)d.src, d0 = (uintptr_t)d.dst;
    if (s0 < d0 + (uintptr_t)bytes && d0 < s0 + (uintptr_t)bytes) return false;        // equal or overlapping
    if (!(d.factor - d.factor == 0.0f)) return false;                                  // inf and NaN fail
    for (int k = 0; k < 6; ++k)
      if (!(d.m[k] - d.m[k] == 0.0)) return false;
    switch (d.kind) {
      case GAVA_AUG_TABLE:
        if (d.op < GAVA_AUG_INVERT || d.op > GAVA_AUG_EQUALIZE) return false;
        if (!a->luts || d.lut_slot < 0 || d.lut_slot >= a->n_luts) return false;
        if (d.op >= GAVA_AUG_CONTRAST) {
          if (!a->hist || d.hist_slot < 0 || d.hist_slot >= a->n_hist) return false;
          ++s.n_hist;
        }
        if ((d.op == GAVA_AUG_POSTERIZE || d.op == GAVA_AUG_SOLARIZE || d.op == GAVA_AUG_SOLARIZE_ADD) && (d.iarg < 0 || d.iarg > 256))
          return false;
        ++s.n_table;
        break;
      case GAVA_AUG_COLOR: case GAVA_AUG_SHARPNESS: break;
      case GAVA_AUG_AFFINE:
        if (d.filter != GAVA_AUG_BILINEAR && d.filter != GAVA_AUG_BICUBIC) return false;
        break;
      default: return false;
    }
    const int pixels = d.H * d.W;
    if (pixels > s.max_pixels) s.max_pixels = pixels;
  }
  *shape = s;
  return true;
}

static unsigned strides_for(int items, int per_group, int cap) {
  const int g = (items + per_group - 1) / per_group;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

extern "C" int gava_augment_hist(const gava_augment_args* a, gava_stream_t stream) {
  LayerShape s;
  if (!augment_args_ok(a, &s)) return GAVA_EINVAL;
  if (!s.n_hist) return GAVA_OK;
  hipLaunchKernelGGL(augment_hist_kernel, dim3((unsigned)a->n, strides_for(s.max_pixels, 256 * 16, 64)), dim3(256), 0, (hipStream_t)stream,
                     a->desc, a->hist);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_augment_luts(const gava_augment_args* a, gava_stream_t stream) {
  LayerShape s;
  if (!augment_args_ok(a, &s)) return GAVA_EINVAL;
  if (!s.n_table) return GAVA_OK;
  hipLaunchKernelGGL(augment_luts_kernel, dim3((unsigned)a->n), dim3(256), 0, (hipStream_t)stream, a->desc, a->hist, a->luts);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_augment_apply(const gava_augment_args* a, gava_stream_t stream) {
  LayerShape s;
  if (!augment_args_ok(a, &s)) return GAVA_EINVAL;
  hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)a->n, strides_for(s.max_pixels, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream,
                     a->desc, a->luts);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_augment_struct_sizes(size_t* out, int cap) {
  const size_t v[] = {sizeof(gava_augment_desc), sizeof(gava_augment_args)};
  for (int i = 0; out && i < 2 && i < cap; ++i) out[i] = v[i];
  return 2;
}
