// mix.hip — Mixup / CutMix of a batch of clips on the device, the soft targets that go with the mix, and the reference's
// criterion for targets of the logits' shape (cross-entropy with class probabilities times the ordinal-focal weight, mean) with
// its backward.  Everything is fp32 (the targets' few values are formed in fp64 and rounded once); reductions run in a fixed
// order (xor butterflies inside a wave, an LDS tree across waves), integer atomics only (the confusion matrix): the same bits
// on every run.  The formulas are in include/gava_hip.h.
#include "common.h"

namespace {

static __device__ __forceinline__ int clamp_label(long y, int C) { return (int)(y < 0 ? 0 : (y >= C ? C - 1 : y)); }

// ---- clips --------------------------------------------------------------------------------------------------------------------
// What a descriptor asks of its clip, decided once per workgroup (blockIdx.y is the clip, so every branch on it is uniform):
//   COPY  own pixels (its own partner, or Mixup with lam == 1)      SWAP  the partner's pixels (Mixup with lam == 0)
//   BOX   CutMix: the partner's pixels inside the box               LERP  lam * own + (1 - lam) * partner
enum { MIX_COPY = 0, MIX_SWAP = 1, MIX_BOX = 2, MIX_LERP = 3 };

static __device__ __forceinline__ int mix_kind(const gava_mix_desc& d, int clip) {
  if (d.partner == clip) return MIX_COPY;
  if (d.y1 > d.y0 && d.x1 > d.x0) return MIX_BOX;
  return d.lam == 1.0f ? MIX_COPY : (d.lam == 0.0f ? MIX_SWAP : MIX_LERP);
}

// does the result at row h, columns [w0, w0 + V) differ from the clip's own pixels?
template <int V>
static __device__ __forceinline__ bool mix_touches(int kind, const gava_mix_desc& d, int h, int w0) {
  if (kind == MIX_BOX) return h >= d.y0 && h < d.y1 && w0 < d.x1 && w0 + V > d.x0;
  return kind != MIX_COPY;
}

// one rounding for 1 - lam, one for its product, one for the fma: the same expression in and out of place
static __device__ __forceinline__ float mix_one(int kind, const gava_mix_desc& d, float own, float other, int h, int w) {
  switch (kind) {
    case MIX_SWAP: return other;
    case MIX_BOX: return (h >= d.y0 && h < d.y1 && w >= d.x0 && w < d.x1) ? other : own;
    case MIX_LERP: return __fmaf_rn(d.lam, own, __fmul_rn(__fsub_rn(1.0f, d.lam), other));
    default: return own;
  }
}

template <int V> struct Vec;
template <> struct Vec<1> {
  float v[1];
  static __device__ __forceinline__ Vec load(const float* p) { Vec r; r.v[0] = p[0]; return r; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <> struct Vec<4> {
  float v[4];
  static __device__ __forceinline__ Vec load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    Vec r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

template <int V>
static __device__ __forceinline__ Vec<V> mix_vec(int kind, const gava_mix_desc& d, const Vec<V>& own, const Vec<V>& other, int h, int w0) {
  Vec<V> r;
#pragma unroll
  for (int e = 0; e < V; ++e) r.v[e] = mix_one(kind, d, own.v[e], other.v[e], h, w0 + e);
  return r;
}

struct MixParams {
  const float* x; float* out;
  const gava_mix_desc* desc;
  int clip0, H, Wv;            // Wv = W / V items per row
  int items;                   // planes * H * W / V items per clip
  long n;                      // elements per clip
};

// grid (x: strides the items of a clip, y: clips from clip0).  V = 4: every item is one aligned 16-byte access (W % 4 == 0 and
// aligned bases, so no item crosses a row); V = 1 otherwise.  An item is addressed only when it lies inside its clip.
template <int V>
__global__ __launch_bounds__(256) void mix_clips_kernel(const MixParams p) {
  const int clip = p.clip0 + blockIdx.y;
  const gava_mix_desc d = p.desc[clip];
  const int kind = mix_kind(d, clip);
  const float* own = p.x + (long)clip * p.n;
  const float* other = p.x + (long)d.partner * p.n;
  float* out = p.out + (long)clip * p.n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.items; i += gridDim.x * 256) {
    int h = 0, w0 = 0;
    if (kind == MIX_BOX) {
      const int row = i / p.Wv;
      h = row % p.H;
      w0 = (i - row * p.Wv) * V;
    }
    const Vec<V> a = Vec<V>::load(own + (long)i * V);
    if (!mix_touches<V>(kind, d, h, w0)) { a.store(out + (long)i * V); continue; }
    const Vec<V> b = Vec<V>::load(other + (long)i * V);
    mix_vec<V>(kind, d, a, b, h, w0).store(out + (long)i * V);
  }
}

// out == x, partner an involution: the workgroups of the lower clip of a pair own both clips of it - a thread reads position i
// of both originals, then writes both results, each by its clip's own descriptor.  Items neither descriptor changes are not
// touched at all; a clip that is its own partner, and the higher clip of a pair, have nothing to do.
template <int V>
__global__ __launch_bounds__(256) void mix_clips_inplace_kernel(const MixParams p) {
  const int clip = p.clip0 + blockIdx.y;
  const gava_mix_desc d = p.desc[clip];
  const int mate = d.partner;
  if (mate <= clip) return;
  const gava_mix_desc dm = p.desc[mate];
  const int kind = mix_kind(d, clip), kind_m = mix_kind(dm, mate);
  if (kind == MIX_COPY && kind_m == MIX_COPY) return;
  float* xa = p.out + (long)clip * p.n;
  float* xb = p.out + (long)mate * p.n;
  const bool boxes = kind == MIX_BOX || kind_m == MIX_BOX;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.items; i += gridDim.x * 256) {
    int h = 0, w0 = 0;
    if (boxes) {
      const int row = i / p.Wv;
      h = row % p.H;
      w0 = (i - row * p.Wv) * V;
    }
    const bool ta = mix_touches<V>(kind, d, h, w0), tb = mix_touches<V>(kind_m, dm, h, w0);
    if (!ta && !tb) continue;
    const Vec<V> a = Vec<V>::load(xa + (long)i * V), b = Vec<V>::load(xb + (long)i * V);
    if (ta) mix_vec<V>(kind, d, a, b, h, w0).store(xa + (long)i * V);
    if (tb) mix_vec<V>(kind_m, dm, b, a, h, w0).store(xb + (long)i * V);
  }
}

// ---- targets ------------------------------------------------------------------------------------------------------------------
// targets[i][c] = lam s(y_i)[c] + (1 - lam) s(y_j)[c],  s(y)[c] = (1 - eps) [c == y] + eps / C: formed in fp64, rounded once
__global__ __launch_bounds__(256) void mix_targets_kernel(const long long* labels, const gava_mix_desc* desc, int B, int C, float eps,
                                                          float* targets, long ld) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * C) return;
  const int i = (int)(idx / C), c = (int)(idx - (long)i * C);
  const gava_mix_desc d = desc[i];
  const int j = d.partner < 0 ? 0 : (d.partner >= B ? B - 1 : d.partner);       // validated on the host; never index past the labels
  const int yi = clamp_label(labels[i], C), yj = clamp_label(labels[j], C);
  const double off = (double)eps / (double)C, on = (1.0 - (double)eps) + off;
  const double lam = j == i ? 1.0 : (double)d.lam;                              // its own partner keeps its label, exactly
  targets[(long)i * ld + c] = (float)(lam * (c == yi ? on : off) + (1.0 - lam) * (c == yj ? on : off));
}

// ---- soft criterion -----------------------------------------------------------------------------------------------------------
// One wave per sample, lanes stride the classes, as criterion_rows_kernel of train_head.hip: with m = max_c z_c at k (the lowest
// such class) and s1 = sum_{c != k} exp(z_c - m), logsumexp = m + log1p(s1) and 1 - p_c = s1 / (1 + s1) for c == k,
// ((1 + s1) - e_c) / (1 + s1) otherwise.  Classes with a zero target add nothing (and are not evaluated).
struct SoftParams {
  const float* logits; long ld;
  const float* targets; long ldt;
  int B, C, weighted;
  float alpha, gamma, beta, scale;
  float* per_sample; float* weight; int* top1; int* target1; int* conf;
  float4* saved;               // two per sample: (m, log1p(s1), s1, bits of k), (w, ce scale alpha gamma, Q, tau)
};

__global__ __launch_bounds__(256) void soft_rows_kernel(const SoftParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B) return;
  const float* z = p.logits + (long)row * p.ld;
  const float* t = p.targets + (long)row * p.ldt;
  float m = -INFINITY, tm = -INFINITY, tau = 0.f;
  int k = 0x7fffffff, ys = 0x7fffffff;
  for (int c = lane; c < p.C; c += 64) {
    const float v = z[c], tv = t[c];
    if (v > m) { m = v; k = c; }                   // c ascends within a lane: strictly greater keeps the lowest class
    if (tv > tm) { tm = tv; ys = c; }
    tau += tv;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), otm = __shfl_xor(tm, o, 64);
    const int ok = __shfl_xor(k, o, 64), oys = __shfl_xor(ys, o, 64);
    if (om > m || (om == m && ok < k)) { m = om; k = ok; }
    if (otm > tm || (otm == tm && oys < ys)) { tm = otm; ys = oys; }
  }
  tau = wave_sum(tau);
  // NaN rows (nothing compared greater): class 0 and a stand-in for the maximum keep every index in range; the row's outputs
  // are then unspecified, as they are for a row holding +-inf
  if (k >= p.C) { k = 0; m = wave_max(z[lane < p.C ? lane : 0]); }
  if (ys >= p.C) ys = 0;
  float s1 = 0.f;
  for (int c = lane; c < p.C; c += 64)
    if (c != k) s1 += expf(z[c] - m);
  s1 = wave_sum(s1);
  const float l = log1pf(s1), sum = 1.0f + s1;
  float ce = 0.f, focal = 0.f, q = 0.f;
  for (int c = lane; c < p.C; c += 64) {
    const float tv = t[c];
    if (tv == 0.f) continue;
    ce += tv * ((m - z[c]) + l);                   // both terms >= 0
    if (p.weighted) {
      const float e = c == k ? 1.0f : expf(z[c] - m);
      const float omp = c == k ? s1 / sum : (sum - e) / sum;
      focal += tv * powf(omp, p.gamma);
      q += tv * powf(omp, p.gamma - 1.0f) * (e / sum);
    }
  }
  ce = wave_sum(ce);
  float w = 1.0f, cg = 0.f, loss = ce;
  if (p.weighted) {
    focal = wave_sum(focal); q = wave_sum(q);
    const int d = ys > k ? ys - k : k - ys;
    const float ordinal = p.beta * ((float)d / (float)(p.C - 1));
    w = p.scale * (ordinal * tau + p.alpha * focal);
    loss = ce * w;
    cg = ce * p.scale * p.alpha * p.gamma;
  }
  if (lane == 0) {
    p.per_sample[row] = loss;
    p.weight[row] = w;
    p.top1[row] = k;
    p.target1[row] = ys;
    p.saved[2 * row] = make_float4(m, l, s1, __int_as_float(k));
    p.saved[2 * row + 1] = make_float4(w, cg, q, tau);
    if (p.conf) atomicAdd(p.conf + (long)ys * p.C + k, 1);
  }
}

// loss = mean of per_sample, hits = #{top1 == target1}: one workgroup; thread t adds samples t, t + 256, ... in order, then a tree
__global__ __launch_bounds__(256) void soft_mean_kernel(const float* per_sample, const int* top1, const int* target1, int B, float* loss,
                                                        int* hits) {
  __shared__ float fs[256];
  __shared__ int hs[256];
  float s = 0.f;
  int h = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    s += per_sample[i];
    h += top1[i] == target1[i] ? 1 : 0;
  }
  fs[threadIdx.x] = s; hs[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { fs[threadIdx.x] += fs[threadIdx.x + o]; hs[threadIdx.x] += hs[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss[0] = fs[0] / (float)B; hits[0] = hs[0]; }
}

struct SoftBwdParams {
  const float* logits; long ld;
  const float* targets; long ldt;
  const float4* saved; const float* grad_loss;
  int B, C, weighted; float gamma;
  float* dlogits; long ldd;
};

__global__ __launch_bounds__(256) void soft_backward_kernel(const SoftBwdParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B) return;
  const float* z = p.logits + (long)row * p.ld;
  const float* t = p.targets + (long)row * p.ldt;
  const float4 s0 = p.saved[2 * row], s1v = p.saved[2 * row + 1];
  const float m = s0.x, s1 = s0.z, sum = 1.0f + s0.z;
  const int k = __float_as_int(s0.w);
  const float w = s1v.x, cg = s1v.y, q = s1v.z, tau = s1v.w;
  const float g = p.grad_loss[0] / (float)p.B;
  for (int c = lane; c < p.C; c += 64) {
    const float e = c == k ? 1.0f : expf(z[c] - m);
    const float pc = e / sum, tv = t[c];
    float d = w * (tau * pc - tv);
    if (p.weighted) {
      const float omp = c == k ? s1 / sum : (sum - e) / sum;
      const float own = tv == 0.f ? 0.f : tv * powf(omp, p.gamma - 1.0f);
      d += cg * pc * (q - own);
    }
    p.dlogits[(long)row * p.ldd + c] = d * g;
  }
}

static bool mix_desc_ok(const gava_mix_desc* d, int B, int H, int W, bool inplace) {
  for (int i = 0; i < B; ++i) {
    if (d[i].partner < 0 || d[i].partner >= B) return false;
    if (!(d[i].lam >= 0.0f && d[i].lam <= 1.0f)) return false;                     // NaN fails both comparisons
    if (d[i].y0 < 0 || d[i].y0 > d[i].y1 || d[i].y1 > H || d[i].x0 < 0 || d[i].x0 > d[i].x1 || d[i].x1 > W) return false;
  }
  for (int i = 0; inplace && i < B; ++i)
    if (d[d[i].partner].partner != i) return false;
  return true;
}

template <int V>
static void launch_mix(const MixParams& base, int B, bool inplace, hipStream_t s) {
  MixParams p = base;
  const int gx = (p.items + 255) / 256 < 1024 ? (p.items + 255) / 256 : 1024;     // the rest by the grid-stride loop
  for (int c0 = 0; c0 < B; c0 += 65535) {                                         // a grid's y extent
    const int nb = B - c0 < 65535 ? B - c0 : 65535;
    p.clip0 = c0;
    if (inplace) hipLaunchKernelGGL(mix_clips_inplace_kernel<V>, dim3(gx, nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(mix_clips_kernel<V>, dim3(gx, nb), dim3(256), 0, s, p);
  }
}

}  // namespace

extern "C" int gava_mix_clips(const gava_mix_clips_args* a, gava_stream_t stream) {
  if (!a || !a->x || !a->out || !a->desc_host || !a->desc) return GAVA_EINVAL;
  if (a->B < 1 || a->planes < 1 || a->H < 1 || a->W < 1) return GAVA_EINVAL;
  const long n = (long)a->planes * a->H * a->W;
  if (n > 0x7fffffffL) return GAVA_EINVAL;
  const bool inplace = a->out == a->x;
  if (!inplace) {                                                                 // a partial overlap would read mixed pixels
    const uintptr_t x0 = (uintptr_t)a->x, o0 = (uintptr_t)a->out, bytes = (uintptr_t)n * a->B * sizeof(float);
    if (x0 < o0 + bytes && o0 < x0 + bytes) return GAVA_EINVAL;
  }
  if (!mix_desc_ok(a->desc_host, a->B, a->H, a->W, inplace)) return GAVA_EINVAL;
  MixParams p{a->x, a->out, a->desc, 0, a->H, a->W, (int)n, n};
  if (a->W % 4 == 0 && ((uintptr_t)a->x | (uintptr_t)a->out) % 16 == 0) {
    p.Wv = a->W / 4; p.items = (int)(n / 4);
    launch_mix<4>(p, a->B, inplace, (hipStream_t)stream);
  } else {
    launch_mix<1>(p, a->B, inplace, (hipStream_t)stream);
  }
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_mix_targets(const gava_mix_targets_args* a, gava_stream_t stream) {
  if (!a || !a->labels || !a->desc || !a->targets) return GAVA_EINVAL;
  if (a->B < 1 || a->C < 1 || a->ld_targets < a->C || !(a->smoothing >= 0.0f && a->smoothing <= 1.0f)) return GAVA_EINVAL;
  const long blocks = ((long)a->B * a->C + 255) / 256;
  if (blocks > 0x7fffffffL) return GAVA_EINVAL;
  hipLaunchKernelGGL(mix_targets_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const long long*)a->labels, a->desc,
                     a->B, a->C, a->smoothing, a->targets, (long)a->ld_targets);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_soft_criterion(const gava_soft_criterion_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->C < 1) return GAVA_EINVAL;
  if (!a->logits || !a->targets || !a->loss || !a->per_sample || !a->weight || !a->top1 || !a->target1 || !a->hits || !a->saved)
    return GAVA_EINVAL;
  if (a->ld_logits < a->C || a->ld_targets < a->C) return GAVA_EINVAL;
  if (a->weighted && (!(a->gamma >= 1.0f) || a->C < 2)) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  SoftParams p{a->logits, (long)a->ld_logits, a->targets, (long)a->ld_targets, a->B, a->C, a->weighted, a->alpha, a->gamma, a->beta,
               a->scale, a->per_sample, a->weight, a->top1, a->target1, a->conf, (float4*)a->saved};
  hipLaunchKernelGGL(soft_rows_kernel, dim3((a->B + 3) / 4), dim3(256), 0, s, p);
  hipLaunchKernelGGL(soft_mean_kernel, dim3(1), dim3(256), 0, s, a->per_sample, a->top1, a->target1, a->B, a->loss, a->hits);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_soft_criterion_backward(const gava_soft_criterion_args* a, gava_stream_t stream) {
  if (!a || a->B < 1 || a->C < 1) return GAVA_EINVAL;
  if (!a->logits || !a->targets || !a->saved || !a->grad_loss || !a->dlogits) return GAVA_EINVAL;
  if (a->ld_logits < a->C || a->ld_targets < a->C || a->ld_dlogits < a->C) return GAVA_EINVAL;
  if (a->weighted && (!(a->gamma >= 1.0f) || a->C < 2)) return GAVA_EINVAL;
  SoftBwdParams p{a->logits, (long)a->ld_logits, a->targets, (long)a->ld_targets, (const float4*)a->saved, a->grad_loss, a->B, a->C,
                  a->weighted, a->gamma, a->dlogits, (long)a->ld_dlogits};
  hipLaunchKernelGGL(soft_backward_kernel, dim3((a->B + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_mix_struct_sizes(size_t* out, int cap) {
  const size_t v[] = {sizeof(gava_mix_desc), sizeof(gava_mix_clips_args), sizeof(gava_mix_targets_args), sizeof(gava_soft_criterion_args)};
  for (int i = 0; out && i < 4 && i < cap; ++i) out[i] = v[i];
  return 4;
}
