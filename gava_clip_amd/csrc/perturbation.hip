// perturbation.hip — faithfulness curves of an importance map (deletion / insertion by patch or frame): the four helpers
// around the plain forward.  gava_patch_ranks ranks the units of a score map, gava_blur_clips makes the blurred baseline,
// gava_perturb_clips writes the S1 perturbed copies of every clip, gava_perturb_scores turns the logits into curves and areas.
// All of it is a few passes over a clip next to S1 forwards of it; the kernels are written to be exact and reproducible
// (no atomics, fixed summation orders) and to touch memory in whole 16-byte lanes, not to be clever.
#include "common.h"

namespace {

// ---- ranks -----------------------------------------------------------------------------------------------------------
// A score becomes a 32-bit key whose UNSIGNED order is the ranking's order: NaN -> 0 (below everything), +-0 -> 0x80000000, a
// negative value -> its complemented bits, any other -> its bits with the sign set.  -inf becomes 0x007fffff: above NaN.
// Unit j is before unit i when key_j > key_i, or key_j == key_i and j < i.  A thread owns one unit, a workgroup RK_THREADS
// consecutive units of one ranking; the ranking's keys stream through LDS RK_TILE at a time, every thread reading the same
// four keys (a broadcast read) against its own: tiles in front of the workgroup's own tile count >=, tiles behind it >, its
// own tile compares the positions too.  The three cases are uniform over the workgroup.  Few units per workgroup on purpose:
// a c2 clip has 1568 units, and the time of the call is the time of one workgroup.
constexpr int RK_THREADS = 256, RK_TILE = 1024;

struct RankParams {
  const float* scores; int* ranks;
  int n;                 // units per ranking
};

// Integer tests only: the order must not depend on the kernel's denormal mode.
static __device__ __forceinline__ unsigned rank_key(float v) {
  const unsigned u = __float_as_uint(v), mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u) return 0u;                    // NaN
  if (mag == 0u) return 0x80000000u;                   // +-0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(RK_THREADS) void patch_ranks_kernel(const RankParams p) {
  __shared__ __attribute__((aligned(16))) unsigned keys[RK_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * RK_THREADS + tid;         // this thread's unit
  const float* scores = p.scores + (long)blockIdx.y * p.n;
  const int own = blockIdx.x * RK_THREADS / RK_TILE;   // the tile this workgroup's units lie in
  const int n_tiles = (p.n + RK_TILE - 1) / RK_TILE;
  const unsigned mine = i < p.n ? rank_key(scores[i]) : 0u;
  int cnt = 0;
  for (int t = 0; t < n_tiles; ++t) {
    // keys[pos] belongs to unit t * RK_TILE + pos.  Past the ranking's end the key is 0 at a position above every real one:
    // it is before nothing, except in the >= case, which only tiles in front of the own one take - and those are full
#pragma unroll
    for (int r = 0; r < RK_TILE / RK_THREADS; ++r) {
      const int j = t * RK_TILE + r * RK_THREADS + tid;
      keys[r * RK_THREADS + tid] = j < p.n ? rank_key(scores[j]) : 0u;
    }
    __syncthreads();
    const int valid = min(RK_TILE, p.n - t * RK_TILE);
    const int quads = (valid + 3) >> 2;                // the tail's keys are 0
    if (t < own) {
#pragma unroll 4
      for (int q = 0; q < quads; ++q) {
        const uint4 k = *reinterpret_cast<const uint4*>(keys + 4 * q);
        cnt += (int)(k.x >= mine) + (int)(k.y >= mine) + (int)(k.z >= mine) + (int)(k.w >= mine);
      }
    } else if (t > own) {
#pragma unroll 4
      for (int q = 0; q < quads; ++q) {
        const uint4 k = *reinterpret_cast<const uint4*>(keys + 4 * q);
        cnt += (int)(k.x > mine) + (int)(k.y > mine) + (int)(k.z > mine) + (int)(k.w > mine);
      }
    } else {
      const int ipos = i - t * RK_TILE;                // pos < ipos: j < i
#pragma unroll 4
      for (int q = 0; q < quads; ++q) {
        const uint4 k = *reinterpret_cast<const uint4*>(keys + 4 * q);
        const int pos = 4 * q;
        cnt += (int)(k.x > mine || (k.x == mine && pos < ipos)) + (int)(k.y > mine || (k.y == mine && pos + 1 < ipos)) +
               (int)(k.z > mine || (k.z == mine && pos + 2 < ipos)) + (int)(k.w > mine || (k.w == mine && pos + 3 < ipos));
      }
    }
    __syncthreads();
  }
  if (i < p.n) p.ranks[(long)blockIdx.y * p.n + i] = cnt;
}

// Pixel scores -> patch scores: a wave per patch.  Lane l adds the patch's pixels l, l + 64, ... (row-major inside the patch) in
// that order, then the lanes are added by the fixed xor butterfly of wave_sum: one order, the same bits on every run.
constexpr int PL_THREADS = 256;

__global__ __launch_bounds__(PL_THREADS) void pool_patches_kernel(const float* __restrict__ pixels, float* __restrict__ pooled,
                                                                  long patches, int g, int patch) {
  const int lane = threadIdx.x & 63;
  const long S = (long)g * patch;
  const int gg = g * g, pp = patch * patch;
  const long waves = (long)gridDim.x * (PL_THREADS / 64);
  for (long u = (long)blockIdx.x * (PL_THREADS / 64) + (threadIdx.x >> 6); u < patches; u += waves) {
    const long frame = u / gg;
    const int r = (int)(u - frame * gg), py = r / g, px = r - py * g;
    const float* src = pixels + frame * S * S + (long)py * patch * S + (long)px * patch;
    float acc = 0.f;
    for (int e = lane; e < pp; e += 64) {
      const int ky = e / patch;
      acc += src[ky * S + (e - ky * patch)];
    }
    acc = wave_sum(acc);
    if (lane == 0) pooled[u] = acc;
  }
}

// ---- blur ------------------------------------------------------------------------------------------------------------
// One thread per output element, a grid-stride loop over all planes; the taps sit in LDS, the pixels come through the
// caches (a row pass reads 2r + 1 neighbours of a row, a column pass 2r + 1 row segments: both coalesced).  `step` is the
// distance between neighbours along the pass: 1 (rows) or size (columns).
constexpr int BL_THREADS = 256;

template <bool COLUMNS>
__global__ __launch_bounds__(BL_THREADS) void blur_pass_kernel(const float* __restrict__ src, const float* __restrict__ taps,
                                                               float* __restrict__ dst, long total, int size, int radius) {
  __shared__ float w[2 * GAVA_BLUR_MAX_RADIUS + 1];
  for (int i = threadIdx.x; i < 2 * radius + 1; i += BL_THREADS) w[i] = taps[i];
  __syncthreads();
  const long stride = (long)gridDim.x * BL_THREADS;
  for (long e = (long)blockIdx.x * BL_THREADS + threadIdx.x; e < total; e += stride) {
    const long row = e / size;                       // plane * size + y
    const int xx = (int)(e - row * size);
    const int yy = (int)(row % size);
    const int pos = COLUMNS ? yy : xx;
    const float* line = COLUMNS ? src + (e - (long)yy * size) : src + row * size;      // the element at pos = 0
    const long step = COLUMNS ? size : 1;
    float acc = 0.f;
    for (int i = 0; i <= 2 * radius; ++i) {
      const int q = min(max(pos + i - radius, 0), size - 1);
      acc = fmaf(w[i], line[q * step], acc);
    }
    dst[e] = acc;
  }
}

// ---- perturbed clips ---------------------------------------------------------------------------------------------------
// A work item is VEC consecutive floats of a clip (VEC divides the patch width, so they share a unit): read x and the
// baseline once, look the unit's rank up, write the n_steps selections.  Everything is moved as 32-bit words.
struct PerturbParams {
  const unsigned* x; const int* ranks; const unsigned* baseline; unsigned* out;
  long items;            // nb * 3 * T * size * size / VEC
  int T, size, patch, g;
  int frame_units, insertion, kind, n_steps;
  int k[GAVA_PERTURB_MAX_STEPS];
};

template <int VEC> struct WordVec;
template <> struct WordVec<4> { typedef unsigned type __attribute__((ext_vector_type(4))); };
template <> struct WordVec<2> { typedef unsigned type __attribute__((ext_vector_type(2))); };
template <> struct WordVec<1> { typedef unsigned type; };

constexpr int PT_THREADS = 256;

template <int VEC>
__global__ __launch_bounds__(PT_THREADS) void perturb_clips_kernel(const PerturbParams p) {
  typedef typename WordVec<VEC>::type V;
  const long plane = (long)p.size * p.size;
  const long clip = 3 * (long)p.T * plane;                 // floats per clip
  const long clip_items = clip / VEC;
  const long units = p.frame_units ? p.T : (long)p.T * p.g * p.g;
  const long stride = (long)gridDim.x * PT_THREADS;
  for (long it = (long)blockIdx.x * PT_THREADS + threadIdx.x; it < p.items; it += stride) {
    const long b = it / clip_items;
    const long e = (it - b * clip_items) * VEC;            // float offset inside the clip
    const int c = (int)(e / ((long)p.T * plane));
    const long r1 = e - (long)c * p.T * plane;
    const int t = (int)(r1 / plane);
    const int r2 = (int)(r1 - (long)t * plane);
    const int y = r2 / p.size, xx = r2 - y * p.size;
    const long unit = p.frame_units ? t : ((long)t * p.g + y / p.patch) * p.g + xx / p.patch;
    const int rank = p.ranks[b * units + unit];
    const V xv = *reinterpret_cast<const V*>(p.x + b * clip + e);
    V bv;
    if (p.kind == GAVA_BASELINE_TENSOR) {
      bv = *reinterpret_cast<const V*>(p.baseline + b * clip + e);
    } else {
      const unsigned word = p.kind == GAVA_BASELINE_CHANNEL ? p.baseline[c] : 0u;
      bv = (V)word;                                        // every component
    }
    const V hit = p.insertion ? xv : bv, miss = p.insertion ? bv : xv;       // rank < k: hit
    unsigned* dst = p.out + b * p.n_steps * clip + e;
    for (int s = 0; s < p.n_steps; ++s)
      *reinterpret_cast<V*>(dst + s * clip) = rank < p.k[s] ? hit : miss;
  }
}

template <int VEC>
void launch_perturb(const PerturbParams& p, hipStream_t s) {
  const long blocks = (p.items + PT_THREADS - 1) / PT_THREADS;
  hipLaunchKernelGGL((perturb_clips_kernel<VEC>), dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(PT_THREADS), 0, s, p);
}

// ---- scores ------------------------------------------------------------------------------------------------------------
// One workgroup per clip, a wave per step (steps dealt to the waves).  The argmax keeps the lowest class on equal values:
// within a lane the classes ascend, across lanes (value, index) pairs are compared.
constexpr int PS_THREADS = 256, PS_WAVES = PS_THREADS / 64;

struct ScoreParams {
  const float* logits; long ld;
  const long long* target;
  float* logit; float* prob; int* top1; float* auc_logit; float* auc_prob; long long* target_out;
  int n_steps, C, ref_step;
  float fractions[GAVA_PERTURB_MAX_STEPS];
};

static __device__ __forceinline__ bool value_beats(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// -> (max, argmax) of a row in every lane; a row of NaNs gives (-inf, 0)
static __device__ __forceinline__ void row_argmax(const float* row, int C, int lane, float& bv, int& bi) {
  bv = -INFINITY; bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    if (value_beats(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (value_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (bi >= C) bi = 0;
}

__global__ __launch_bounds__(PS_THREADS) void perturb_scores_kernel(const ScoreParams p) {
  __shared__ float y_logit[GAVA_PERTURB_MAX_STEPS], y_prob[GAVA_PERTURB_MAX_STEPS];
  __shared__ long long tgt_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.x;
  const float* rows = p.logits + b * p.n_steps * p.ld;
  if (wave == 0) {
    long long tg;
    if (p.target) {
      tg = p.target[b];
    } else {
      float bv; int bi;
      row_argmax(rows + p.ref_step * p.ld, p.C, lane, bv, bi);
      tg = bi;
    }
    if (lane == 0) { tgt_s = tg; p.target_out[b] = tg; }
  }
  __syncthreads();
  const long long tg = tgt_s;
  const bool ok = tg >= 0 && tg < p.C;
  const float nan = __builtin_nanf("");
  for (int s = wave; s < p.n_steps; s += PS_WAVES) {
    const float* row = rows + s * p.ld;
    float m; int am;
    row_argmax(row, p.C, lane, m, am);
    float sum = 0.f;
    for (int c = lane; c < p.C; c += 64) sum += expf(row[c] - m);
    sum = wave_sum(sum);
    if (lane == 0) {
      const float xt = ok ? row[tg] : nan;
      const float pr = ok ? expf(xt - m) / sum : nan;
      y_logit[s] = xt; y_prob[s] = pr;
      p.logit[b * p.n_steps + s] = xt;
      p.prob[b * p.n_steps + s] = pr;
      p.top1[b * p.n_steps + s] = am;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {                               // thread 0: the logit curve's area, thread 1: the probability curve's
    const float* y = threadIdx.x ? y_prob : y_logit;
    float acc = ok ? 0.f : nan;                        // (a single step has no area, but a refused target still has no value)
    for (int s = 1; s < p.n_steps; ++s) acc = fmaf(p.fractions[s] - p.fractions[s - 1], 0.5f * (y[s] + y[s - 1]), acc);
    (threadIdx.x ? p.auc_prob : p.auc_logit)[b] = acc;
  }
}

}  // namespace

extern "C" int gava_patch_ranks(const gava_patch_ranks_args* a, gava_stream_t stream) {
  if (!a || !a->scores || !a->ranks) return GAVA_EINVAL;
  if (a->B < 1 || a->T < 1) return GAVA_EINVAL;
  if (a->layout != GAVA_RANK_PATCH && a->layout != GAVA_RANK_PIXEL && a->layout != GAVA_RANK_FRAME) return GAVA_EINVAL;
  if (a->scope != GAVA_SCOPE_CLIP && a->scope != GAVA_SCOPE_FRAME) return GAVA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  long n, rankings;
  RankParams p;
  p.scores = a->scores; p.ranks = a->ranks;
  if (a->layout == GAVA_RANK_FRAME) {
    if (a->scope != GAVA_SCOPE_CLIP) return GAVA_EINVAL;
    n = a->T; rankings = a->B;
  } else {
    if (a->g < 1 || a->g > 32768) return GAVA_EINVAL;
    const long gg = (long)a->g * a->g;
    if (a->scope == GAVA_SCOPE_CLIP) { n = (long)a->T * gg; rankings = a->B; }
    else { n = gg; rankings = (long)a->B * a->T; }
  }
  if (n > GAVA_PERTURB_MAX_UNITS || rankings > 0x7fffffffL || n * rankings > 0x7fffffffL) return GAVA_EINVAL;
  if (a->layout == GAVA_RANK_PIXEL) {
    if (a->patch < 1 || (long)a->g * a->patch > 0x7fffffffL || !a->pooled) return GAVA_EINVAL;
    const long patches = n * rankings, blocks = (patches + PL_THREADS / 64 - 1) / (PL_THREADS / 64);
    hipLaunchKernelGGL(pool_patches_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(PL_THREADS), 0, s, a->scores, a->pooled,
                       patches, a->g, a->patch);
    GAVA_CHECK_LAUNCH();
    p.scores = a->pooled;
  }
  p.n = (int)n;
  // rankings ride on the grid's y extent, 65535 at a time
  const unsigned groups = (unsigned)((n + RK_THREADS - 1) / RK_THREADS);
  for (long r0 = 0; r0 < rankings; r0 += 65535) {
    const long nr = rankings - r0 < 65535 ? rankings - r0 : 65535;
    RankParams q = p;
    q.scores = p.scores + r0 * n;
    q.ranks = p.ranks + r0 * n;
    hipLaunchKernelGGL(patch_ranks_kernel, dim3(groups, (unsigned)nr), dim3(RK_THREADS), 0, s, q);
    GAVA_CHECK_LAUNCH();
  }
  return GAVA_OK;
}

extern "C" int gava_blur_clips(const gava_blur_clips_args* a, gava_stream_t stream) {
  if (!a || !a->x || !a->taps || !a->tmp || !a->out) return GAVA_EINVAL;
  if (a->B < 1 || a->T < 1 || a->size < 1 || a->radius < 0 || a->radius > GAVA_BLUR_MAX_RADIUS) return GAVA_EINVAL;
  if (a->x == a->tmp || a->tmp == a->out || a->x == a->out) return GAVA_EINVAL;
  const long total = 3L * a->B * a->T * a->size * a->size;
  const long blocks = (total + BL_THREADS - 1) / BL_THREADS;
  const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
  hipLaunchKernelGGL((blur_pass_kernel<false>), grid, dim3(BL_THREADS), 0, (hipStream_t)stream, a->x, a->taps, a->tmp, total, a->size, a->radius);
  GAVA_CHECK_LAUNCH();
  hipLaunchKernelGGL((blur_pass_kernel<true>), grid, dim3(BL_THREADS), 0, (hipStream_t)stream, (const float*)a->tmp, a->taps, a->out, total, a->size,
                     a->radius);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_perturb_clips(const gava_perturb_clips_args* a, gava_stream_t stream) {
  if (!a || !a->x || !a->ranks || !a->out) return GAVA_EINVAL;
  if (a->nb < 1 || a->T < 1 || a->size < 1 || a->patch < 1 || a->size % a->patch) return GAVA_EINVAL;
  if (a->n_steps < 1 || a->n_steps > GAVA_PERTURB_MAX_STEPS) return GAVA_EINVAL;
  if (a->units != GAVA_UNITS_PATCH && a->units != GAVA_UNITS_FRAME) return GAVA_EINVAL;
  if (a->mode != GAVA_PERTURB_DELETION && a->mode != GAVA_PERTURB_INSERTION) return GAVA_EINVAL;
  if (a->baseline_kind != GAVA_BASELINE_ZERO && a->baseline_kind != GAVA_BASELINE_CHANNEL && a->baseline_kind != GAVA_BASELINE_TENSOR)
    return GAVA_EINVAL;
  if ((a->baseline_kind == GAVA_BASELINE_ZERO) != (a->baseline == nullptr)) return GAVA_EINVAL;
  if (((uintptr_t)a->x | (uintptr_t)a->out) & 15) return GAVA_EINVAL;
  if (a->baseline_kind == GAVA_BASELINE_TENSOR && ((uintptr_t)a->baseline & 15)) return GAVA_EINVAL;
  if (((uintptr_t)a->ranks | (uintptr_t)a->baseline) & 3) return GAVA_EINVAL;
  for (int s = 0; s < a->n_steps; ++s)
    if (a->k[s] < 0 || (s && a->k[s] < a->k[s - 1])) return GAVA_EINVAL;
  PerturbParams p;
  p.x = (const unsigned*)a->x; p.ranks = a->ranks; p.baseline = (const unsigned*)a->baseline; p.out = (unsigned*)a->out;
  p.T = a->T; p.size = a->size; p.patch = a->patch; p.g = a->size / a->patch;
  p.frame_units = a->units == GAVA_UNITS_FRAME; p.insertion = a->mode == GAVA_PERTURB_INSERTION;
  p.kind = a->baseline_kind; p.n_steps = a->n_steps;
  for (int s = 0; s < a->n_steps; ++s) p.k[s] = a->k[s];
  for (int s = a->n_steps; s < GAVA_PERTURB_MAX_STEPS; ++s) p.k[s] = 0;
  const long floats = 3L * a->nb * a->T * a->size * a->size;
  // a vector must not straddle two patches, and every row (size floats) must start on a vector boundary: VEC | patch is both
  const int vec = a->patch % 4 == 0 ? 4 : a->patch % 2 == 0 ? 2 : 1;
  p.items = floats / vec;
  hipStream_t s = (hipStream_t)stream;
  if (vec == 4) launch_perturb<4>(p, s);
  else if (vec == 2) launch_perturb<2>(p, s);
  else launch_perturb<1>(p, s);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_perturb_scores(const gava_perturb_scores_args* a, gava_stream_t stream) {
  if (!a || !a->logits || !a->logit || !a->prob || !a->top1 || !a->auc_logit || !a->auc_prob || !a->target_out) return GAVA_EINVAL;
  if (a->nb < 1 || a->C < 1 || a->ld < a->C) return GAVA_EINVAL;
  if (a->n_steps < 1 || a->n_steps > GAVA_PERTURB_MAX_STEPS || a->ref_step < 0 || a->ref_step >= a->n_steps) return GAVA_EINVAL;
  ScoreParams p;
  p.logits = a->logits; p.ld = (long)a->ld; p.target = (const long long*)a->target;
  p.logit = a->logit; p.prob = a->prob; p.top1 = a->top1; p.auc_logit = a->auc_logit; p.auc_prob = a->auc_prob;
  p.target_out = (long long*)a->target_out;
  p.n_steps = a->n_steps; p.C = a->C; p.ref_step = a->ref_step;
  for (int s = 0; s < GAVA_PERTURB_MAX_STEPS; ++s) p.fractions[s] = s < a->n_steps ? a->fractions[s] : 0.f;
  hipLaunchKernelGGL(perturb_scores_kernel, dim3((unsigned)a->nb), dim3(PS_THREADS), 0, (hipStream_t)stream, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

extern "C" int gava_perturbation_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_patch_ranks_args), sizeof(gava_blur_clips_args), sizeof(gava_perturb_clips_args),
                          sizeof(gava_perturb_scores_args)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
