// attention_relevance.hip — one step of gradient-weighted attention relevance (Chefer et al., self-attention rule):
//   out[f][h][j] = sum_{i < n_q} w[f][i] * max(0, P_h[i][j] * G_h[i][j])       j in [0, n_kmain)
// with P = softmax_j(q_i . k_j) over ALL keys of the block (the frame's own rows and its prompt rows, the probabilities the
// forward used) and G_h[i][j] = dout_i(head h) . v_j(head h) = d s / d P_h[i][j] (see gava_attention_relevance_args).
//
// The shape is attention_maps.hip's: one 4-wave workgroup per (frame, head), K of the head in LDS (128-byte rows, 16-byte
// chunks XOR-swizzled by row & 6, up to 640 keys), scores as MFMA products S^T = K Q^T with the KEY on the MFMA row, so that a
// lane holds, for its own query (lane & 15), four consecutive keys of a 16-key tile.  Phases A1 / A2 give every query its row
// maximum and row sum over all keys; (M_i log2 e, c_i = w_i / row sum) goes to LDS, padding queries carry c_i = 0.  Phase B
// walks blocks of four key tiles of the frame's OWN keys (the prompt rows' columns are not asked for): the K fragments and the
// V fragments of the block stay in registers - V comes straight from global memory, it never needs LDS -, the wave walks all
// query tiles in ascending order and forms two products per tile, S^T = K Q^T and G^T = V dO^T (the same layout, V in K's
// place, dO in Q's), then adds c_i * max(0, exp2(...) * g) into four accumulators per tile and lane.  The clamp is applied
// before the weight, so a negative w_i is honoured.  The sixteen lanes that share a key column are added by a fixed xor
// butterfly (8, 4, 2, 1) and one lane stores: every output element is summed by one wave in one order, no atomics, the same
// bits on every run.  Nothing is rounded to 16 bits after the MFMAs.
// PA is the storage type of q / k / v (the kept activations), PG that of dout: the scores are PA products on the stored bits,
// V is converted to PG as it is loaded (what gava_attention_backward does with it) and G is a PG product.
#include <type_traits>
#include "common.h"
#include "internal.h"

namespace {

constexpr int LDS_ROW = 128;
constexpr int NWV = 4;            // waves per workgroup
constexpr int KB = 4;             // key tiles a wave holds in registers in phase B
constexpr int MAX_KEYS = 640;
constexpr float LOG2E = 1.4426950408889634f;

struct RelParams {
  const unsigned short* q; const unsigned short* k; const unsigned short* v; long ld;
  const unsigned short* sk; long lds;
  const unsigned short* dout; long ldd;
  const float* w; float* out;
  int batch, heads, n_q, n_kmain, n_g, T, n_keys;
  int qbr; long ldq;
};

template <class PA, class PG>
__device__ __forceinline__ s16x8_t load_v8(const unsigned short* p) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  if constexpr (!std::is_same<PA, PG>::value) {
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = PG::cvt2(PA::up((unsigned short)w[e]), PA::up((unsigned short)(w[e] >> 16)));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return __builtin_bit_cast(s16x8_t, v);
}

template <class P>
__device__ __forceinline__ f32x4_t scores(const char* krow, unsigned k0, unsigned k1, s16x8_t q0, s16x8_t q1) {
  const s16x8_t a0 = *reinterpret_cast<const s16x8_t*>(krow + k0);
  const s16x8_t a1 = *reinterpret_cast<const s16x8_t*>(krow + k1);
  f32x4_t s = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  s = P::mfma(a0, q0, s);
  return P::mfma(a1, q1, s);
}

template <class PA, class PG, int NKT>
__global__ __launch_bounds__(256) void attention_relevance_kernel(const RelParams p) {
  constexpr int KP = NKT * 16;
  __shared__ __attribute__((aligned(16))) char Ks[KP * LDS_ROW];
  __shared__ float2 stats[KP];                       // n_q <= n_kmain <= KP, rounded up to whole tiles
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x / p.heads, h = blockIdx.x - n * p.heads;
  const int fr = lane & 15, fg = lane >> 4;
  const int n_qt = (p.n_q + 15) >> 4, n_kt = (p.n_keys + 15) >> 4, n_mt = (p.n_kmain + 15) >> 4;

  // ---- stage K: rows past n_keys hold key 0 (finite; their scores are masked)
  for (int id = tid; id < n_kt * 16 * 8; id += NWV * 64) {
    const int row = id >> 3, c = id & 7;
    const gava::KeyRowSrc src = gava::key_row_src(n, row, p.n_kmain, p.n_keys, p.n_g, p.T, p.batch);
    const unsigned short* g = (src.is_main ? p.k + src.row * p.ld : p.sk + src.row * p.lds) + h * 64 + c * 8;
    *reinterpret_cast<uint4*>(Ks + row * LDS_ROW + ((c ^ (row & 6)) << 4)) = *reinterpret_cast<const uint4*>(g);
  }
  __syncthreads();

  const unsigned k0 = fr * LDS_ROW + ((fg ^ (fr & 6)) << 4), k1 = fr * LDS_ROW + (((fg + 4) ^ (fr & 6)) << 4);
  auto q_row = [&](int qt) {
    const int qi = qt * 16 + fr;
    return (long)n * p.qbr + (qi < p.n_q ? qi : p.n_q - 1);      // a padding query reads the last one; its weight is 0
  };

  // ---- A: per query the maximum and the row sum over all keys
  for (int qt = wave; qt < n_qt; qt += NWV) {
    const unsigned short* qp = p.q + q_row(qt) * p.ldq + h * 64 + 8 * fg;
    const s16x8_t q0 = *reinterpret_cast<const s16x8_t*>(qp), q1 = *reinterpret_cast<const s16x8_t*>(qp + 32);
    float mx = -INFINITY;
    for (int kt = 0; kt < n_kt; ++kt) {
      const f32x4_t s = scores<PA>(Ks + kt * 16 * LDS_ROW, k0, k1, q0, q1);
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, kt * 16 + 4 * fg + r < p.n_keys ? s[r] : -INFINITY);
    }
    mx = max_across_lane_groups(mx);                 // key 0 is always valid: finite
    const float m2 = mx * LOG2E;
    float sum = 0.f;
    for (int kt = 0; kt < n_kt; ++kt) {
      const f32x4_t s = scores<PA>(Ks + kt * 16 * LDS_ROW, k0, k1, q0, q1);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sum += kt * 16 + 4 * fg + r < p.n_keys ? __builtin_amdgcn_exp2f(fmaf(s[r], LOG2E, -m2)) : 0.f;
    }
    sum = sum_across_lane_groups(sum);
    if (fg == 0) {
      const int qi = qt * 16 + fr;
      const float wq = qi < p.n_q ? (p.w ? p.w[(long)n * p.n_q + qi] : 1.f) : 0.f;
      stats[qt * 16 + fr] = make_float2(m2, wq / sum);
    }
  }
  __syncthreads();

  // ---- B: column sums over the queries, KB tiles of the frame's own keys at a time
  float* orow = p.out + ((long)n * p.heads + h) * p.n_kmain;
  for (int kb = wave * KB; kb < n_mt; kb += NWV * KB) {
    s16x8_t kf[KB][2], vf[KB][2];
    f32x4_t acc[KB];
#pragma unroll
    for (int t = 0; t < KB; ++t) {
      const int kt = kb + t < n_mt ? kb + t : n_mt - 1;          // a tile past the end repeats the last one and stores nothing
      kf[t][0] = *reinterpret_cast<const s16x8_t*>(Ks + kt * 16 * LDS_ROW + k0);
      kf[t][1] = *reinterpret_cast<const s16x8_t*>(Ks + kt * 16 * LDS_ROW + k1);
      const int key = kt * 16 + fr;                              // a key past the frame's own reads its last one and is not stored
      const unsigned short* vp = p.v + ((long)n * p.n_kmain + (key < p.n_kmain ? key : p.n_kmain - 1)) * p.ld + h * 64 + 8 * fg;
      vf[t][0] = load_v8<PA, PG>(vp);
      vf[t][1] = load_v8<PA, PG>(vp + 32);
      acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    for (int qt = 0; qt < n_qt; ++qt) {
      const long row = q_row(qt);
      const unsigned short* qp = p.q + row * p.ldq + h * 64 + 8 * fg;
      const unsigned short* dp = p.dout + row * p.ldd + h * 64 + 8 * fg;
      const s16x8_t q0 = *reinterpret_cast<const s16x8_t*>(qp), q1 = *reinterpret_cast<const s16x8_t*>(qp + 32);
      const s16x8_t d0 = *reinterpret_cast<const s16x8_t*>(dp), d1 = *reinterpret_cast<const s16x8_t*>(dp + 32);
      const float2 st = stats[qt * 16 + fr];
#pragma unroll
      for (int t = 0; t < KB; ++t) {
        f32x4_t s = (f32x4_t){0.f, 0.f, 0.f, 0.f}, g = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        s = PA::mfma(kf[t][0], q0, s);
        s = PA::mfma(kf[t][1], q1, s);
        g = PG::mfma(vf[t][0], d0, g);
        g = PG::mfma(vf[t][1], d1, g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[t][r] = fmaf(fmaxf(__builtin_amdgcn_exp2f(fmaf(s[r], LOG2E, -st.x)) * g[r], 0.f), st.y, acc[t][r]);
      }
    }
#pragma unroll
    for (int t = 0; t < KB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[t][r];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 1, 64);
        const int j = (kb + t) * 16 + 4 * fg + r;
        if (fr == 0 && kb + t < n_mt && j < p.n_kmain) orow[j] = v;
      }
  }
}

template <class PA, class PG>
int launch_relevance(const RelParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((long)p.batch * p.heads)), block(NWV * 64);
  const int tiles = (p.n_keys + 15) >> 4;
  if (tiles <= 4) hipLaunchKernelGGL((attention_relevance_kernel<PA, PG, 4>), grid, block, 0, s, p);
  else if (tiles <= 14) hipLaunchKernelGGL((attention_relevance_kernel<PA, PG, 14>), grid, block, 0, s, p);
  else if (tiles <= 26) hipLaunchKernelGGL((attention_relevance_kernel<PA, PG, 26>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((attention_relevance_kernel<PA, PG, MAX_KEYS / 16>), grid, block, 0, s, p);
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

}  // namespace

extern "C" int gava_attention_relevance(const gava_attention_relevance_args* a, gava_stream_t stream) {
  if (!a || !a->q || !a->k || !a->v || !a->dout || !a->out) return GAVA_EINVAL;
  if (a->batch <= 0 || a->heads <= 0 || a->n_q <= 0 || a->n_kmain <= 0) return GAVA_EINVAL;
  if ((long)a->batch * a->heads > 0x7fffffffL) return GAVA_EINVAL;
  if (a->ld_qkv % 8 || a->ld_qkv < (int64_t)a->heads * 64) return GAVA_EINVAL;
  if (a->ld_dout % 8 || a->ld_dout < (int64_t)a->heads * 64) return GAVA_EINVAL;
  if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->dout) & 15) return GAVA_EINVAL;
  if (((uintptr_t)a->out | (uintptr_t)a->w) & 3) return GAVA_EINVAL;
  int n_side = 0;
  if (a->n_g || a->T || a->has_summary) {
    if (!a->side_k || a->ld_side % 8 || a->ld_side < (int64_t)a->heads * 64 || a->n_g < 0 || a->T <= 0) return GAVA_EINVAL;
    if ((uintptr_t)a->side_k & 15) return GAVA_EINVAL;
    if (a->batch % a->T) return GAVA_EINVAL;
    n_side = a->n_g + a->T + (a->has_summary ? 1 : 0);
  }
  if ((long)a->n_kmain + n_side > MAX_KEYS) return GAVA_EINVAL;   // K of one (frame, head) is resident in LDS
  if (a->n_q > a->n_kmain) return GAVA_EINVAL;                    // queries are rows of the frame itself
  RelParams p;
  p.q = (const unsigned short*)a->q; p.k = (const unsigned short*)a->k; p.v = (const unsigned short*)a->v; p.ld = a->ld_qkv;
  p.sk = (const unsigned short*)a->side_k; p.lds = a->ld_side;
  p.dout = (const unsigned short*)a->dout; p.ldd = a->ld_dout;
  p.w = a->w; p.out = a->out;
  p.batch = a->batch; p.heads = a->heads; p.n_q = a->n_q; p.n_kmain = a->n_kmain;
  p.n_g = a->n_g; p.T = n_side ? a->T : 1;
  p.n_keys = a->n_kmain + n_side;
  p.qbr = a->q_batch_rows > 0 ? a->q_batch_rows : a->n_q;
  p.ldq = a->ld_q > 0 ? a->ld_q : a->ld_qkv;
  if (p.ldq % 8 || p.ldq < (int64_t)a->heads * 64 || p.qbr < a->n_q) return GAVA_EINVAL;
  const int act = a->act_prec_set ? a->act_prec : a->prec;
  hipStream_t s = (hipStream_t)stream;
  if (a->prec == GAVA_PREC_F16 && act == GAVA_PREC_F16) return launch_relevance<PrecF16, PrecF16>(p, s);
  if (a->prec == GAVA_PREC_BF16 && act == GAVA_PREC_BF16) return launch_relevance<PrecBF16, PrecBF16>(p, s);
  if (a->prec == GAVA_PREC_BF16 && act == GAVA_PREC_F16) return launch_relevance<PrecF16, PrecBF16>(p, s);   // fp16 forward, bf16 gradients
  return GAVA_EINVAL;
}

extern "C" int gava_attention_relevance_struct_sizes(size_t* out, int cap) {
  const size_t sizes[] = {sizeof(gava_attention_relevance_args)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
  return n;
}
