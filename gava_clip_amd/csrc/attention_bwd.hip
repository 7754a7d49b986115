// attention_bwd.hip — MFMA backward of softmax(Q K^T) V, head dim 64: the vision-block attention (the frame's rows +
// the gathered prompt rows), the T-token summary attention and the causal text attention, built from the same pieces as
// attention.hip:
//   S^T = K Q^T accumulators ARE the B operand of the next product, transposed operands come from the
//   hardware-transposing LDS read, 160-byte padded LDS rows, one workgroup (4 waves) per (frame, head).
// Two kernels (the two contraction directions need the score tile in the two orientations):
//   1. attn_bwd_dq_kernel   per 16-query tile: S^T = K Q^T -> P^T; dP^T = V dO^T; delta = rowsum(P * dP);
//                           dS^T = P^T * (dP^T - delta); dQ^T = K^T dS^T.  Also writes the row statistics
//                           L2[q] = log2(sum_k exp(s_qk)) (+ max) and delta[q] for the second kernel.
//   2. attn_bwd_dkv_kernel  per 16-key tile, looping over query tiles: S = Q K^T, dP = dO V^T (query on the MFMA
//                           row), P = exp2(S*log2e - L2), dS = P * (dP - delta); dV^T += dO^T P, dK^T += Q^T dS with
//                           P / dS again used straight from the accumulators as B operands (contraction over queries).
// Each has a streaming form (attn_bwd_dq_stream_kernel, attn_bwd_dkv_stream_kernel) for the shapes it cannot hold.  The
// four kernels differ in the loop around the tiles and in how the scores and the statistics of a dQ tile are scheduled;
// the tile code itself exists once, in the device functions ahead of them:
//   kv_off                          key row -> K/V or prompt-matrix offset (gava::key_row_src)
//   load_/store_kv_rows, _qo_rows   operand staging: 16-byte pieces to registers, then converted into padded LDS rows
//   read_tr_pair                    the transposed LDS read of a 32-row block
//   dq_accum, dq_store              dQ^T += K^T dS^T for 32 keys; the scaled dQ rows
//   dkv_pair, dkv_store             two query tiles of the dK/dV products; dK/dV rows and the prompt rows' partials
// q is expected pre-scaled by 1/sqrt(dh) (as the forward's QKV GEMM writes it); dq is multiplied by q_scale.
#include "common.h"
#include "internal.h"
#include <type_traits>

namespace {

constexpr int LDS_ROW = 160;  // bytes per row in LDS (64 x 2 B + 32 B pad): conflict-free for b128 and tr_b64 reads
constexpr float LOG2E = 1.4426950408889634f;

// Activations kept from the forward may be stored in another 16-bit type (PA, e.g. fp16) than the one the gradients
// and the MFMAs use (P, bf16): convert 8 packed values on load.  PA == P compiles to nothing.
template <class PA, class P>
static __device__ __forceinline__ uint4 to_p(uint4 v) {
  if constexpr (std::is_same<PA, P>::value) {
    return v;
  } else {
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = P::cvt2(PA::up((unsigned short)w[e]), PA::up((unsigned short)(w[e] >> 16)));
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
}
template <class PA, class P>
static __device__ __forceinline__ s16x8_t load_act8(const unsigned short* p) {
  return __builtin_bit_cast(s16x8_t, to_p<PA, P>(*reinterpret_cast<const uint4*>(p)));
}

// Element offset of head h of key row `key` of frame n, in k / v (is_main) or in sk / sv; keys past n_keys read key 0
static __device__ __forceinline__ long kv_off(const gava::AttnBwdMfmaParams& p, int n, int h, int key, bool& is_main) {
  const gava::KeyRowSrc src = gava::key_row_src(n, key, p.n_kmain, p.n_keys, p.n_g, p.T, p.batch);
  is_main = src.is_main;
  return src.row * (src.is_main ? p.ld_qkv : p.ld_side) + h * 64;
}

// ---- Operand staging.  The 16-byte pieces of ROWS rows (8 per row) are dealt to the 256 threads, in two phases so that a
// block's global loads can be in flight under the block before it: load_* fills registers, store_* converts and writes the
// padded LDS rows, zero past the end of the operand.
constexpr int pieces(int rows) { return (rows * 8 + 255) / 256; }

template <class PA, class P>
static __device__ __forceinline__ void store_piece(char* dst, int row, int chunk, bool ok, uint4 v) {
  *reinterpret_cast<uint4*>(dst + row * LDS_ROW + chunk * 16) = ok ? to_p<PA, P>(v) : make_uint4(0, 0, 0, 0);
}

// keys key0 .. key0 + ROWS - 1 of K and V (prompt rows gathered)
template <int ROWS>
static __device__ __forceinline__ void load_kv_rows(const gava::AttnBwdMfmaParams& p, int n, int h, int key0, int tid,
                                                    uint4 (&kv)[pieces(ROWS)], uint4 (&vv)[pieces(ROWS)]) {
#pragma unroll
  for (int it = 0; it < pieces(ROWS); ++it) {
    const int id = tid + it * 256;
    bool is_main;
    const long off = kv_off(p, n, h, key0 + (id >> 3), is_main) + (id & 7) * 8;
    kv[it] = *reinterpret_cast<const uint4*>((is_main ? p.k : p.sk) + off);
    vv[it] = *reinterpret_cast<const uint4*>((is_main ? p.v : p.sv) + off);
  }
}
template <class PA, class P, int ROWS>
static __device__ __forceinline__ void store_kv_rows(const gava::AttnBwdMfmaParams& p, int key0, int tid, char* Ks, char* Vs,
                                                     const uint4 (&kv)[pieces(ROWS)], const uint4 (&vv)[pieces(ROWS)]) {
#pragma unroll
  for (int it = 0; it < pieces(ROWS); ++it) {
    const int id = tid + it * 256;
    const int row = id >> 3, chunk = id & 7;
    if (ROWS % 32 == 0 || id < ROWS * 8) {
      const bool ok = key0 + row < p.n_keys;
      store_piece<PA, P>(Ks, row, chunk, ok, kv[it]);
      store_piece<PA, P>(Vs, row, chunk, ok, vv[it]);
    }
  }
}

// queries q0 .. q0 + ROWS - 1 of Q and dO with their row statistics; a padded query gets L2 = +inf, so that its P = 0
template <int ROWS>
struct QoRows {
  uint4 q[pieces(ROWS)], o[pieces(ROWS)];
  float l2[(ROWS + 255) / 256], dl[(ROWS + 255) / 256];
};
template <int ROWS>
static __device__ __forceinline__ void load_qo_rows(const gava::AttnBwdMfmaParams& p, int n, int h, int q0, int tid, QoRows<ROWS>& r) {
#pragma unroll
  for (int it = 0; it < pieces(ROWS); ++it) {
    const int id = tid + it * 256;
    const int row = q0 + (id >> 3), chunk = id & 7;
    const int rowc = row < p.n_q ? row : 0;
    r.q[it] = *reinterpret_cast<const uint4*>(p.q + ((long)n * p.q_rows + rowc) * p.ld_q + h * 64 + chunk * 8);
    r.o[it] = *reinterpret_cast<const uint4*>(p.dout + ((long)n * p.q_rows + rowc) * p.ld_dout + h * 64 + chunk * 8);
  }
#pragma unroll
  for (int it = 0; it < (ROWS + 255) / 256; ++it) {
    const int qx = q0 + tid + it * 256;
    if (tid + it * 256 < ROWS) {
      const float* st = p.stats + ((long)blockIdx.x * p.q_pad + (qx < p.n_q ? qx : 0)) * 2;
      r.l2[it] = st[0]; r.dl[it] = st[1];
    }
  }
}
template <class PA, class P, int ROWS>
static __device__ __forceinline__ void store_qo_rows(const gava::AttnBwdMfmaParams& p, int q0, int tid, char* Qs, char* Os,
                                                     float* L2s, float* Dls, const QoRows<ROWS>& r) {
#pragma unroll
  for (int it = 0; it < pieces(ROWS); ++it) {
    const int id = tid + it * 256;
    const int row = id >> 3, chunk = id & 7;
    if (ROWS % 32 == 0 || id < ROWS * 8) {
      const bool ok = q0 + row < p.n_q;
      store_piece<PA, P>(Qs, row, chunk, ok, r.q[it]);
      store_piece<P, P>(Os, row, chunk, ok, r.o[it]);
    }
  }
#pragma unroll
  for (int it = 0; it < (ROWS + 255) / 256; ++it) {
    const int qx = tid + it * 256;
    if (qx < ROWS) {
      const bool ok = q0 + qx < p.n_q;
      L2s[qx] = ok ? r.l2[it] : INFINITY;
      Dls[qx] = ok ? r.dl[it] : 0.f;
    }
  }
}

// ---- Tile code.  fr = lane & 15, fg = lane >> 4 throughout.
// Rows 0..31 of a padded LDS block, transposed: for dt = 0..3, {t0[dt], t1[dt]} is the A operand holding columns
// dt*16 .. dt*16 + 15 (on the MFMA row) against the 32 rows (contraction)
static __device__ __forceinline__ void read_tr_pair(const char* rows, int fr, int fg, s16x4_t (&t0)[4], s16x4_t (&t1)[4]) {
  const char* b = rows + (4 * fg + (fr >> 2)) * LDS_ROW + (fr & 3) * 8;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    t0[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, b + dt * 32));
    t1[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, b + 16 * LDS_ROW + dt * 32));
  }
}
static __device__ __forceinline__ s16x8_t join(s16x4_t a, s16x4_t b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
// two accumulator tiles (fp32, the same 4 rows of the lane in each) -> the 16-bit B operand of a 32-deep contraction
template <class P>
static __device__ __forceinline__ s16x8_t pack_pair(f32x4_t a, f32x4_t b) {
  const uint2 lo = pack4<P>(a[0], a[1], a[2], a[3]), hi = pack4<P>(b[0], b[1], b[2], b[3]);
  return __builtin_bit_cast(s16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
}

// Query qi of frame n (clamped to a valid row: a tile beyond n_q computes garbage, stores nothing) as the B operands of the
// dQ kernels' products: q0, q1 / g0, g1 = head dims 8*fg.. and 32 + 8*fg.. of its Q / dO row.  The query-side buffers
// (q, dout, dq) hold q_rows rows per frame.
template <class PA, class P>
static __device__ __forceinline__ void load_q_frags(const gava::AttnBwdMfmaParams& p, int n, int h, int qi, int fg,
                                                    s16x8_t& q0, s16x8_t& q1, s16x8_t& g0, s16x8_t& g1) {
  const long row = (long)n * p.q_rows + (qi < p.n_q ? qi : p.n_q - 1);
  const unsigned short* qp = p.q + row * p.ld_q + h * 64 + 8 * fg;
  const unsigned short* gp = p.dout + row * p.ld_dout + h * 64 + 8 * fg;
  q0 = load_act8<PA, P>(qp); q1 = load_act8<PA, P>(qp + 32);
  g0 = *reinterpret_cast<const s16x8_t*>(gp); g1 = *reinterpret_cast<const s16x8_t*>(gp + 32);
}

// dQ^T += K^T dS^T over 32 keys: t0 / t1 = read_tr_pair of their K rows, ds0 / ds1 = dS^T of the two 16-key tiles (exactly
// the forward's O^T = V^T P^T with K for V)
template <class P>
static __device__ __forceinline__ void dq_accum(const s16x4_t (&t0)[4], const s16x4_t (&t1)[4], f32x4_t ds0, f32x4_t ds1, f32x4_t (&o)[4]) {
  const s16x8_t df = pack_pair<P>(ds0, ds1);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = P::mfma(join(t0[dt], t1[dt]), df, o[dt]);
}
// o[dt][r] = dQ[query qi][d = dt*16 + 4*fg + r], before the scale
template <class P>
static __device__ __forceinline__ void dq_store(const gava::AttnBwdMfmaParams& p, int n, int h, int qi, int fg, const f32x4_t (&o)[4]) {
  unsigned short* dq = p.dq + ((long)n * p.q_rows + qi) * p.ld_dq + h * 64 + 4 * fg;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<uint2*>(dq + dt * 16) = pack4<P>(o[dt][0] * p.q_scale, o[dt][1] * p.q_scale, o[dt][2] * p.q_scale, o[dt][3] * p.q_scale);
}

// Query tiles 2c, 2c+1 of the block in Qs / Os / L2s / Dls (the first of their queries is query q_first of the problem:
// the causal test) against the lane's key: kb0, kb1 / vb0, vb1 are its K / V rows as B operands (head dims 8*fg.. and
// 32 + 8*fg..).  S = Q K^T, dP = dO V^T: lane holds key fr, queries t*16 + 4*fg + r; then dV^T += dO^T P, dK^T += Q^T dS.
template <class P, bool CAUSAL>
static __device__ __forceinline__ void dkv_pair(const char* Qs, const char* Os, const float* L2s, const float* Dls, int c, int q_first,
                                                int fr, int fg, s16x8_t kb0, s16x8_t kb1, s16x8_t vb0, s16x8_t vb1, int key, bool key_ok,
                                                f32x4_t (&dk)[4], f32x4_t (&dv)[4]) {
  f32x4_t st[2], pt[2];
  s16x4_t oT0[4], oT1[4], qT0[4], qT1[4];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ro = ((2 * c + t) * 16 + fr) * LDS_ROW + fg * 16;
    const s16x8_t qa0 = *reinterpret_cast<const s16x8_t*>(Qs + ro), qa1 = *reinterpret_cast<const s16x8_t*>(Qs + ro + 64);
    const s16x8_t oa0 = *reinterpret_cast<const s16x8_t*>(Os + ro), oa1 = *reinterpret_cast<const s16x8_t*>(Os + ro + 64);
    f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f}, b = a;
    a = P::mfma(qa0, kb0, a);
    a = P::mfma(qa1, kb1, a);
    b = P::mfma(oa0, vb0, b);
    b = P::mfma(oa1, vb1, b);
    st[t] = a;
    pt[t] = b;
  }
  read_tr_pair(Os + c * 32 * LDS_ROW, fr, fg, oT0, oT1);
  read_tr_pair(Qs + c * 32 * LDS_ROW, fr, fg, qT0, qT1);
  f32x4_t pv[2], dsv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 l2 = *reinterpret_cast<const float4*>(L2s + (2 * c + t) * 16 + 4 * fg);
    const float4 dl = *reinterpret_cast<const float4*>(Dls + (2 * c + t) * 16 + 4 * fg);
    const float l2a[4] = {l2.x, l2.y, l2.z, l2.w}, dla[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool vis = key_ok && (!CAUSAL || key <= q_first + t * 16 + 4 * fg + r);
      const float pr = vis ? __builtin_amdgcn_exp2f(fmaf(st[t][r], LOG2E, -l2a[r])) : 0.f;
      pv[t][r] = pr;
      dsv[t][r] = pr * (pt[t][r] - dla[r]);
    }
  }
  const s16x8_t pf = pack_pair<P>(pv[0], pv[1]), df = pack_pair<P>(dsv[0], dsv[1]);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    dv[dt] = P::mfma(join(oT0[dt], oT1[dt]), pf, dv[dt]);
    dk[dt] = P::mfma(join(qT0[dt], qT1[dt]), df, dk[dt]);
  }
}
// dk[dt][r] = dK[key][d = dt*16 + 4*fg + r]: 16-bit rows for the frame's own keys; for a shared prompt row the fp32 per-frame
// partial (the caller sums over the frames sharing it)
template <class P>
static __device__ __forceinline__ void dkv_store(const gava::AttnBwdMfmaParams& p, int n, int h, int key, int fg, bool is_main,
                                                 const f32x4_t (&dk)[4], const f32x4_t (&dv)[4]) {
  if (is_main) {
    const long row = (long)n * p.n_kmain + key;
    unsigned short* ok_ = p.dk + row * p.ld_dqkv + h * 64 + 4 * fg;
    unsigned short* ov_ = p.dv + row * p.ld_dqkv + h * 64 + 4 * fg;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *reinterpret_cast<uint2*>(ok_ + dt * 16) = pack4<P>(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
      *reinterpret_cast<uint2*>(ov_ + dt * 16) = pack4<P>(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
    }
  } else {
    const long row = (long)n * (p.n_keys - p.n_kmain) + (key - p.n_kmain);
    float* ok_ = p.dsk + row * p.ld_dside + h * 64 + 4 * fg;
    float* ov_ = p.dsv + row * p.ld_dside + h * 64 + 4 * fg;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *reinterpret_cast<float4*>(ok_ + dt * 16) = make_float4(dk[dt][0], dk[dt][1], dk[dt][2], dk[dt][3]);
      *reinterpret_cast<float4*>(ov_ + dt * 16) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
    }
  }
}

template <class P, class PA, int NKT, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const gava::AttnBwdMfmaParams p) {
  constexpr int KP = NKT * 16;
  __shared__ __attribute__((aligned(16))) char smem[2 * KP * LDS_ROW];
  char* Ks = smem;
  char* Vs = smem + KP * LDS_ROW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x / p.heads, h = blockIdx.x - n * p.heads;
  const int fr = lane & 15, fg = lane >> 4;
  const int n_qt = (p.n_q + 15) >> 4;

  // ---- stage K, V (prompt rows gathered), zero rows beyond n_keys
  {
    uint4 kv[pieces(KP)], vv[pieces(KP)];
    load_kv_rows<KP>(p, n, h, 0, tid, kv, vv);
    store_kv_rows<PA, P, KP>(p, 0, tid, Ks, Vs, kv, vv);
  }
  __syncthreads();

  for (int qt = wave; qt < n_qt; qt += 4) {
    const int qi = qt * 16 + fr;
    s16x8_t q0, q1, g0, g1;
    load_q_frags<PA, P>(p, n, h, qi, fg, q0, q1, g0, g1);

    // S^T = K Q^T and dP^T = V dO^T: lane holds, for its query fr, keys kt*16 + 4*fg + r
    f32x4_t s[NKT], dp[NKT];
    constexpr int QCH = NKT <= 7 ? NKT : (NKT % 7 == 0 ? 7 : (NKT % 5 == 0 ? 5 : 2));
    // two passes (K then V) so that only one chunk of fragments is live beside the 2 x NKT accumulators
#pragma unroll
    for (int c0 = 0; c0 < NKT; c0 += QCH) {
      s16x8_t kf[QCH][2];
#pragma unroll
      for (int t = 0; t < QCH; ++t) {
        const int ro = ((c0 + t) * 16 + fr) * LDS_ROW + fg * 16;
        kf[t][0] = *reinterpret_cast<const s16x8_t*>(Ks + ro);
        kf[t][1] = *reinterpret_cast<const s16x8_t*>(Ks + ro + 64);
      }
#pragma unroll
      for (int t = 0; t < QCH; ++t) {
        f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        a = P::mfma(kf[t][0], q0, a);
        a = P::mfma(kf[t][1], q1, a);
        s[c0 + t] = a;
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * QCH, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * QCH, 0);
    }
#pragma unroll
    for (int c0 = 0; c0 < NKT; c0 += QCH) {
      s16x8_t vf[QCH][2];
#pragma unroll
      for (int t = 0; t < QCH; ++t) {
        const int ro = ((c0 + t) * 16 + fr) * LDS_ROW + fg * 16;
        vf[t][0] = *reinterpret_cast<const s16x8_t*>(Vs + ro);
        vf[t][1] = *reinterpret_cast<const s16x8_t*>(Vs + ro + 64);
      }
#pragma unroll
      for (int t = 0; t < QCH; ++t) {
        f32x4_t b = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        b = P::mfma(vf[t][0], g0, b);
        b = P::mfma(vf[t][1], g1, b);
        dp[c0 + t] = b;
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * QCH, 1);
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * QCH, 1);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt * 16 + 16 > p.n_keys || (CAUSAL && kt * 16 + 15 > qt * 16)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + 4 * fg + r;
          s[kt][r] = (key < p.n_keys && (!CAUSAL || key <= qi)) ? s[kt][r] : -INFINITY;
        }
      }
      mx = fmaxf(fmaxf(mx, s[kt][0]), fmaxf(s[kt][1], fmaxf(s[kt][2], s[kt][3])));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mneg = -mx * LOG2E;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][r], LOG2E, mneg));
        s[kt][r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(sum);
    float delta = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] *= inv;                       // P
        delta += s[kt][r] * dp[kt][r];
      }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
    if (fg == 0 && qi < p.n_q) {
      float* st = p.stats + ((long)blockIdx.x * p.q_pad + qi) * 2;
      st[0] = mx * LOG2E + __builtin_amdgcn_logf(sum);   // log2(sum_k exp(s_k)): P = exp2(s*log2e - L2)
      st[1] = delta;
    }
    // dS^T = P^T * (dP^T - delta), then dQ^T += K^T dS^T, the K^T reads a batch of PCH 32-key chunks ahead
    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    constexpr int NC2 = NKT / 2;
    constexpr int PCH = NC2 % 7 == 0 ? 7 : (NC2 % 5 == 0 ? 5 : (NC2 % 3 == 0 ? 3 : 1));
#pragma unroll
    for (int b0 = 0; b0 < NC2; b0 += PCH) {
      s16x4_t t0[PCH][4], t1[PCH][4];
#pragma unroll
      for (int c = 0; c < PCH; ++c) read_tr_pair(Ks + (b0 + c) * 32 * LDS_ROW, fr, fg, t0[c], t1[c]);
#pragma unroll
      for (int c = 0; c < PCH; ++c) {
        const int cc = b0 + c;
        f32x4_t ds[2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ds[0][r] = s[2 * cc][r] * (dp[2 * cc][r] - delta);
          ds[1][r] = s[2 * cc + 1][r] * (dp[2 * cc + 1][r] - delta);
        }
        dq_accum<P>(t0[c], t1[c], ds[0], ds[1], o);
      }
    }
    if (qi < p.n_q) dq_store<P>(p, n, h, qi, fg, o);
  }
}

template <class P, class PA, int NQT, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const gava::AttnBwdMfmaParams p) {
  static_assert(NQT % 2 == 0, "query tiles are consumed in pairs (32-deep MFMA contraction)");
  constexpr int QP = NQT * 16;
  __shared__ __attribute__((aligned(16))) char smem[2 * QP * LDS_ROW + 2 * QP * sizeof(float)];
  char* Qs = smem;
  char* Os = smem + QP * LDS_ROW;
  float* L2s = reinterpret_cast<float*>(smem + 2 * QP * LDS_ROW);
  float* Dls = L2s + QP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x / p.heads, h = blockIdx.x - n * p.heads;
  const int fr = lane & 15, fg = lane >> 4;
  const int n_kt = (p.n_keys + 15) >> 4;
  // ---- stage Q, dO (zero rows beyond n_q) and the row statistics (P = 0 for padded queries)
  {
    QoRows<QP> r;
    load_qo_rows<QP>(p, n, h, 0, tid, r);
    store_qo_rows<PA, P, QP>(p, 0, tid, Qs, Os, L2s, Dls, r);
  }
  __syncthreads();

  for (int kt = wave; kt < n_kt; kt += 4) {
    const int key = kt * 16 + fr;
    const bool key_ok = key < p.n_keys;
    bool is_main;
    const long koff = kv_off(p, n, h, key, is_main) + 8 * fg;
    const unsigned short* kp = (is_main ? p.k : p.sk) + koff;
    const unsigned short* vp = (is_main ? p.v : p.sv) + koff;
    // B operands: this lane's key, head dims 8*fg.. and 32 + 8*fg..
    const s16x8_t kb0 = load_act8<PA, P>(kp), kb1 = load_act8<PA, P>(kp + 32);
    const s16x8_t vb0 = load_act8<PA, P>(vp), vb1 = load_act8<PA, P>(vp + 32);
    f32x4_t dv[4], dk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dv[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; dk[dt] = dv[dt]; }

#pragma unroll 1
    for (int c = 0; c < NQT / 2; ++c) dkv_pair<P, CAUSAL>(Qs, Os, L2s, Dls, c, c * 32, fr, fg, kb0, kb1, vb0, vb1, key, key_ok, dk, dv);
    if (key_ok) dkv_store<P>(p, n, h, key, fg, is_main, dk, dv);
  }
}

// ---------------------------------------------------------------------------------------------
// Streaming forms for the shapes the kernels above cannot hold (non-causal only): more than 320 keys (dQ kernel: all
// scores of a tile in registers) or more than 288 queries (dK/dV kernel: all of Q and dO in LDS).  Each workgroup owns 4
// tiles (one per wave) for the whole walk over the other side, which arrives in blocks of SB rows through LDS (padded
// 160-byte rows as above); the next block's rows are loaded into registers while the current one is computed.
constexpr int SB = 128;

// dQ, keys streamed in two passes over the key blocks:
//   pass 1: S^T and dP^T per block; running max m, sum l = sum exp(s - m) and delta' = sum exp(s - m) dP, both rescaled
//           when m moves; at the end L2 = m log2e + log2 l and delta = delta' / l (the row statistics of the dK/dV kernel)
//   pass 2: S^T and dP^T again, P = exp2(s log2e - L2), dS^T = P^T * (dP^T - delta), dQ^T += K^T dS^T
// so that dS is formed in fp32 and rounded once, as in attn_bwd_dq_kernel.
template <class P, class PA>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_stream_kernel(const gava::AttnBwdMfmaParams p) {
  constexpr int NKT = SB / 16;
  __shared__ __attribute__((aligned(16))) char smem[2 * SB * LDS_ROW];
  char* Ks = smem;
  char* Vs = smem + SB * LDS_ROW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x / p.heads, h = blockIdx.x - n * p.heads;
  const int fr = lane & 15, fg = lane >> 4;
  const int n_qt = (p.n_q + 15) >> 4;
  const int qt = blockIdx.y * 4 + wave;
  const bool active = qt < n_qt;                       // wave-uniform; idle waves still stage and meet the barriers
  const int qi = qt * 16 + fr;
  const int n_kb = (p.n_keys + SB - 1) / SB;

  s16x8_t q0, q1, g0, g1;
  load_q_frags<PA, P>(p, n, h, qi, fg, q0, q1, g0, g1);

  uint4 kv[pieces(SB)], vv[pieces(SB)];
  load_kv_rows<SB>(p, n, h, 0, tid, kv, vv);
  float m = -INFINITY, l = 0.f, dl = 0.f;   // l, dl: this lane's partial sums (its 4 keys per tile)
  float L2 = 0.f, delta = 0.f;
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int it = 0; it < 2 * n_kb; ++it) {
    const int kb = it < n_kb ? it : it - n_kb;
    const bool pass2 = it >= n_kb;
    __syncthreads();                                   // the previous block is read by everyone
    store_kv_rows<PA, P, SB>(p, kb * SB, tid, Ks, Vs, kv, vv);
    __syncthreads();
    if (it + 1 < 2 * n_kb) load_kv_rows<SB>(p, n, h, (it + 1 < n_kb ? it + 1 : it + 1 - n_kb) * SB, tid, kv, vv);   // in flight under this block's work
    if (!active) continue;

    f32x4_t s[NKT], dp[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const int ro = (t * 16 + fr) * LDS_ROW + fg * 16;
      const s16x8_t k0 = *reinterpret_cast<const s16x8_t*>(Ks + ro), k1 = *reinterpret_cast<const s16x8_t*>(Ks + ro + 64);
      const s16x8_t v0 = *reinterpret_cast<const s16x8_t*>(Vs + ro), v1 = *reinterpret_cast<const s16x8_t*>(Vs + ro + 64);
      f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f}, b = a;
      a = P::mfma(k0, q0, a);
      a = P::mfma(k1, q1, a);
      b = P::mfma(v0, g0, b);
      b = P::mfma(v1, g1, b);
      s[t] = a;
      dp[t] = b;
    }
    if (kb * SB + SB > p.n_keys) {                     // the last block: mask the keys past n_keys
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = kb * SB + t * 16 + 4 * fg + r < p.n_keys ? s[t][r] : -INFINITY;
    }
    if (!pass2) {
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < NKT; ++t) bm = fmaxf(fmaxf(bm, s[t][0]), fmaxf(s[t][1], fmaxf(s[t][2], s[t][3])));
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float mn = fmaxf(m, bm);
      const float alpha = m == mn ? 1.f : __builtin_amdgcn_exp2f((m - mn) * LOG2E);
      const float mneg = mn == -INFINITY ? 0.f : -mn * LOG2E;
      m = mn;
      l *= alpha; dl *= alpha;
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(fmaf(s[t][r], LOG2E, mneg));
          l += e;
          dl += e * dp[t][r];
        }
      if (kb == n_kb - 1) {                            // end of pass 1: the row statistics
        float lt = l + __shfl_xor(l, 16, 64);
        lt += __shfl_xor(lt, 32, 64);
        float dt_ = dl + __shfl_xor(dl, 16, 64);
        dt_ += __shfl_xor(dt_, 32, 64);
        L2 = m * LOG2E + __builtin_amdgcn_logf(lt);
        delta = dt_ * __builtin_amdgcn_rcpf(lt);
        if (fg == 0 && qi < p.n_q) {
          float* st = p.stats + ((long)blockIdx.x * p.q_pad + qi) * 2;
          st[0] = L2;
          st[1] = delta;
        }
      }
      continue;
    }
#pragma unroll
    for (int c = 0; c < NKT / 2; ++c) {
      s16x4_t t0[4], t1[4];
      read_tr_pair(Ks + c * 32 * LDS_ROW, fr, fg, t0, t1);
      f32x4_t ds[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ds[0][r] = __builtin_amdgcn_exp2f(fmaf(s[2 * c][r], LOG2E, -L2)) * (dp[2 * c][r] - delta);
        ds[1][r] = __builtin_amdgcn_exp2f(fmaf(s[2 * c + 1][r], LOG2E, -L2)) * (dp[2 * c + 1][r] - delta);
      }
      dq_accum<P>(t0, t1, ds[0], ds[1], o);
    }
  }
  if (active && qi < p.n_q) dq_store<P>(p, n, h, qi, fg, o);
}

// dK/dV, queries streamed: each wave owns one 16-key tile (dK^T, dV^T accumulators in registers) and walks the query blocks;
// per block the same products as attn_bwd_dkv_kernel.  Rows past n_q are zero with L2 = +inf (P = 0).
template <class P, class PA>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_stream_kernel(const gava::AttnBwdMfmaParams p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * SB * LDS_ROW + 2 * SB * sizeof(float)];
  char* Qs = smem;
  char* Os = smem + SB * LDS_ROW;
  float* L2s = reinterpret_cast<float*>(smem + 2 * SB * LDS_ROW);
  float* Dls = L2s + SB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x / p.heads, h = blockIdx.x - n * p.heads;
  const int fr = lane & 15, fg = lane >> 4;
  const int n_kt = (p.n_keys + 15) >> 4;
  const int kt = blockIdx.y * 4 + wave;
  const bool active = kt < n_kt;
  const int n_qb = (p.n_q + SB - 1) / SB;

  QoRows<SB> r;
  load_qo_rows<SB>(p, n, h, 0, tid, r);

  const int key = kt * 16 + fr;
  const bool key_ok = key < p.n_keys;
  bool is_main;
  const long koff = kv_off(p, n, h, key, is_main) + 8 * fg;
  const unsigned short* kp = (is_main ? p.k : p.sk) + koff;
  const unsigned short* vp = (is_main ? p.v : p.sv) + koff;
  const s16x8_t kb0 = load_act8<PA, P>(kp), kb1 = load_act8<PA, P>(kp + 32);
  const s16x8_t vb0 = load_act8<PA, P>(vp), vb1 = load_act8<PA, P>(vp + 32);
  f32x4_t dv[4], dk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dv[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; dk[dt] = dv[dt]; }

  const int tr_off = (4 * fg + (fr >> 2)) * LDS_ROW + (fr & 3) * 8;
  for (int qb = 0; qb < n_qb; ++qb) {
    __syncthreads();                                   // the previous block is read by everyone
    store_qo_rows<PA, P, SB>(p, qb * SB, tid, Qs, Os, L2s, Dls, r);
    __syncthreads();
    if (qb + 1 < n_qb) load_qo_rows<SB>(p, n, h, (qb + 1) * SB, tid, r);   // in flight under this block's work
    if (!active) continue;
    const int nc = (min(SB, p.n_q - qb * SB) + 31) >> 5;   // query-tile pairs of this block that hold a valid query
    // dkv_pair<P, false> written out: called as the function, this loop takes 172 VGPRs instead of 168 and the kernel
    // drops from 3 to 2 waves per SIMD (the same statements; only the inlining differs)
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
      f32x4_t st[2], pt[2];
      s16x4_t oT0[4], oT1[4], qT0[4], qT1[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ro = ((2 * c + t) * 16 + fr) * LDS_ROW + fg * 16;
        const s16x8_t qa0 = *reinterpret_cast<const s16x8_t*>(Qs + ro), qa1 = *reinterpret_cast<const s16x8_t*>(Qs + ro + 64);
        const s16x8_t oa0 = *reinterpret_cast<const s16x8_t*>(Os + ro), oa1 = *reinterpret_cast<const s16x8_t*>(Os + ro + 64);
        f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f}, b = a;
        a = P::mfma(qa0, kb0, a);
        a = P::mfma(qa1, kb1, a);
        b = P::mfma(oa0, vb0, b);
        b = P::mfma(oa1, vb1, b);
        st[t] = a;
        pt[t] = b;
      }
      {
        const char* ob = Os + c * 32 * LDS_ROW + tr_off;
        const char* qb_ = Qs + c * 32 * LDS_ROW + tr_off;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          oT0[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, ob + dt * 32));
          oT1[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, ob + 16 * LDS_ROW + dt * 32));
          qT0[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, qb_ + dt * 32));
          qT1[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, qb_ + 16 * LDS_ROW + dt * 32));
        }
      }
      float pv[8], dsv[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 l2 = *reinterpret_cast<const float4*>(L2s + (2 * c + t) * 16 + 4 * fg);
        const float4 dl = *reinterpret_cast<const float4*>(Dls + (2 * c + t) * 16 + 4 * fg);
        const float l2a[4] = {l2.x, l2.y, l2.z, l2.w}, dla[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = key_ok ? __builtin_amdgcn_exp2f(fmaf(st[t][r], LOG2E, -l2a[r])) : 0.f;
          pv[4 * t + r] = pr;
          dsv[4 * t + r] = pr * (pt[t][r] - dla[r]);
        }
      }
      const uint2 plo = pack4<P>(pv[0], pv[1], pv[2], pv[3]), phi = pack4<P>(pv[4], pv[5], pv[6], pv[7]);
      const uint2 dlo = pack4<P>(dsv[0], dsv[1], dsv[2], dsv[3]), dhi = pack4<P>(dsv[4], dsv[5], dsv[6], dsv[7]);
      const s16x8_t pf = __builtin_bit_cast(s16x8_t, make_uint4(plo.x, plo.y, phi.x, phi.y));
      const s16x8_t df = __builtin_bit_cast(s16x8_t, make_uint4(dlo.x, dlo.y, dhi.x, dhi.y));
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dv[dt] = P::mfma(__builtin_shufflevector(oT0[dt], oT1[dt], 0, 1, 2, 3, 4, 5, 6, 7), pf, dv[dt]);
        dk[dt] = P::mfma(__builtin_shufflevector(qT0[dt], qT1[dt], 0, 1, 2, 3, 4, 5, 6, 7), df, dk[dt]);
      }
    }
  }
  if (active && key_ok) dkv_store<P>(p, n, h, key, fg, is_main, dk, dv);
}

template <class P, class PA, bool CAUSAL>
int launch(const gava::AttnBwdMfmaParams& p, hipStream_t s) {
  dim3 grid(p.batch * p.heads), block(256);
  const int kt = (p.n_keys + 15) / 16, qt2 = ((p.n_q + 15) / 16 + 1) / 2 * 2;
  // the dQ kernel writes the row statistics the dK/dV kernel reads: both stream forms take the same statistics layout
  const bool stream_q = !CAUSAL && (kt > 20 || gava::stream_forced());
  const bool stream_kv = !CAUSAL && (qt2 > 18 || gava::stream_forced());
  if (stream_q) hipLaunchKernelGGL((attn_bwd_dq_stream_kernel<P, PA>), dim3(p.batch * p.heads, ((p.n_q + 15) / 16 + 3) / 4), block, 0, s, p);
  else if (kt <= 2) hipLaunchKernelGGL((attn_bwd_dq_kernel<P, PA, 2, CAUSAL>), grid, block, 0, s, p);
  else if (kt <= 6) hipLaunchKernelGGL((attn_bwd_dq_kernel<P, PA, 6, CAUSAL>), grid, block, 0, s, p);
  else if (kt <= 14) hipLaunchKernelGGL((attn_bwd_dq_kernel<P, PA, 14, CAUSAL>), grid, block, 0, s, p);
  else if (kt <= 20) hipLaunchKernelGGL((attn_bwd_dq_kernel<P, PA, 20, CAUSAL>), grid, block, 0, s, p);
  else return GAVA_EINVAL;
  if (stream_kv) hipLaunchKernelGGL((attn_bwd_dkv_stream_kernel<P, PA>), dim3(p.batch * p.heads, (kt + 3) / 4), block, 0, s, p);
  else if (qt2 <= 2) hipLaunchKernelGGL((attn_bwd_dkv_kernel<P, PA, 2, CAUSAL>), grid, block, 0, s, p);
  else if (qt2 <= 6) hipLaunchKernelGGL((attn_bwd_dkv_kernel<P, PA, 6, CAUSAL>), grid, block, 0, s, p);
  else if (qt2 <= 14) hipLaunchKernelGGL((attn_bwd_dkv_kernel<P, PA, 14, CAUSAL>), grid, block, 0, s, p);
  else if (qt2 <= 18) hipLaunchKernelGGL((attn_bwd_dkv_kernel<P, PA, 18, CAUSAL>), grid, block, 0, s, p);
  else return GAVA_EINVAL;
  GAVA_CHECK_LAUNCH();
  return GAVA_OK;
}

}  // namespace

namespace gava {
int attention_bwd_mfma(const AttnBwdMfmaParams& p, int prec, int act_prec, int causal, hipStream_t s) {
  if (causal) {   // the text tower (77 tokens, no prompt rows): same-precision only
    if (p.n_keys != p.n_kmain || prec != act_prec) return GAVA_EINVAL;
    if (prec == GAVA_PREC_F16) return launch<PrecF16, PrecF16, true>(p, s);
    if (prec == GAVA_PREC_BF16) return launch<PrecBF16, PrecBF16, true>(p, s);
    return GAVA_EINVAL;
  }
  if (prec == GAVA_PREC_F16 && act_prec == GAVA_PREC_F16) return launch<PrecF16, PrecF16, false>(p, s);
  if (prec == GAVA_PREC_BF16 && act_prec == GAVA_PREC_BF16) return launch<PrecBF16, PrecBF16, false>(p, s);
  if (prec == GAVA_PREC_BF16 && act_prec == GAVA_PREC_F16) return launch<PrecBF16, PrecF16, false>(p, s);   // fp16 forward, bf16 gradients
  return GAVA_EINVAL;
}
}  // namespace gava
