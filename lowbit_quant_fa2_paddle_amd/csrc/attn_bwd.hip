// Attention backward (dQ, dK, dV) for gfx950: the FlashAttention-2 two-kernel form, deterministic (no float atomics).
//
// Contract (DESIGN.md "Backward"): straight-through on the quantiser.  P is the forward's own P, recomputed from the scores
// the forward used and the LSE it returned - P = exp2(s2 - lse2) with s2 = (q codes . k codes) * q_scale * k_scale (int8 /
// int4-range operators; sm_scale * log2(e) is folded into q_scale) or s2 = (q . k) * sm_scale * log2(e) (lbfa_sdpa_fwd), and
// lse2 the base-2 LSE without the smooth-K correction (bwd_prep_kernel).  The products that carry the gradient run on the
// un-quantised 16-bit tensors in the input dtype (fp16 / bf16 MFMA, fp32 accumulation):
//     dV = P^T dO,  dP = dO V^T,  delta_i = sum_d dO_id O_id - dLSE_i,  dS = P o (dP - delta),
//     dQ = sm_scale dS K,  dK = sm_scale dS^T Q.
//
// Kernels (one launch each, in this order on one stream):
//   bwd_prep_kernel  one thread per query row: delta and lse2.
//   bwd_dkdv_kernel  one workgroup per (b, kv head, 64-key block), 4 waves x 16 keys; loops over the group's query heads and
//                    64-row query tiles (Q / dO tiles and their transposes through LDS); K and V fragments stay in registers.
//   bwd_dq_kernel    one workgroup per (b, q head, 64-row query block), 4 waves x 16 queries; loops over 64-key tiles (K, K^T
//                    and V through LDS); the wave's Q and dO fragments stay in registers.
// Every sum is formed in one fixed order by one workgroup: results are bitwise reproducible run to run.
//
// Packed batches (VARLEN, lbfa_backward_varlen): sequence b owns query tokens [cu_q[b], cu_q[b+1]) and key tokens
// [cu_k[b], cu_k[b+1]), lengths cut at the maxima Sq / Sk as in the forward; batch strides are 0, rows of lse / dlse / corr
// / lse2 / delta are [Hq, total_q].  The grids are sized by the maxima and workgroups past a sequence's end exit at once; the
// same three kernels then run on per-sequence bases and lengths, so one packed sequence forms the dense sums in the dense
// order.  The pre-pass also zeroes the dq / dk / dv rows of tokens that lie in no sequence or past the cut.
//
// MFMA: v_mfma_f32_16x16x32_{f16,bf16}.  Lane l holds A[row l&15][k = 8(l>>4) + j] and B[k = 8(l>>4) + j][col l&15], j = 0..7,
// and receives C[row 4(l>>4) + i][col l&15], i = 0..3.  An accumulator tile pair (rows 0..15 and 16..31) is used directly as
// the A operand of a product that sums over those rows by taking the k order j < 4 -> row 4(l>>4) + j, j >= 4 -> row
// 16 + 4(l>>4) + j - 4; the B operand of that product is read from a transposed LDS tile in the same k order (pair_b).
//
// Integer scores: q / k codes (|code| <= 127) are exact in fp16 and their products (< 2^14) and sums over D <= 128 channels
// (< 2^21) are exact in fp32, so an fp16 MFMA on the codes gives the forward's integer dot product bit for bit.
#include "lbfa_common.h"
#include "attn_common.h"

namespace lbfa {
namespace {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBlk = 64;       // keys per dK/dV workgroup, queries per dQ workgroup, rows per LDS tile
constexpr int kThreads = 256;  // 4 waves x 16 rows
constexpr int kPad = 8;        // LDS row padding (elements): 16-byte aligned rows, rows spread over the banks
constexpr float kLog2e = 1.44269504f;

template <int T>
__device__ __forceinline__ f32x4 mma(u16x8 a, u16x8 b, f32x4 c) {
  if constexpr (T == LBFA_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// 8 elements of row `row` (< S, else zeros), columns c..c+7, as 16-bit patterns of the MFMA type: int8 codes -> fp16 (QUANT)
// or the raw 16-bit values
template <bool CODES>
__device__ __forceinline__ u16x8 load8(const void* base, int64_t off, bool ok) {
  u16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!ok) return r;
  if constexpr (CODES) {
    const u32x2 raw = *reinterpret_cast<const u32x2*>(reinterpret_cast<const int8_t*>(base) + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = (int)(int8_t)((raw[e >> 2] >> (8 * (e & 3))) & 0xffu);
      r[e] = f32_to_f16_bits((float)c);
    }
  } else {
    r = *reinterpret_cast<const u16x8*>(reinterpret_cast<const unsigned short*>(base) + off);
  }
  return r;
}

__device__ __forceinline__ u16x8 cat4(u16x4 a, u16x4 b) { return u16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

// two accumulator tiles (rows 0..15, 16..31) as one A operand in the pair k order
template <int DT>
__device__ __forceinline__ u16x8 pack_pair(const f32x4& t0, const f32x4& t1) {
  u16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = store_cvt<DT>(t0[i]);
    r[4 + i] = store_cvt<DT>(t1[i]);
  }
  return r;
}

// B operand in the pair k order from a transposed LDS tile T[col][row]: rows r0 + 4g + 0..3 and r0 + 16 + 4g + 0..3
__device__ __forceinline__ u16x8 pair_b(const unsigned short* T, int ld, int col, int r0, int g) {
  const unsigned short* p = T + col * ld + r0 + 4 * g;
  return cat4(*reinterpret_cast<const u16x4*>(p), *reinterpret_cast<const u16x4*>(p + 16));
}

// cooperative load of a 64 x D tile (rows r0.. of one (b, h) panel) into LDS: row-major R[row][D + kPad] (if R) and / or
// transposed T[d][64 + kPad] (if T).  Rows >= S are zeros.
template <int D, bool CODES>
__device__ __forceinline__ void load_tile(const void* base, int64_t rs, int r0, int S, unsigned short* R, unsigned short* T) {
  constexpr int CH = D / 8;  // 16-byte chunks per row
#pragma unroll
  for (int it = 0; it < kBlk * CH / kThreads; ++it) {
    const int idx = threadIdx.x + it * kThreads;
    const int row = idx / CH, c = (idx % CH) * 8;
    const u16x8 v = load8<CODES>(base, (int64_t)(r0 + row) * rs + c, r0 + row < S);
    if (R) *reinterpret_cast<u16x8*>(R + row * (D + kPad) + c) = v;
    if (T) {
#pragma unroll
      for (int e = 0; e < 8; ++e) T[(c + e) * (kBlk + kPad) + row] = v[e];
    }
  }
}

// packed batch: token t lies in a sequence and within its first `cap` tokens (the last b with cu[b] <= t, by bisection)
__device__ __forceinline__ bool covered(const int* cu, int B, int cap, int t) {
  if (t < cu[0]) return false;
  int lo = 0, hi = B;  // cu[lo] <= t; the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= t) lo = mid;
    else hi = mid;
  }
  return t < cu[lo + 1] && t - cu[lo] < cap;
}

__device__ __forceinline__ void zero_row(unsigned short* r, int D) {
  for (int c = 0; c < D; ++c) r[c] = 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// delta_i = sum_d dO_id O_id - dLSE_i (fp32, d ascending) and lse2_i = (lse_i - corr_i * sm_scale) * log2(e)
// VARLEN: rows [Hq, total_q], then one thread per key row [Hkv, total_k]; rows of no sequence get zero gradients here
// corr_i = dtype(q_i . km) is the value the forward added to the LSE, formed in the forward kernels' order (the in-kernel Q
// quantiser of attn_fwd16.hip / attn_fwd.hip): lane group g = 0..3 of a row sums the exact products of columns
// 64 s + 16 g + 0..15, s ascending, in sequence; then (S0 + S1) + (S2 + S3), rounded to the dtype.  Any other order can round
// to the neighbouring dtype value, which scales every P of the row by 2^(ulp(corr) * sm_scale * log2(e)).
template <int DT>
__device__ __forceinline__ float fwd_corr(const unsigned short* q, const unsigned short* km, int D) {
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < D; s += 64) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int c = s + 16 * g + 8 * hf;
        const u16x8 qv = *reinterpret_cast<const u16x8*>(q + c), kv = *reinterpret_cast<const u16x8*>(km + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) part[g] = part[g] + load_cvt<DT>(qv[e]) * load_cvt<DT>(kv[e]);
      }
  }
  return load_cvt<DT>(store_cvt<DT>((part[0] + part[1]) + (part[2] + part[3])));
}

// ------------------------------------------------------------------------------------------------------------------------
template <int DT, bool VARLEN>
__global__ void __launch_bounds__(256) bwd_prep_kernel(BwdParams p) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = VARLEN ? p.total_q : p.Sq;
  const int64_t rows = (int64_t)(VARLEN ? 1 : p.B) * p.Hq * S;
  if constexpr (VARLEN) {
    if (row >= rows) {
      const int64_t kr = row - rows;
      if (kr >= (int64_t)p.Hkv * p.total_k) return;
      const int t = (int)(kr % p.total_k), hk = (int)(kr / p.total_k);
      if (!covered(p.cu_k, p.B, p.Sk, t)) {
        zero_row(p.dk + hk * p.dkh + t * p.dks, p.D);
        zero_row(p.dv + hk * p.dvh + t * p.dvs, p.D);
      }
      return;
    }
  }
  if (row >= rows) return;
  const int s = (int)(row % S);
  const int64_t bh = row / S;
  const int h = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
  if constexpr (VARLEN) {
    if (!covered(p.cu_q, p.B, p.Sq, s)) {
      zero_row(p.dq + h * p.dqh + s * p.dqs, p.D);
      return;
    }
  }
  const unsigned short* o = p.o + b * p.ob + h * p.oh + s * p.os;
  const unsigned short* d = p.dout + b * p.db + h * p.dh + s * p.ds;
  float acc = 0.f;
  for (int c = 0; c < p.D; c += 8) {
    const u16x8 ov = *reinterpret_cast<const u16x8*>(o + c), dv = *reinterpret_cast<const u16x8*>(d + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(load_cvt<DT>(ov[e]), load_cvt<DT>(dv[e]), acc);
  }
  if (p.dlse) acc -= p.dlse[row];
  p.delta[row] = acc;
  float l = p.lse[row];
  if (p.km) l -= fwd_corr<DT>(p.q + b * p.qb + h * p.qh + s * p.qs, p.km + ((int64_t)b * p.Hkv + h / p.group) * p.D, p.D) * p.corr_scale;
  p.lse2[row] = l * kLog2e;
}

// ------------------------------------------------------------------------------------------------------------------------
// dK, dV: one workgroup per (b, kv head, 64-key block)
// ------------------------------------------------------------------------------------------------------------------------
template <int D, int DT, bool QUANT, bool CAUSAL, bool VARLEN>
__global__ void __launch_bounds__(kThreads) bwd_dkdv_kernel(BwdParams p) {
  constexpr int ST = QUANT ? LBFA_F16 : DT;  // MFMA type of the score product
  constexpr int KS = D / 32;                 // k steps over the head dim
  constexpr int NT = D / 16;                 // 16-column output tiles
  constexpr int LR = D + kPad, LT = kBlk + kPad;
  __shared__ __attribute__((aligned(16))) unsigned short sQ[kBlk * LR];   // score operand of Q (codes or raw), row-major
  __shared__ __attribute__((aligned(16))) unsigned short sQT[D * LT];     // Q^T (raw)
  __shared__ __attribute__((aligned(16))) unsigned short sO[kBlk * LR];   // dO row-major
  __shared__ __attribute__((aligned(16))) unsigned short sOT[D * LT];     // dO^T
  __shared__ float sL[kBlk], sDelta[kBlk];

  const int nkb = (p.Sk + kBlk - 1) / kBlk;
  int id = blockIdx.x;
  const int kb = id % nkb; id /= nkb;
  const int hk = id % p.Hkv;
  const int b = id / p.Hkv;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int k0 = kb * kBlk;
  const int key = k0 + 16 * w + c16;  // this lane's key as a score column / operand row
  int Sq = p.Sq, Sk = p.Sk;
  int64_t qt0 = 0, kt0 = 0;  // first query / key token of the sequence (packed batch)
  if constexpr (VARLEN) {
    qt0 = p.cu_q[b]; kt0 = p.cu_k[b];
    Sq = min(p.cu_q[b + 1] - (int)qt0, p.Sq);
    Sk = min(p.cu_k[b + 1] - (int)kt0, p.Sk);
    if (k0 >= Sk) return;  // whole workgroup, before any barrier
  }

  // K (score operand) and V fragments of the wave's 16 keys: lane holds row `key`, k = 8g + j of each 32-wide step
  u16x8 kf[KS], vf[KS];
  {
    const void* kbase = QUANT ? (const void*)(p.k8 + b * p.k8b + hk * p.k8h + kt0 * p.k8s)
                              : (const void*)(p.k + b * p.kb + hk * p.kh + kt0 * p.ks);
    const int64_t krs = QUANT ? p.k8s : p.ks;
    const unsigned short* vbase = p.v + b * p.vb + hk * p.vh + kt0 * p.vs;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kf[s] = load8<QUANT>(kbase, (int64_t)key * krs + 32 * s + 8 * g, key < Sk);
      vf[s] = load8<false>(vbase, (int64_t)key * p.vs + 32 * s + 8 * g, key < Sk);
    }
  }
  const float ksc = QUANT ? p.k_scale[((int64_t)b * p.Hkv + hk) * p.nK + kb] : 1.f;

  f32x4 dk[NT], dv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nqb = (Sq + kBlk - 1) / kBlk;
  const int qb_first = CAUSAL ? kb : 0;  // causal (Sq == Sk): queries below k0 see none of these keys
  for (int hq = hk * p.group; hq < (hk + 1) * p.group; ++hq) {
    const void* qsb = QUANT ? (const void*)(p.q8 + b * p.q8b + hq * p.q8h + qt0 * p.q8s)
                            : (const void*)(p.q + b * p.qb + hq * p.qh + qt0 * p.qs);
    const int64_t qsrs = QUANT ? p.q8s : p.qs;
    const unsigned short* qraw = p.q + b * p.qb + hq * p.qh + qt0 * p.qs;
    const unsigned short* dob = p.dout + b * p.db + hq * p.dh + qt0 * p.ds;
    const int64_t rowbase = VARLEN ? (int64_t)hq * p.total_q + qt0 : ((int64_t)b * p.Hq + hq) * p.Sq;
    for (int qb = qb_first; qb < nqb; ++qb) {
      const int q0 = qb * kBlk;
      __syncthreads();  // the previous tile's readers are done
      if constexpr (QUANT) {
        load_tile<D, true>(qsb, qsrs, q0, Sq, sQ, nullptr);
        load_tile<D, false>(qraw, p.qs, q0, Sq, nullptr, sQT);
      } else {
        load_tile<D, false>(qraw, p.qs, q0, Sq, sQ, sQT);
      }
      load_tile<D, false>(dob, p.ds, q0, Sq, sO, sOT);
      if (threadIdx.x < kBlk) {
        const int q = q0 + threadIdx.x;
        sL[threadIdx.x] = q < Sq ? p.lse2[rowbase + q] : 0.f;
        sDelta[threadIdx.x] = q < Sq ? p.delta[rowbase + q] : 0.f;
      }
      __syncthreads();
      const float sc = QUANT ? p.q_scale[((int64_t)b * p.Hq + hq) * p.nQ + (q0 / LBFA_BLKQ)] * ksc : p.qk_scale;

      // S = Q K^T and dP = dO V^T for 4 tiles of 16 queries x this wave's 16 keys
      f32x4 sP[4], sD[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
        const int r = 16 * t + c16;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const u16x8 qa = *reinterpret_cast<const u16x8*>(sQ + r * LR + 32 * s + 8 * g);
          const u16x8 oa = *reinterpret_cast<const u16x8*>(sO + r * LR + 32 * s + 8 * g);
          a = mma<ST>(qa, kf[s], a);
          d = mma<DT>(oa, vf[s], d);
        }
        // P = exp2(s2 - lse2), masked; dS = P (dP - delta)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ql = 16 * t + 4 * g + i, q = q0 + ql;
          bool ok = q < Sq && key < Sk;
          if (CAUSAL) ok = ok && key <= q;
          const float pv = ok ? __builtin_amdgcn_exp2f(a[i] * sc - sL[ql]) : 0.f;
          a[i] = pv;
          d[i] = pv * (d[i] - sDelta[ql]);
        }
        sP[t] = a;
        sD[t] = d;
      }
      // dV += P^T dO, dK += dS^T Q over the tile's 64 queries (two pairs of 16-row tiles)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const u16x8 pa = pack_pair<DT>(sP[2 * pr], sP[2 * pr + 1]);
        const u16x8 da = pack_pair<DT>(sD[2 * pr], sD[2 * pr + 1]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          dv[t] = mma<DT>(pa, pair_b(sOT, LT, 16 * t + c16, 32 * pr, g), dv[t]);
          dk[t] = mma<DT>(da, pair_b(sQT, LT, 16 * t + c16, 32 * pr, g), dk[t]);
        }
      }
    }
  }
  // store: lane holds rows (keys) 16w + 4g + i, column 16t + c16
  unsigned short* dkb = p.dk + b * p.dkb + hk * p.dkh + kt0 * p.dks;
  unsigned short* dvb = p.dv + b * p.dvb + hk * p.dvh + kt0 * p.dvs;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = k0 + 16 * w + 4 * g + i;
    if (kr >= Sk) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      dkb[(int64_t)kr * p.dks + 16 * t + c16] = store_cvt<DT>(dk[t][i] * p.sm_scale);
      dvb[(int64_t)kr * p.dvs + 16 * t + c16] = store_cvt<DT>(dv[t][i]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// dQ: one workgroup per (b, q head, 64-row query block).  Scores are formed transposed (S^T = K Q^T: keys on the rows), so
// dS^T's accumulator tiles are the A operand of dQ = dS K directly.
// ------------------------------------------------------------------------------------------------------------------------
template <int D, int DT, bool QUANT, bool CAUSAL, bool VARLEN>
__global__ void __launch_bounds__(kThreads) bwd_dq_kernel(BwdParams p) {
  constexpr int ST = QUANT ? LBFA_F16 : DT;
  constexpr int KS = D / 32;
  constexpr int NT = D / 16;
  constexpr int LR = D + kPad, LT = kBlk + kPad;
  __shared__ __attribute__((aligned(16))) unsigned short sK[kBlk * LR];   // score operand of K, row-major
  __shared__ __attribute__((aligned(16))) unsigned short sKT[D * LT];     // K^T (raw)
  __shared__ __attribute__((aligned(16))) unsigned short sV[kBlk * LR];   // V row-major

  const int nqb = (p.Sq + kBlk - 1) / kBlk;
  int id = blockIdx.x;
  const int qb = id % nqb; id /= nqb;
  const int hq = id % p.Hq;
  const int b = id / p.Hq;
  const int hk = hq / p.group;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
  const int q0 = qb * kBlk;
  const int q = q0 + 16 * w + c16;  // this lane's query (score column / operand row)
  int Sq = p.Sq, Sk = p.Sk;
  int64_t qt0 = 0, kt0 = 0;  // first query / key token of the sequence (packed batch)
  if constexpr (VARLEN) {
    qt0 = p.cu_q[b]; kt0 = p.cu_k[b];
    Sq = min(p.cu_q[b + 1] - (int)qt0, p.Sq);
    Sk = min(p.cu_k[b + 1] - (int)kt0, p.Sk);
    if (q0 >= Sq) return;  // whole workgroup, before any barrier
  }
  const bool qok = q < Sq;

  u16x8 qf[KS], of[KS];
  {
    const void* qsb = QUANT ? (const void*)(p.q8 + b * p.q8b + hq * p.q8h + qt0 * p.q8s)
                            : (const void*)(p.q + b * p.qb + hq * p.qh + qt0 * p.qs);
    const int64_t qsrs = QUANT ? p.q8s : p.qs;
    const unsigned short* dob = p.dout + b * p.db + hq * p.dh + qt0 * p.ds;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = load8<QUANT>(qsb, (int64_t)q * qsrs + 32 * s + 8 * g, qok);
      of[s] = load8<false>(dob, (int64_t)q * p.ds + 32 * s + 8 * g, qok);
    }
  }
  const int64_t row = (VARLEN ? (int64_t)hq * p.total_q + qt0 : ((int64_t)b * p.Hq + hq) * p.Sq) + q;
  const float l2 = qok ? p.lse2[row] : 0.f, dl = qok ? p.delta[row] : 0.f;
  const float qsc = QUANT ? p.q_scale[((int64_t)b * p.Hq + hq) * p.nQ + (q0 / LBFA_BLKQ)] : p.qk_scale;

  f32x4 dq[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const void* ksb = QUANT ? (const void*)(p.k8 + b * p.k8b + hk * p.k8h + kt0 * p.k8s)
                          : (const void*)(p.k + b * p.kb + hk * p.kh + kt0 * p.ks);
  const int64_t ksrs = QUANT ? p.k8s : p.ks;
  const unsigned short* kraw = p.k + b * p.kb + hk * p.kh + kt0 * p.ks;
  const unsigned short* vb = p.v + b * p.vb + hk * p.vh + kt0 * p.vs;
  const int nkb = (Sk + kBlk - 1) / kBlk;
  int kb_end = CAUSAL ? qb + 1 : nkb;  // causal (Sq == Sk): keys beyond q0 + 63 are masked for the whole block
  if constexpr (VARLEN && CAUSAL) kb_end = min(kb_end, nkb);  // len_q == len_k is the caller's promise: stay in the scale rows
  for (int kb = 0; kb < kb_end; ++kb) {
    const int k0 = kb * kBlk;
    __syncthreads();
    if constexpr (QUANT) {
      load_tile<D, true>(ksb, ksrs, k0, Sk, sK, nullptr);
      load_tile<D, false>(kraw, p.ks, k0, Sk, nullptr, sKT);
    } else {
      load_tile<D, false>(kraw, p.ks, k0, Sk, sK, sKT);
    }
    load_tile<D, false>(vb, p.vs, k0, Sk, sV, nullptr);
    __syncthreads();
    const float sc = QUANT ? qsc * p.k_scale[((int64_t)b * p.Hkv + hk) * p.nK + kb] : qsc;

    f32x4 sD[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
      const int r = 16 * t + c16;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const u16x8 ka = *reinterpret_cast<const u16x8*>(sK + r * LR + 32 * s + 8 * g);
        const u16x8 va = *reinterpret_cast<const u16x8*>(sV + r * LR + 32 * s + 8 * g);
        a = mma<ST>(ka, qf[s], a);
        d = mma<DT>(va, of[s], d);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = k0 + 16 * t + 4 * g + i;
        bool ok = qok && kk < Sk;
        if (CAUSAL) ok = ok && kk <= q;
        const float pv = ok ? __builtin_amdgcn_exp2f(a[i] * sc - l2) : 0.f;
        d[i] = pv * (d[i] - dl);
      }
      sD[t] = d;
    }
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const u16x8 da = pack_pair<DT>(sD[2 * pr], sD[2 * pr + 1]);
#pragma unroll
      for (int t = 0; t < NT; ++t) dq[t] = mma<DT>(da, pair_b(sKT, LT, 16 * t + c16, 32 * pr, g), dq[t]);
    }
  }
  // store: lane holds rows (queries) 16w + 4g + i, column 16t + c16
  unsigned short* dqb = p.dq + b * p.dqb + hq * p.dqh + qt0 * p.dqs;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qr = q0 + 16 * w + 4 * g + i;
    if (qr >= Sq) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) dqb[(int64_t)qr * p.dqs + 16 * t + c16] = store_cvt<DT>(dq[t][i] * p.sm_scale);
  }
}

template <int D, int DT, bool QUANT, bool CAUSAL, bool VARLEN>
hipError_t launch_bwd_t(const BwdParams& p, hipStream_t stream) {
  const unsigned rows = VARLEN ? (unsigned)((int64_t)p.Hq * p.total_q + (int64_t)p.Hkv * p.total_k)
                               : (unsigned)((int64_t)p.B * p.Hq * p.Sq);
  hipLaunchKernelGGL((bwd_prep_kernel<DT, VARLEN>), dim3((rows + 255) / 256), dim3(256), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned nkb = (unsigned)((p.Sk + kBlk - 1) / kBlk), nqb = (unsigned)((p.Sq + kBlk - 1) / kBlk);
  hipLaunchKernelGGL((bwd_dkdv_kernel<D, DT, QUANT, CAUSAL, VARLEN>), dim3(nkb * p.Hkv * p.B), dim3(kThreads), 0, stream, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bwd_dq_kernel<D, DT, QUANT, CAUSAL, VARLEN>), dim3(nqb * p.Hq * p.B), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

template <int D, int DT>
hipError_t launch_bwd_d(const BwdParams& p, bool quant, bool causal, hipStream_t stream) {
  if (p.cu_q != nullptr)  // packed batches are always quantised (the varlen forward has no un-quantised mode)
    return causal ? launch_bwd_t<D, DT, true, true, true>(p, stream) : launch_bwd_t<D, DT, true, false, true>(p, stream);
  if (quant) return causal ? launch_bwd_t<D, DT, true, true, false>(p, stream) : launch_bwd_t<D, DT, true, false, false>(p, stream);
  return causal ? launch_bwd_t<D, DT, false, true, false>(p, stream) : launch_bwd_t<D, DT, false, false, false>(p, stream);
}

}  // namespace

hipError_t launch_attn_bwd(const BwdParams& p, int dtype, bool quant, bool causal, hipStream_t stream) {
  if (p.D == 64)
    return dtype == LBFA_F16 ? launch_bwd_d<64, LBFA_F16>(p, quant, causal, stream) : launch_bwd_d<64, LBFA_BF16>(p, quant, causal, stream);
  return dtype == LBFA_F16 ? launch_bwd_d<128, LBFA_F16>(p, quant, causal, stream) : launch_bwd_d<128, LBFA_BF16>(p, quant, causal, stream);
}

}  // namespace lbfa
