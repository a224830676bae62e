// Cached prefill: attention of ANY number of new queries to the int8 KV cache (kvcache.hip), contiguous or paged, gfx950.
//
// One workgroup = FOUR waves = one (batch, query head, 128-row Q block, key slice); each wave owns 32 query rows as two 16-row
// blocks (the MB = 2 shape of attn_decode.hip), with that kernel's lane roles, MFMA shapes and tile arithmetic:
//   S^T = K Q^T  (v_mfma_i32_16x16x64_i8), s = fp32(int32(q . k)) * q_scale * k_scale, keys >= the row's limit -> -inf,
//   online softmax in base 2 on the exact argument s - m, P rounded to fp16, O^T += V^T P^T (v_mfma_f32_16x16x32_f16, fp32
//   accumulation), V read back transposed with ds_read_b64_tr_b16 from the [64][2 D + 32] image.
// What differs from decode:
//   * Q is quantised in blocks of 128 rows counted from row 0 of each (batch, query head), the last block cut at q_lens[b]: the
//     block amax crosses the four waves through LDS.  Codes and scales are those of quant_per_block_kernel (blk = 128) on the valid
//     rows, bit for bit.
//   * ragged queries: sequence b owns the first q_lens[b] rows (clamped to [0, Sq]); rows at or past it load as zeros, see no key
//     and are written as zeros with LSE -inf.
//   * causal, bottom-right aligned: query i sees keys < n - q_lens[b] + 1 + i.  A Q block walks only the tiles below its last
//     row's limit; the key-limit compare is applied only to the tiles a limit of the wave's rows cuts.
//   * a 64-key V tile is fetched once per workgroup (register staging, one tile ahead) and shared by the four waves through LDS.
//     K fragments go from global memory straight to the registers of each wave, one tile ahead, as in decode: the simplest
//     correct form.  Sharing K through a double-buffered LDS image as well was measured within 5 % of this: not kept.
// Slices: tile range [split * tps, (split + 1) * tps) of the tiles the Q BLOCK can see, tps = ceil(tiles / splits).  With more
// than one slice each writes the decode kernel's partials - [B, Hkv, splits, M, D] and [.., M, 4], row hl * Sq + sq, M = Sq * group
// - and the unchanged attn_decode_combine_kernel adds them: every (row, slice) entry of ws_ml is written here, m = -inf, l = 0 where
// a slice or a Q block had nothing to do.  No atomics: bitwise reproducible for a given number of slices.
// The body is written once over the KV policies of kv_policy.h: the same products in the same order per slice, so the two layouts
// give bit-identical results.
#include "attn_common.h"
#include "kv_policy.h"

namespace lbfa {

hipError_t launch_attn_decode_combine(const DecodeParams& p, int dtype, int D, hipStream_t stream);  // attn_decode.hip

template <class KV>
struct PrefillOf;
template <>
struct PrefillOf<ContiguousKV> { typedef PrefillParams type; };
template <>
struct PrefillOf<PagedKV> { typedef PagedPrefillParams type; };

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return __builtin_amdgcn_readfirstlane(v);
}

template <class KV, int DT, int D>
__global__ __launch_bounds__(256) void attn_prefill_kernel(typename PrefillOf<KV>::type p) {
  constexpr int MB = 2;             // 16-row blocks per wave
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D / 32;       // 16-byte chunks of a V tile per thread
  typedef typename KV::tile_t tile_t;
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * VROW];
  __shared__ float wamax[4];
  const int qblk = blockIdx.x / p.splits, split = blockIdx.x - qblk * p.splits;
  const int h = blockIdx.y, b = blockIdx.z, hk = h / p.group;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, g = lane >> 4;
  const KV kv(p, b, hk, D);
  const int n = min(max(p.seqlens[kv.slot], 0), p.max_k);
  const int ql = p.q_lens != nullptr ? min(max(p.q_lens[b], 0), p.Sq) : p.Sq;
  // tiles this Q block can see: below the limit of its last valid row (none: the block lies past the sequence's queries)
  const int last = min(qblk * 128 + 127, ql - 1);
  const int see = last < qblk * 128 ? 0 : (p.causal ? max(n - ql + 1 + last, 0) : n);
  const int ntiles = (see + 63) >> 6;
  const int tps = (ntiles + p.splits - 1) / p.splits;
  const int t0 = split * tps, t1 = min(t0 + tps, ntiles);
  const int64_t sh = (int64_t)kv.slot * p.Hkv + hk;  // (slot, kv head): km

  // ---- query rows of this lane: load, quantise with the block's scale, q . km ------------------------------------------
  int row[MB], lim[MB];
  i32x4 qf[MB][KS];
  float corr[MB];
  float qsc;
  {
    float xq[MB][KS][16];
    float amax = 0.f;
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      row[rb] = qblk * 128 + wave * 32 + 16 * rb + i16;
      const bool valid = row[rb] < ql;
      lim[rb] = valid ? (p.causal ? n - ql + 1 + row[rb] : n) : 0;
      float dot = 0.f;
      const unsigned short* qp = p.q + (int64_t)b * p.qb + (int64_t)h * p.qh + (int64_t)(valid ? row[rb] : 0) * p.qs + 16 * g;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        uint4 raw[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (valid) {
          raw[0] = *reinterpret_cast<const uint4*>(qp + 64 * s);
          raw[1] = *reinterpret_cast<const uint4*>(qp + 64 * s + 8);
        }
        uint4 kmr[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (p.km != nullptr) {
          kmr[0] = *reinterpret_cast<const uint4*>(p.km + sh * D + 64 * s + 16 * g);
          kmr[1] = *reinterpret_cast<const uint4*>(p.km + sh * D + 64 * s + 16 * g + 8);
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = elem16<DT>(raw[hf], e);
            dot += v * elem16<DT>(kmr[hf], e);
            const float x = v * p.q_sm_scale;
            xq[rb][s][hf * 8 + e] = x;
            amax = fmaxf(amax, fabsf(x));
          }
      }
      dot += __shfl_xor(dot, 16, 64);
      dot += __shfl_xor(dot, 32, 64);
      corr[rb] = load_cvt<DT>(store_cvt<DT>(dot));  // the correction is a storage-dtype matmul (src/core.py:294-304)
    }
    amax = wave_max(amax);
    if (lane == 0) wamax[wave] = amax;
    __syncthreads();
    qsc = block_scale(amax_collect(wamax), p.q_qmax);
#pragma unroll
    for (int rb = 0; rb < MB; ++rb)
#pragma unroll
      for (int s = 0; s < KS; ++s) qf[rb][s] = quant_codes16<false>(xq[rb][s], qsc, 0.f);  // the plain division
  }
  // the compare against the row limits is needed only in tiles that reach past the smallest limit of this wave's rows
  const int lim_min = wave_min_i32(min(lim[0], lim[1]));

  // ---- running state ---------------------------------------------------------------------------------------------------
  f32x4 acc[MB][CB];
  float m_run[MB], l_run[MB];
#pragma unroll
  for (int rb = 0; rb < MB; ++rb) {
    m_run[rb] = -__builtin_inff();
    l_run[rb] = 0.f;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int8_t* kbase = kv.codes + (int64_t)i16 * D + 16 * g;
  const unsigned short* vbase = kv.v;
  const float* ksc = kv.scale;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  typedef __attribute__((address_space(3))) s16x4v lds_s16x4;
  lds_byte* const vt_lane = (lds_byte*)smem + (4 * g + (i16 >> 2)) * VROW + (i16 & 3) * 8;

  auto load_k = [&](tile_t t, i32x4 (&kf)[4][KS]) __attribute__((always_inline)) {
    const int8_t* kt = kbase + (int64_t)t * 64 * D;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const i32x4*>(kt + kb * 16 * D + 64 * s);
  };
  auto load_v = [&](tile_t t, uint4 (&vr)[VCH]) __attribute__((always_inline)) {
    const unsigned short* vt = vbase + (int64_t)t * 64 * D;
#pragma unroll
    for (int u = 0; u < VCH; ++u) vr[u] = *reinterpret_cast<const uint4*>(vt + (u * 256 + tid) * 8);  // the tile is contiguous
  };
  auto store_v = [&](int t, const uint4 (&vr)[VCH]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < VCH; ++u) {
      const int cidx = u * 256 + tid, r = cidx / (D / 8), ch = cidx % (D / 8);
      // rows past the end may hold anything (0 * NaN): they enter the product as zeros
      const uint4 val = (t * 64 + r < n) ? vr[u] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(smem + r * VROW + ch * 16) = val;
    }
  };
  auto compute = [&](int t, tile_t gt, const i32x4 (&kf)[4][KS], auto masked) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(masked)::value;
    const float kscale = ksc[gt];
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      float sc[4][4];
      float tmax = -__builtin_inff();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        i32x4 sacc = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KS; ++s) sacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf[kb][s], qf[rb][s], sacc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s2 = (float)sacc[r] * qsc * kscale;
          if constexpr (MASK) s2 = t * 64 + kb * 16 + 4 * g + r < lim[rb] ? s2 : -__builtin_inff();
          sc[kb][r] = s2;
          tmax = fmaxf(tmax, s2);
        }
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m_run[rb], tmax);
      const float m_use = m_new == -__builtin_inff() ? 0.f : m_new;  // a row with no visible key yet: p = 0, no NaN
      const float alpha = __builtin_amdgcn_exp2f(m_run[rb] - m_use);
      float lsum = 0.f;
      f16x8 pf[2];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pe = __builtin_amdgcn_exp2f(sc[kb][r] - m_use);
          lsum += pe;
          pf[kb >> 1][(kb & 1) * 4 + r] = (_Float16)pe;
        }
      lsum += __shfl_xor(lsum, 16, 64);
      lsum += __shfl_xor(lsum, 32, 64);
      l_run[rb] = l_run[rb] * alpha + lsum;
      m_run[rb] = m_new;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        acc[rb][cb] *= alpha;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const s16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt_lane + (32 * s) * VROW + cb * 32));
          const s16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt_lane + (32 * s + 16) * VROW + cb * 32));
          const f16x4 lo16 = __builtin_bit_cast(f16x4, lo), hi16 = __builtin_bit_cast(f16x4, hi);
          const f16x8 vf = f16x8{lo16[0], lo16[1], lo16[2], lo16[3], hi16[0], hi16[1], hi16[2], hi16[3]};
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[s], acc[rb][cb], 0, 0, 0);
        }
      }
    }
  };
  // wave-uniform: a tile wholly below every limit of the wave's rows takes the form without the compare (same bits)
  auto tile = [&](int t, tile_t gt, const i32x4 (&kf)[4][KS]) __attribute__((always_inline)) {
    if (t * 64 + 64 <= lim_min) compute(t, gt, kf, std::false_type{});
    else compute(t, gt, kf, std::true_type{});
  };

  // ---- tile loop: K of tile t + 1 lands in the other register set, V of tile t + 1 in registers, while tile t is computed.
  // The look-ahead index is clamped to the slice (the last tile is requested twice, from cache) so no load sits in a branch; the
  // page id of the tile after the look-ahead tile is fetched one step early (ContiguousKV: fetch() is nothing, locate(t) = t).
  // All four waves take every barrier: t0, t1 depend on the workgroup only.
  if (t0 < t1) {
    i32x4 ka[4][KS], kb_[4][KS];
    uint4 vr[VCH];
    tile_t ga = kv.locate(t0, kv.fetch(t0)), gb;
    int pn = kv.fetch(min(t0 + 1, t1 - 1));
    load_k(ga, ka);
    load_v(ga, vr);
    store_v(t0, vr);
    __syncthreads();
    for (int t = t0; t < t1; t += 2) {
      const int ta = min(t + 1, t1 - 1);
      gb = kv.locate(ta, pn);
      pn = kv.fetch(min(t + 2, t1 - 1));
      load_k(gb, kb_);
      load_v(gb, vr);
      tile(t, ga, ka);
      __syncthreads();
      if (t + 1 >= t1) break;
      store_v(ta, vr);
      __syncthreads();
      const int tb = min(t + 2, t1 - 1);
      ga = kv.locate(tb, pn);
      pn = kv.fetch(min(t + 3, t1 - 1));
      load_k(ga, ka);
      load_v(ga, vr);
      tile(t + 1, gb, kb_);
      __syncthreads();
      store_v(tb, vr);
      __syncthreads();
    }
  }

  // ---- epilogue: rows past Sq do not exist; rows in [q_lens[b], Sq) saw no key: zeros, -inf ----------------------------------
  if (p.splits == 1) {
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (row[rb] >= p.Sq) continue;
      const float l = l_run[rb];
      const float inv = l > 0.f ? 1.0f / l : 0.f;  // no visible key: zeros, LSE -inf (as the varlen operator)
      unsigned short* op = reinterpret_cast<unsigned short*>(p.o) + (int64_t)b * p.ob + (int64_t)h * p.oh + (int64_t)row[rb] * p.os + 4 * g;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const f32x4 a = acc[rb][cb];
        const unsigned w0 = (unsigned)store_cvt<DT>(a[0] * inv) | ((unsigned)store_cvt<DT>(a[1] * inv) << 16);
        const unsigned w1 = (unsigned)store_cvt<DT>(a[2] * inv) | ((unsigned)store_cvt<DT>(a[3] * inv) << 16);
        *reinterpret_cast<uint2*>(op + 16 * cb) = make_uint2(w0, w1);
      }
      if (p.lse != nullptr && g == 0) {
        const float lse2 = l > 0.f ? __builtin_amdgcn_logf(l) + m_run[rb] : -__builtin_inff();
        p.lse[((int64_t)b * p.Hq + h) * p.Sq + row[rb]] = lse2 / kLog2e + corr[rb] * p.corr_scale;
      }
    }
  } else {
    const int64_t bh = (int64_t)b * p.Hkv + hk;  // (row of the call, kv head): the partials
    const int64_t slot = (bh * p.splits + split) * p.M + (int64_t)(h - hk * p.group) * p.Sq;
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (row[rb] >= p.Sq) continue;
      if (t0 < t1) {  // the combine never reads the acc of a slice whose m is -inf
        float* ap = p.ws_acc + (slot + row[rb]) * D + 4 * g;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) *reinterpret_cast<f32x4*>(ap + 16 * cb) = acc[rb][cb];
      }
      if (g == 0) *reinterpret_cast<f32x4*>(p.ws_ml + (slot + row[rb]) * 4) = f32x4{m_run[rb], l_run[rb], corr[rb], 0.f};
    }
  }
}

// ---- host-side launchers (called from lbfa_api.hip) ----------------------------------------------------------------------
template <class KV>
static hipError_t launch_prefill(const typename PrefillOf<KV>::type& p, int dtype, int D, hipStream_t stream) {
  dim3 grid((unsigned)p.nQ * (unsigned)p.splits, p.Hq, p.B);
#define LBFA_PRE(DT, DD) hipLaunchKernelGGL((attn_prefill_kernel<KV, DT, DD>), grid, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_PRE(LBFA_F16, 64); else LBFA_PRE(LBFA_F16, 128); }
  else { if (D == 64) LBFA_PRE(LBFA_BF16, 64); else LBFA_PRE(LBFA_BF16, 128); }
#undef LBFA_PRE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.splits == 1) return e;
  return launch_attn_decode_combine(p, dtype, D, stream);  // the partials are the decode kernel's: its second launch, unchanged
}
hipError_t launch_attn_prefill(const PrefillParams& p, int dtype, int D, hipStream_t stream) {
  return launch_prefill<ContiguousKV>(p, dtype, D, stream);
}
hipError_t launch_attn_paged_prefill(const PagedPrefillParams& p, int dtype, int D, hipStream_t stream) {
  return launch_prefill<PagedKV>(p, dtype, D, stream);
}

}  // namespace lbfa
