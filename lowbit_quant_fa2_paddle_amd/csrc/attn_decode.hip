// Split-KV decode attention over the int8 KV cache (kvcache.hip), contiguous or paged, for short queries, gfx950.
//
// One workgroup = ONE wave = one (batch, kv head, key slice) and all M = Sq * (Hq / Hkv) <= 64 query rows that share the kv head:
// K codes and V are streamed once per GQA group.  The kernel is HBM-bound (3 D bytes per key), so it has none of the prefill
// machinery: K fragments go from global memory straight to the registers the MFMA reads, V goes through a wave-private LDS
// image only because the PV product needs it transposed, both one 64-key tile ahead of the arithmetic; parallelism comes from
// the key slices (lbfa_decode_num_splits), a dozen waves per CU each with a tile in flight.
//
// Arithmetic of a tile (the reference's kernel, attn_qk_int8_per_block.py:51-61, with P V accumulated in fp32):
//   s = fp32(int32(q . k)) * q_scale * k_scale;  keys >= the row's limit -> -inf;  m' = max(m, rowmax);  p = exp2(s - m');
//   l = l * exp2(m - m') + sum(p);  acc = acc * exp2(m - m') + fp16(p) V.
// Q is quantised here, the Sq rows of one (batch, query head) as one block - what quant_per_block_kernel does for Sq <= 128 -
// with the same fp32 operations (codes and scale bit-identical).
//
// Lane roles (i = lane & 15, g = lane >> 4), as in attn_fwd16.hip:
//   S^T = K Q^T  (v_mfma_i32_16x16x64_i8)   A = K: key 16 kb + i, bytes [64 s + 16 g, +16);  B = Q: row 16 rb + i, same bytes;
//                C: the lane holds, for ITS query row 16 rb + i, keys 16 kb + 4 g + {0..3}
//   O^T += V^T P^T (v_mfma_f32_16x16x32_f16) B = P^T of k-step s: element j = key 32 s + 16 (j >> 2) + 4 g + (j & 3), the lane's
//                own scores;  A = V^T in the same key order: two ds_read_b64_tr_b16 of the row-major V tile (rows
//                32 s + 4 g + {0..3} and + 16);  C: for its query row, channels 16 cb + 4 g + {0..3}
// V tile in LDS: [64 keys][2 D + 32 bytes]: the pad puts the 8 rows a 32-lane half reads at once on distinct banks.
// Slices: tile range [split * tps, (split + 1) * tps) of the sequence's ceil(n / 64) tiles, tps = ceil(tiles / splits).  With
// more than one slice each writes un-normalised fp32 acc and (m, l); attn_decode_combine_kernel adds them in one fixed order (no
// atomics: bitwise reproducible for a given number of slices).
//
// ONE kernel body serves the contiguous cache and the paged one.  What differs - where a tile lives - is the KV policy:
// ContiguousKV (cache [B, Hkv, cap, D], row b of the call is sequence b) or PagedKV (pool of pages behind a block table, row b
// addresses slot slots[b]).  A policy owns the slot of the row with its clamp, the bases of codes, V and scales, fetch(t) (the
// table load for tile t) and locate(t, pg) (the number that names the tile to the loads).  Everything else - Q prologue, masks,
// online softmax, V staging, epilogue, partials - is written once and does not know where a tile lives (the schedule of the
// tile loop has a form with and one without table look-ups, see there): same products in the same order per slice, so the two layouts give bit-identical results for the same number of slices.
// What happens to a tile - load_k / load_v / store_v / compute with the running state of the online softmax - is written once for
// this kernel and for cached prefill (attn_prefill.hip), in attn_cache_tile.inc; the Q prologue, the tile loop and the epilogue are
// this kernel's own (attn_decode_body.inc).
#include "attn_common.h"
#include "kv_policy.h"

namespace lbfa {

// The body is written once, in attn_decode_body.inc, and included as text into both kernels: VB = bits of a cached V element, 16 (fp16) or 8
// (e4m3 codes with a scale per key, kv_policy.h).  Text, not a function the two kernels call: routed through an inlined function
// the fp16 instances compile to other code than they had (same instructions, another schedule), and they are the yardstick the fp8
// family is measured against.  Included, they are the code they were, byte for byte.  The body includes attn_cache_tile.inc, the
// text it shares with the prefill body, for the same reason.
// The V format is known to load_v and store_v only; KB = bits of a cached K code, known to load_k and the score product only.
template <class KV, int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_decode_kernel(typename KV::Params p) {
  constexpr int VB = 16, KB = 8;
#include "attn_decode_body.inc"
}
// the same kernel over the fp8 V cache; the name keeps its family apart from the fp16 one in the code object
template <class KV, int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_decode_v8_kernel(V8Params<typename KV::Params, const float*> p) {
  constexpr int VB = 8, KB = 8;
#include "attn_decode_body.inc"
}
// the same two kernels over the nibble-packed K cache (K4Params, lbfa_common.h): half the K bytes per key, widened in registers
template <class KV, int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_decode_k4_kernel(K4Params<typename KV::Params> p) {
  constexpr int VB = 16, KB = 4;
#include "attn_decode_body.inc"
}
template <class KV, int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_decode_k4_v8_kernel(K4Params<V8Params<typename KV::Params, const float*>> p) {
  constexpr int VB = 8, KB = 4;
#include "attn_decode_body.inc"
}

#ifndef LBFA_K4_UNIT  // the combine kernel lives in the unit of the byte-per-code instances

// Adds the slices of one query row: m = max m_s, l = sum l_s 2^(m_s - m), O = sum acc_s 2^(m_s - m) / l, in ONE fixed order - the
// 256 threads are 256 / D groups of one thread per channel, group g adds its contiguous run of ceil(splits / groups) slices in
// slice order (eight independent loads in flight: a dependent chain over 128 slices cost three times the decode kernel itself),
// then the groups are added in group order.  A slice that saw no key (m_s = -inf) is skipped - its acc may never have been
// written.
template <int DT, int D>
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(DecodeParams p) {
  constexpr int NG = 256 / D, NB = 8;
  __shared__ float red[256];
  __shared__ float part_a[NG][D];
  __shared__ float part_l[NG];
  const int r = blockIdx.x, hk = blockIdx.y, b = blockIdx.z, t = threadIdx.x, d = t % D, grp = t / D;
  const int64_t bh = (int64_t)b * p.Hkv + hk;
  const float* ml = p.ws_ml + (bh * p.splits * p.M + r) * 4;
  const float* ap = p.ws_acc + (bh * p.splits * p.M + r) * D + d;
  const int64_t sstep = (int64_t)p.M;
  const float ninf = -__builtin_inff();
  float m = ninf;
  for (int s = t; s < p.splits; s += 256) m = fmaxf(m, ml[s * sstep * 4]);
  red[t] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // a maximum: any order gives the same bits
    if (t < o) red[t] = fmaxf(red[t], red[t + o]);
    __syncthreads();
  }
  m = red[0];
  const int chunk = (p.splits + NG - 1) / NG, s_lo = grp * chunk, s_hi = min(s_lo + chunk, p.splits);
  float l = 0.f, a = 0.f;
  if (m != ninf)
    for (int s0 = s_lo; s0 < s_hi; s0 += NB) {
      float ms[NB], ls[NB], as[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {  // the index is clamped, not the load skipped: all NB loads go out together
        const int64_t sj = min(s0 + j, s_hi - 1) * sstep;
        ms[j] = ml[sj * 4];
        ls[j] = ml[sj * 4 + 1];
        as[j] = ap[sj * D];
      }
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (s0 + j < s_hi && ms[j] != ninf) {
          const float w = __builtin_amdgcn_exp2f(ms[j] - m);
          l = l + ls[j] * w;
          a = a + as[j] * w;
        }
    }
  part_a[grp][d] = a;
  if (d == 0) part_l[grp] = l;
  __syncthreads();
  if (grp != 0) return;
  l = part_l[0];
  a = part_a[0][d];
#pragma unroll
  for (int g2 = 1; g2 < NG; ++g2) {
    l = l + part_l[g2];
    a = a + part_a[g2][d];
  }
  const int hl = r / p.Sq, sq = r - hl * p.Sq, hq = hk * p.group + hl;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  reinterpret_cast<unsigned short*>(p.o)[(int64_t)b * p.ob + (int64_t)hq * p.oh + (int64_t)sq * p.os + d] = store_cvt<DT>(a * inv);
  if (p.lse != nullptr && d == 0) {
    const float lse2 = l > 0.f ? __builtin_amdgcn_logf(l) + m : ninf;
    p.lse[((int64_t)b * p.Hq + hq) * p.Sq + sq] = lse2 / kLog2e + ml[2] * p.corr_scale;
  }
}

// the second launch of a call with more than one slice, whichever the layout of the cache
hipError_t launch_attn_decode_combine(const DecodeParams& p, int dtype, int D, hipStream_t stream) {
  dim3 g2(p.M, p.Hkv, p.B);
#define LBFA_CMB(DT, DD) hipLaunchKernelGGL((attn_decode_combine_kernel<DT, DD>), g2, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_CMB(LBFA_F16, 64); else LBFA_CMB(LBFA_F16, 128); }
  else { if (D == 64) LBFA_CMB(LBFA_BF16, 64); else LBFA_CMB(LBFA_BF16, 128); }
#undef LBFA_CMB
  return hipGetLastError();
}

#endif  // LBFA_K4_UNIT

// ---- host-side launchers (called from lbfa_api.hip) ----------------------------------------------------------------------
// One launcher for the eight decodes: the KV policy and the formats of K and V are the block's (CacheBlock, lbfa_common.h).  The
// file is compiled twice: as it is for the byte-per-code blocks, with LBFA_K4_UNIT for the packed-K ones.
template <class P>
hipError_t launch_decode(const P& p, int dtype, int D, hipStream_t stream) {
  static_assert(CacheBlock<P>::op == CacheOp::kDecode, "not a parameter block of the decode kernels");
  using KV = std::conditional_t<CacheBlock<P>::paged, PagedKV, ContiguousKV>;
  constexpr int VB = CacheBlock<P>::v_bits, KB = CacheBlock<P>::k_bits;
  dim3 grid(p.splits, p.Hkv, p.B);
  const int mb = (p.M + 15) / 16;
#define LBFA_DEC(DT, DD, MB)                                                                                       \
  do {                                                                                                             \
    if constexpr (KB == 4 && VB == 8) hipLaunchKernelGGL((attn_decode_k4_v8_kernel<KV, DT, DD, MB>), grid, dim3(64), 0, stream, p); \
    else if constexpr (KB == 4) hipLaunchKernelGGL((attn_decode_k4_kernel<KV, DT, DD, MB>), grid, dim3(64), 0, stream, p); \
    else if constexpr (VB == 8) hipLaunchKernelGGL((attn_decode_v8_kernel<KV, DT, DD, MB>), grid, dim3(64), 0, stream, p); \
    else hipLaunchKernelGGL((attn_decode_kernel<KV, DT, DD, MB>), grid, dim3(64), 0, stream, p);                   \
  } while (0)
#define LBFA_DEC1(DT, DD)                 \
  do {                                    \
    if (mb <= 1) LBFA_DEC(DT, DD, 1);     \
    else if (mb == 2) LBFA_DEC(DT, DD, 2); \
    else LBFA_DEC(DT, DD, 4);             \
  } while (0)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_DEC1(LBFA_F16, 64); else LBFA_DEC1(LBFA_F16, 128); }
  else { if (D == 64) LBFA_DEC1(LBFA_BF16, 64); else LBFA_DEC1(LBFA_BF16, 128); }
#undef LBFA_DEC1
#undef LBFA_DEC
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.splits == 1) return e;
  return launch_attn_decode_combine(p, dtype, D, stream);  // the partials are indexed by row of the call: nothing paged in them
}
#ifndef LBFA_K4_UNIT
template hipError_t launch_decode(const DecodeParams&, int, int, hipStream_t);
template hipError_t launch_decode(const PagedDecodeParams&, int, int, hipStream_t);
template hipError_t launch_decode(const V8Params<DecodeParams, const float*>&, int, int, hipStream_t);
template hipError_t launch_decode(const V8Params<PagedDecodeParams, const float*>&, int, int, hipStream_t);
#else
template hipError_t launch_decode(const K4Params<DecodeParams>&, int, int, hipStream_t);
template hipError_t launch_decode(const K4Params<PagedDecodeParams>&, int, int, hipStream_t);
template hipError_t launch_decode(const K4Params<V8Params<DecodeParams, const float*>>&, int, int, hipStream_t);
template hipError_t launch_decode(const K4Params<V8Params<PagedDecodeParams, const float*>>&, int, int, hipStream_t);
#endif

}  // namespace lbfa
