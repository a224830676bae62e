// Cached prefill: attention of ANY number of new queries to the int8 KV cache (kvcache.hip), contiguous or paged, gfx950.
//
// One workgroup = FOUR waves = one (batch, query head, 128-row Q block, key slice); each wave owns 32 query rows as two 16-row
// blocks (the MB = 2 shape of attn_decode.hip), with that kernel's lane roles, MFMA shapes and tile arithmetic - not a copy of it:
// both bodies include the one text of it, attn_cache_tile.inc (running state, tile bases, load_k / load_v / store_v / compute):
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

// The body is written once, in attn_prefill_body.inc, and included as text into both kernels: VB = bits of a cached V element, 16 (fp16) or 8
// (e4m3 codes with a scale per key, kv_policy.h).  Text, not a function the two kernels call: routed through an inlined function
// the fp16 instances compile to other code than they had (same instructions, another schedule), and they are the yardstick the fp8
// family is measured against.  Included, they are the code they were, byte for byte.  The body includes attn_cache_tile.inc, the
// text it shares with the decode body: a V tile belongs to the 256 threads here (NT, tix), the Q scale is the block's, and a tile
// below every row limit of the wave calls compute without the key-limit compare.
// The V format is known to load_v and store_v only; KB = bits of a cached K code, known to load_k and the score product only.
template <class KV, int DT, int D>
__global__ __launch_bounds__(256) void attn_prefill_kernel(typename PrefillOf<KV>::type p) {
  constexpr int VB = 16, KB = 8;
#include "attn_prefill_body.inc"
}
// the same kernel over the fp8 V cache; the name keeps its family apart from the fp16 one in the code object
template <class KV, int DT, int D>
__global__ __launch_bounds__(256) void attn_prefill_v8_kernel(V8Params<typename PrefillOf<KV>::type, const float*> p) {
  constexpr int VB = 8, KB = 8;
#include "attn_prefill_body.inc"
}
// the same two kernels over the nibble-packed K cache (K4Params, lbfa_common.h): half the K bytes per key, widened in registers
template <class KV, int DT, int D>
__global__ __launch_bounds__(256) void attn_prefill_k4_kernel(K4Params<typename PrefillOf<KV>::type> p) {
  constexpr int VB = 16, KB = 4;
#include "attn_prefill_body.inc"
}
template <class KV, int DT, int D>
__global__ __launch_bounds__(256) void attn_prefill_k4_v8_kernel(K4Params<V8Params<typename PrefillOf<KV>::type, const float*>> p) {
  constexpr int VB = 8, KB = 4;
#include "attn_prefill_body.inc"
}

// ---- host-side launchers (called from lbfa_api.hip) ----------------------------------------------------------------------
// One launcher for the eight cached prefills: the KV policy and the formats of K and V are the block's (CacheBlock,
// lbfa_common.h).  The file is compiled twice: as it is for the byte-per-code blocks, with LBFA_K4_UNIT for the packed-K ones.
template <class P>
hipError_t launch_prefill(const P& p, int dtype, int D, hipStream_t stream) {
  static_assert(CacheBlock<P>::op == CacheOp::kPrefill, "not a parameter block of the prefill kernels");
  using KV = std::conditional_t<CacheBlock<P>::paged, PagedKV, ContiguousKV>;
  constexpr int VB = CacheBlock<P>::v_bits, KB = CacheBlock<P>::k_bits;
  dim3 grid((unsigned)p.nQ * (unsigned)p.splits, p.Hq, p.B);
#define LBFA_PRE(DT, DD)                                                                                        \
  do {                                                                                                          \
    if constexpr (KB == 4 && VB == 8) hipLaunchKernelGGL((attn_prefill_k4_v8_kernel<KV, DT, DD>), grid, dim3(256), 0, stream, p); \
    else if constexpr (KB == 4) hipLaunchKernelGGL((attn_prefill_k4_kernel<KV, DT, DD>), grid, dim3(256), 0, stream, p); \
    else if constexpr (VB == 8) hipLaunchKernelGGL((attn_prefill_v8_kernel<KV, DT, DD>), grid, dim3(256), 0, stream, p); \
    else hipLaunchKernelGGL((attn_prefill_kernel<KV, DT, DD>), grid, dim3(256), 0, stream, p);                  \
  } while (0)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_PRE(LBFA_F16, 64); else LBFA_PRE(LBFA_F16, 128); }
  else { if (D == 64) LBFA_PRE(LBFA_BF16, 64); else LBFA_PRE(LBFA_BF16, 128); }
#undef LBFA_PRE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.splits == 1) return e;
  return launch_attn_decode_combine(p, dtype, D, stream);  // the partials are the decode kernel's: its second launch, unchanged
}
#ifndef LBFA_K4_UNIT
template hipError_t launch_prefill(const PrefillParams&, int, int, hipStream_t);
template hipError_t launch_prefill(const PagedPrefillParams&, int, int, hipStream_t);
template hipError_t launch_prefill(const V8Params<PrefillParams, const float*>&, int, int, hipStream_t);
template hipError_t launch_prefill(const V8Params<PagedPrefillParams, const float*>&, int, int, hipStream_t);
#else
template hipError_t launch_prefill(const K4Params<PrefillParams>&, int, int, hipStream_t);
template hipError_t launch_prefill(const K4Params<PagedPrefillParams>&, int, int, hipStream_t);
template hipError_t launch_prefill(const K4Params<V8Params<PrefillParams, const float*>>&, int, int, hipStream_t);
template hipError_t launch_prefill(const K4Params<V8Params<PagedPrefillParams, const float*>>&, int, int, hipStream_t);
#endif

}  // namespace lbfa
