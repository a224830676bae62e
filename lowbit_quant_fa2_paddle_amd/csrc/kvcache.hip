// Int8 KV cache for autoregressive decode (gfx950): the append kernel and the smooth-K mean of a ragged first append.
//
// Cache of one (batch, kv head): k_codes int8 [cap, D], k_scale fp32 [cap / 64], v fp16 [cap, D], and k_tail [64, D] in the
// storage dtype - the raw rows of the OPEN 64-key block (the block the next token falls into).  The K quantiser of the dense
// operators gives every 64-key block one scale taken from the rows present (quant_per_block_kernel, BLK = 64): a block that
// grows is therefore re-quantised from its raw rows, old ones from k_tail and new ones from the append, and every block that an
// append touches ends up with the codes and the scale the dense quantiser produces for that block of the concatenated K, bit
// for bit (same fp32 operations in the same order per element; the block maximum is order-independent).
//
// Work split: sequence b appends rows [s0, s0 + T_b), s0 = seqlens[b] read on the device.  They touch the blocks first = s0 / 64
// .. last = (s0 + T_b - 1) / 64.  Workgroup x = 0 of a (batch, head) owns BOTH ends: it reads k_tail for block `first`, and -
// behind a barrier - stores the rows of block `last` to k_tail when that block stays open.  No other workgroup touches k_tail, so
// any T from one token to a whole prompt is race-free and scheduling cannot change the result.  Workgroup x >= 1 takes the middle
// block first + x (whole 64 new rows, never open).  V rows are cast to fp16 by the workgroup that owns their block.
//
// ONE kernel body writes the contiguous cache and the paged one; where a 64-key block lives is the policy's (ContiguousDst /
// PagedDst): the slot a row of the call addresses with its range test, and the block's place with - paged - the page look-up
// and its range test.  seqlens, k_tail and km are indexed by SLOT, k_new / v_new / new_lens by ROW of the call.
// Built with -ffp-contract=off and correctly rounded fp32 division, as the quantiser is.
#include "lbfa_common.h"

namespace lbfa {

// lengths of the sequence in slot sl that row b of the call appends to, clipped so that nothing is written past the capacity
// (paged: cap = max_pages * page_size)
__device__ __forceinline__ void append_range(const AppendParams& p, int b, int sl, int& s0, int& tb) {
  s0 = min(max(p.seqlens[sl], 0), p.cap);
  tb = p.new_lens != nullptr ? min(max(p.new_lens[b], 0), p.T) : p.T;
  tb = min(tb, p.cap - s0);
}

// Contiguous cache [B, Hkv, cap, D] (scales [B, Hkv, cap / 64]): row b of the call is sequence b, block blk of (b, h) is block
// (b * Hkv + h) * (cap / 64) + blk of the cache seen as 64-key blocks.
struct ContiguousDst {
  typedef AppendParams Params;
  static __device__ __forceinline__ bool slot(const Params&, int b, int& sl) {
    sl = b;
    return true;
  }
  static __device__ __forceinline__ bool block(const Params& p, int sl, int h, int blk, int64_t& gb) {
    gb = ((int64_t)sl * p.Hkv + h) * (p.cap >> 6) + blk;
    return true;
  }
};
// Pool of pages: k_codes int8 / v fp16 [num_pages, Hkv, page_size, D], k_scale fp32 [num_pages, Hkv, page_size / 64]; block blk of
// the sequence in slot sl lives in page block_table[sl * max_pages + blk / (page_size / 64)].  page_size is a multiple of 64, so a
// quantiser block never straddles two pages.  Row b addresses slot slots[b], or b when slots is null.  Slot and page ids are
// device data the host cannot check: a row whose slot is outside [0, num_slots) is skipped, and so is a block whose page is
// outside [0, num_pages) - workgroup-uniform scalar tests; no address is ever formed from such an id.
struct PagedDst {
  typedef PagedAppendParams Params;
  static __device__ __forceinline__ bool slot(const Params& p, int b, int& sl) {
    sl = p.slots != nullptr ? p.slots[b] : b;
    return sl >= 0 && sl < p.num_slots;
  }
  static __device__ __forceinline__ bool block(const Params& p, int sl, int h, int blk, int64_t& gb) {
    const int bpp = p.page_size >> 6;  // 64-key blocks per page
    const int pg = p.block_table[(int64_t)sl * p.max_pages + blk / bpp];
    if (pg < 0 || pg >= p.num_pages) return false;
    gb = ((int64_t)pg * p.Hkv + h) * bpp + blk % bpp;  // block of the pool [num_pages, Hkv, page_size / 64]
    return true;
  }
};

// One appended V row as e4m3 codes with a scale of its own (the fp8 V cache, kv_policy.h), all in fp32: x = fp32(v), amax =
// max(max |x|, 1e-7) over the D channels, scale = amax / 448 (correctly rounded), code = e4m3fn_rne(x / scale).  |x / scale| stays
// below 448 (1 + 2^-23), so the conversion never depends on how it treats what lies past 464.  The CPR = D / 8 threads that hold the
// row (consecutive lanes, each 8 channels) reduce the amax among themselves; every one of them must call this.
template <int DT, int CPR>
__device__ __forceinline__ uint2 quant_v_row_e4m3(const u32x4& raw, float& scale) {
  float x[8];
  unpack8<DT>(raw, x);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
  for (int o = 1; o < CPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  scale = fmaxf(amax, 1e-7f) / 448.f;
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] / scale, x[1] / scale, w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] / scale, x[3] / scale, w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] / scale, x[5] / scale, w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] / scale, x[7] / scale, w1, true);
  return make_uint2((unsigned)w0, (unsigned)w1);
}

// The body is written once, in kvcache_append_body.inc, and included as text into both kernels: VB = bits of a cached V element, 16 (fp16) or 8
// (e4m3 codes with a scale per key, kv_policy.h).  Text, not a function the two kernels call: routed through an inlined function
// the fp16 instances compile to other code than they had (same instructions, another schedule), and they are the yardstick the fp8
// family is measured against.  Included, they are the code they were, byte for byte.
// K is quantised the same way in all of them; KB = bits of a stored K code: 8, or 4 for the nibble-packed cache (K4Params,
// lbfa_common.h), which differs in the store alone - a thread's 8 codes become 4 bytes of its own, no lane exchange.
template <class Dst, int DT, int D>
__global__ __launch_bounds__(256) void kvcache_append_kernel(typename Dst::Params p) {
  constexpr int VB = 16, KB = 8;
#include "kvcache_append_body.inc"
}
// the same kernel for the fp8 V cache; the name keeps its family apart from the fp16 one in the code object
template <class Dst, int DT, int D>
__global__ __launch_bounds__(256) void kvcache_append_v8_kernel(V8Params<typename Dst::Params, float*> p) {
  constexpr int VB = 8, KB = 8;
#include "kvcache_append_body.inc"
}
// the same two kernels for the nibble-packed K cache
template <class Dst, int DT, int D>
__global__ __launch_bounds__(256) void kvcache_append_k4_kernel(K4Params<typename Dst::Params> p) {
  constexpr int VB = 16, KB = 4;
#include "kvcache_append_body.inc"
}
template <class Dst, int DT, int D>
__global__ __launch_bounds__(256) void kvcache_append_k4_v8_kernel(K4Params<V8Params<typename Dst::Params, float*>> p) {
  constexpr int VB = 8, KB = 4;
#include "kvcache_append_body.inc"
}

#ifndef LBFA_K4_UNIT  // the mean kernel lives in the unit of the byte-per-code instances

// Smooth-K mean of a first append whose sequences have different lengths: km[b, h, :] = storage dtype of the fp32 of the float64
// mean over the new_lens[b] valid rows (zeros for an empty sequence).  One workgroup per (batch, head), fp64 sums in one fixed
// order.  (With equal lengths the caller uses lbfa_mean_seq, whose result the dense operators use.)
template <int DT, int D>
__global__ __launch_bounds__(256) void kvcache_mean_kernel(RaggedMeanParams p) {
  constexpr int CPR = D / 8;
  constexpr int RL = 256 / CPR;
  __shared__ double red[RL][D + 1];
  const int h = blockIdx.x, b = blockIdx.y;
  const int t = threadIdx.x, c = t % CPR, rl = t / CPR;
  const int n = min(max(p.new_lens[b], 0), p.T);
  const unsigned short* base = p.k_new + (int64_t)b * p.kb + (int64_t)h * p.kh + c * 8;
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0;
  for (int r = rl; r < n; r += RL) {
    float v[8];
    unpack8<DT>(*reinterpret_cast<const uint4*>(base + (int64_t)r * p.ks), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += (double)v[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[rl][c * 8 + i] = acc[i];
  __syncthreads();
  if (t < D) {
    double s = 0.0;
    for (int r = 0; r < RL; ++r) s += red[r][t];
    const float m = n > 0 ? (float)(s / (double)n) : 0.f;
    p.km[((int64_t)b * p.Hkv + h) * D + t] = store_cvt<DT>(m);
  }
}

#endif  // LBFA_K4_UNIT

// ---- host-side launchers (called from lbfa_api.hip) ---------------------------------------------------------------
static int kvcache_append_grid_x(int T) {
  // T rows starting anywhere in a block touch at most (T + 126) / 64 blocks; workgroup 0 takes the first and the last
  const int touched = (T + 126) / 64;
  return touched > 2 ? touched - 1 : 1;
}

// One launcher for the eight appends: the destination policy and the formats of K and V are the block's (CacheBlock,
// lbfa_common.h).  The file is compiled twice: as it is for the byte-per-code blocks, with LBFA_K4_UNIT for the packed-K ones.
template <class P>
hipError_t launch_append(const P& p, int dtype, int D, hipStream_t stream) {
  static_assert(CacheBlock<P>::op == CacheOp::kAppend, "not a parameter block of the append kernels");
  using Dst = std::conditional_t<CacheBlock<P>::paged, PagedDst, ContiguousDst>;
  constexpr int VB = CacheBlock<P>::v_bits, KB = CacheBlock<P>::k_bits;
  dim3 grid(kvcache_append_grid_x(p.T), p.Hkv, p.B);
#define LBFA_APP(DT, DD)                                                                                         \
  do {                                                                                                           \
    if constexpr (KB == 4 && VB == 8) hipLaunchKernelGGL((kvcache_append_k4_v8_kernel<Dst, DT, DD>), grid, dim3(256), 0, stream, p); \
    else if constexpr (KB == 4) hipLaunchKernelGGL((kvcache_append_k4_kernel<Dst, DT, DD>), grid, dim3(256), 0, stream, p); \
    else if constexpr (VB == 8) hipLaunchKernelGGL((kvcache_append_v8_kernel<Dst, DT, DD>), grid, dim3(256), 0, stream, p); \
    else hipLaunchKernelGGL((kvcache_append_kernel<Dst, DT, DD>), grid, dim3(256), 0, stream, p);                \
  } while (0)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_APP(LBFA_F16, 64); else LBFA_APP(LBFA_F16, 128); }
  else { if (D == 64) LBFA_APP(LBFA_BF16, 64); else LBFA_APP(LBFA_BF16, 128); }
#undef LBFA_APP
  return hipGetLastError();
}
#ifndef LBFA_K4_UNIT
template hipError_t launch_append(const AppendParams&, int, int, hipStream_t);
template hipError_t launch_append(const PagedAppendParams&, int, int, hipStream_t);
template hipError_t launch_append(const V8Params<AppendParams, float*>&, int, int, hipStream_t);
template hipError_t launch_append(const V8Params<PagedAppendParams, float*>&, int, int, hipStream_t);
#else
template hipError_t launch_append(const K4Params<AppendParams>&, int, int, hipStream_t);
template hipError_t launch_append(const K4Params<PagedAppendParams>&, int, int, hipStream_t);
template hipError_t launch_append(const K4Params<V8Params<AppendParams, float*>>&, int, int, hipStream_t);
template hipError_t launch_append(const K4Params<V8Params<PagedAppendParams, float*>>&, int, int, hipStream_t);
#endif

#ifndef LBFA_K4_UNIT
hipError_t launch_kvcache_mean(const RaggedMeanParams& p, int dtype, int B, int D, hipStream_t stream) {
  dim3 grid(p.Hkv, B);
#define LBFA_KM(DT, DD) hipLaunchKernelGGL((kvcache_mean_kernel<DT, DD>), grid, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_KM(LBFA_F16, 64); else LBFA_KM(LBFA_F16, 128); }
  else { if (D == 64) LBFA_KM(LBFA_BF16, 64); else LBFA_KM(LBFA_BF16, 128); }
#undef LBFA_KM
  return hipGetLastError();
}
#endif

}  // namespace lbfa
