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

template <class Dst, int DT, int D>
__global__ __launch_bounds__(256) void kvcache_append_kernel(typename Dst::Params p) {
  constexpr int CPR = D / 8;       // 16-byte chunks per row
  constexpr int RPP = 256 / CPR;   // rows per pass
  constexpr int NP = 64 / RPP;     // passes per 64-key block
  __shared__ float wmax[4];
  const int x = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, c = t % CPR, rl = t / CPR;
  int sl, s0, tb;
  if (!Dst::slot(p, b, sl)) return;  // workgroup-uniform
  append_range(p, b, sl, s0, tb);
  if (tb <= 0) return;  // workgroup-uniform
  const int first = s0 >> 6, last = (s0 + tb - 1) >> 6;
  if (x > 0 && first + x >= last) return;
  const int64_t sh = (int64_t)sl * p.Hkv + h;  // (slot, head): k_tail, km
  const unsigned short* knew = p.k_new + (int64_t)b * p.kb + (int64_t)h * p.kh + c * 8;
  const unsigned short* vnew = p.v_new + (int64_t)b * p.vb + (int64_t)h * p.vh + c * 8;
  unsigned short* tail = p.k_tail + sh * 64 * D + c * 8;
  float mean[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) mean[i] = 0.f;
  const bool has_mean = p.km != nullptr;
  if (has_mean) unpack8<DT>(*reinterpret_cast<const uint4*>(p.km + sh * D + c * 8), mean);
  const int end = s0 + tb;

  // x = 0: block `first`, then block `last` when it is another one; x >= 1: one middle block
  const int npass = (x == 0 && last > first) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const int blk = x > 0 ? first + x : (pass == 0 ? first : last);
    const int r0 = blk << 6;
    int64_t gb;
    if (!Dst::block(p, sl, h, blk, gb)) continue;     // workgroup-uniform, before the barriers of the pass: the block is skipped
    int8_t* codes = p.k_codes + gb * 64 * D + c * 8;  // row r0 of the sequence
    unsigned short* vdst = p.v + gb * 64 * D + c * 8;
    uint4 raw[NP];
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      raw[ps] = make_uint4(0, 0, 0, 0);
      if (row < s0) raw[ps] = *reinterpret_cast<const uint4*>(tail + (int64_t)(row - r0) * D);  // only block `first` has such rows
      else if (row < end) raw[ps] = *reinterpret_cast<const uint4*>(knew + (int64_t)(row - s0) * p.ks);
    }
    float xs[NP][8];
    float amax = 0.f;
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      float v[8];
      unpack8<DT>(raw[ps], v);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float xv = v[i];
        // `k - km` in the storage dtype, rows past the end stay 0: exactly quant_per_block_kernel (sm_scale = 1 for K)
        if (has_mean) xv = (row < end) ? load_cvt<DT>(store_cvt<DT>(xv - mean[i])) : 0.f;
        xs[ps][i] = xv;
        amax = fmaxf(amax, fabsf(xv));
      }
    }
    amax = wave_max_nonneg(amax);
    if ((t & 63) == 0) wmax[t >> 6] = amax;
    __syncthreads();  // also: every read of k_tail (pass 0) is done before pass 1 stores to it
    const float scale = block_scale(amax_collect(wmax), p.qmax);
    if (t == 0) p.k_scale[gb] = scale;
    const bool open = (blk == last) && (end & 63) != 0;  // this block is the open one afterwards: keep its raw rows
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      int q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = quant_code<false>(xs[ps][i], scale, 0.f);  // the plain division
      if (row < end) *reinterpret_cast<uint2*>(codes + (int64_t)(row - r0) * D) = pack8_i8(q);
      if (row >= s0 && row < end) {
        if (open) *reinterpret_cast<uint4*>(tail + (int64_t)(row - r0) * D) = raw[ps];
        u32x4 vr = *reinterpret_cast<const u32x4*>(vnew + (int64_t)(row - s0) * p.vs);
        if constexpr (DT == LBFA_BF16) vr = bf16x8_to_f16x8(vr);
        *reinterpret_cast<u32x4*>(vdst + (int64_t)(row - r0) * D) = vr;
      }
    }
    __syncthreads();  // wmax is reused by the second pass
  }
}

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

// ---- host-side launchers (called from lbfa_api.hip) ---------------------------------------------------------------
static int kvcache_append_grid_x(int T) {
  // T rows starting anywhere in a block touch at most (T + 126) / 64 blocks; workgroup 0 takes the first and the last
  const int touched = (T + 126) / 64;
  return touched > 2 ? touched - 1 : 1;
}

template <class Dst>
static hipError_t launch_append(const typename Dst::Params& p, int dtype, int D, hipStream_t stream) {
  dim3 grid(kvcache_append_grid_x(p.T), p.Hkv, p.B);
#define LBFA_APP(DT, DD) hipLaunchKernelGGL((kvcache_append_kernel<Dst, DT, DD>), grid, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_APP(LBFA_F16, 64); else LBFA_APP(LBFA_F16, 128); }
  else { if (D == 64) LBFA_APP(LBFA_BF16, 64); else LBFA_APP(LBFA_BF16, 128); }
#undef LBFA_APP
  return hipGetLastError();
}
hipError_t launch_kvcache_append(const AppendParams& p, int dtype, int D, hipStream_t stream) {
  return launch_append<ContiguousDst>(p, dtype, D, stream);
}
hipError_t launch_kvcache_paged_append(const PagedAppendParams& p, int dtype, int D, hipStream_t stream) {
  return launch_append<PagedDst>(p, dtype, D, stream);
}

hipError_t launch_kvcache_mean(const RaggedMeanParams& p, int dtype, int B, int D, hipStream_t stream) {
  dim3 grid(p.Hkv, B);
#define LBFA_KM(DT, DD) hipLaunchKernelGGL((kvcache_mean_kernel<DT, DD>), grid, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_KM(LBFA_F16, 64); else LBFA_KM(LBFA_F16, 128); }
  else { if (D == 64) LBFA_KM(LBFA_BF16, 64); else LBFA_KM(LBFA_BF16, 128); }
#undef LBFA_KM
  return hipGetLastError();
}

}  // namespace lbfa
