// Append to the PAGED int8 KV cache (gfx950): kvcache_append_kernel (kvcache.hip - the open-block scheme, the work split and why
// the result is the dense quantiser's bit for bit are described there) writing into the pages of a pool.
//
// Pool: k_codes int8 / v fp16 [num_pages, Hkv, page_size, D], k_scale fp32 [num_pages, Hkv, page_size / 64]; 64-key block `blk` of
// the sequence in slot `sl` lives in page block_table[sl * max_pages + blk / (page_size / 64)].  page_size is a multiple of 64, so
// a quantiser block never straddles two pages and the quantiser is the same text.  seqlens, k_tail, km and the table are indexed
// by SLOT, k_new / v_new / new_lens by ROW of the call (row b addresses slot slots[b], or b when slots is null).  Workgroup 0 of
// a (row, head) owns both ends of the appended range, as in the contiguous kernel.
// Slot and page ids are device data the host cannot check: a row whose slot is outside [0, num_slots) is skipped, and so is a
// block whose page is outside [0, num_pages) - workgroup-uniform scalar tests; no address is ever formed from such an id.
//
// A COPY of kvcache_append_kernel's text, not a shared body: behind a PAGED flag the compiler assigned other registers and
// re-ordered instructions in all four contiguous instances, which have to stay the parent's instruction for instruction.
// Built with -ffp-contract=off and correctly rounded fp32 division, as the quantiser is.
#include "lbfa_common.h"

namespace lbfa {

int kvcache_append_grid_x(int T);  // kvcache.hip

template <int DT, int D>
__global__ __launch_bounds__(256) void kvcache_paged_append_kernel(PagedAppendParams p) {
  constexpr int CPR = D / 8;       // 16-byte chunks per row
  constexpr int RPP = 256 / CPR;   // rows per pass
  constexpr int NP = 64 / RPP;     // passes per 64-key block
  __shared__ float wmax[4];
  const int x = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, c = t % CPR, rl = t / CPR;
  const int sl = p.slots != nullptr ? p.slots[b] : b;
  if (sl < 0 || sl >= p.num_slots) return;  // workgroup-uniform
  // lengths of the sequence, clipped so that nothing is written past max_pages * page_size (= p.cap)
  const int s0 = min(max(p.seqlens[sl], 0), p.cap);
  int tb = p.new_lens != nullptr ? min(max(p.new_lens[b], 0), p.T) : p.T;
  tb = min(tb, p.cap - s0);
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
  const int bpp = p.page_size >> 6;  // 64-key blocks per page

  // x = 0: block `first`, then block `last` when it is another one; x >= 1: one middle block
  const int npass = (x == 0 && last > first) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const int blk = x > 0 ? first + x : (pass == 0 ? first : last);
    const int r0 = blk << 6;
    const int pg = p.block_table[(int64_t)sl * p.max_pages + blk / bpp];
    if (pg < 0 || pg >= p.num_pages) continue;  // workgroup-uniform, before the barriers of the pass: the block is skipped
    const int64_t gb = ((int64_t)pg * p.Hkv + h) * bpp + blk % bpp;  // block of the pool [num_pages, Hkv, page_size / 64]
    int8_t* codes = p.k_codes + gb * 64 * D + c * 8;                 // row r0 of the sequence
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

// ---- host-side launcher (called from lbfa_api.hip) ---------------------------------------------------------------
hipError_t launch_kvcache_paged_append(const PagedAppendParams& p, int dtype, int D, hipStream_t stream) {
  dim3 grid(kvcache_append_grid_x(p.T), p.Hkv, p.B);
#define LBFA_APP(DT, DD) hipLaunchKernelGGL((kvcache_paged_append_kernel<DT, DD>), grid, dim3(256), 0, stream, p)
  if (dtype == LBFA_F16) { if (D == 64) LBFA_APP(LBFA_F16, 64); else LBFA_APP(LBFA_F16, 128); }
  else { if (D == 64) LBFA_APP(LBFA_BF16, 64); else LBFA_APP(LBFA_BF16, 128); }
#undef LBFA_APP
  return hipGetLastError();
}

}  // namespace lbfa
