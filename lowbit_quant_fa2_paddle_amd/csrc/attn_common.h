// Device helpers shared by the attention kernels (gfx950).
#pragma once
#include <type_traits>

#include "lbfa_common.h"

namespace lbfa {

// ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block of 16-bit elements, delivered column-major (lane i gets column
// i of the 4 rows).  EXEC must be all ones.  Issued behind the compiler's back (inline asm, no memory operand): the intrinsic form
// following a `buffer_load ... lds` makes the compiler wait for vmcnt(0) first - it cannot know that the DMA in flight fills the
// OTHER buffer - which parks every wave in the middle of each tile until the prefetch has landed.  The result is valid only
// after lds_wait_keep() has been given the registers.
template <int OFF>
__device__ __forceinline__ f16x4 lds_read_tr16_raw(unsigned lds_addr) {
  f16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "n"(OFF));
  return v;
}
// Wait until at most N operations issued AFTER the reads that produced these registers are still in flight.  N = the reads
// this wave has requested since (LDS returns in order).  Anything else the compiler has outstanding on the same counter (its own
// LDS reads, scalar loads - which may return out of order) only makes the wait stricter: the count cannot fall to N while one
// of the older reads is pending, because N younger LDS reads stand behind it.
template <int N>
__device__ __forceinline__ void lds_wait_keep(f16x4& a, f16x4& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait_keep(f16x4& a, f16x4& b, f16x4& c, f16x4& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait_keep(f16x4& a, f16x4& b, f16x4& c, f16x4& d, f16x4& e, f16x4& f, f16x4& g, f16x4& h) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(N));
}
__device__ __forceinline__ unsigned lds_offset_of(const void* shared_ptr) {
  return (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) const char*)shared_ptr;
}

template <int RB>
__device__ __forceinline__ int kx(int row) {  // K-tile 16-B chunk swizzle for rows of RB bytes (int8: RB = D, fp16: 2 D)
  if constexpr (RB == 64) return (row >> 2) & 3;
  else if constexpr (RB == 128) return (row >> 1) & 7;
  else return row & 15;
}

__device__ __forceinline__ float half_swap_max(float x) {
  // max over the two 32-lane halves holding the same query row
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_swap_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- reductions over the four lanes l, l + 16, l + 32, l + 48 (one lane per 16-lane row) without the LDS crossbar -----------
// v_permlane16_swap exchanges the odd rows of its first operand with the even rows of the second, v_permlane32_swap the two
// halves: after each step both partners hold both values.  Two VALU instructions per step instead of a ds_bpermute round trip.
__device__ __forceinline__ float rows4_sum(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// "Order keys": the scores of the int8 product are the accumulator bits of kMagic + s, which compare like the integers s as
// signed int32 (-inf = 0xFF800000 sorts below all of them) - integer maxima need no NaN canonicalisation in front and come as
// v_max3_i32.  The fp32 scores of the un-quantised product compare as floats: max(a, b) = med3(a, b, +inf), one v_med3_f32
// without the canonicalising v_max the compiler puts in front of an fmaxf on MFMA output.  (Not inline asm: hipcc pads no
// MFMA -> VALU wait states for an asm statement's operands - a hand-written v_max3_f32 read the score accumulators early.)
template <bool AS_INT>
__device__ __forceinline__ float key_max(float a, float b) {
  if constexpr (AS_INT) {
    const int x = __float_as_int(a), y = __float_as_int(b);
    return __int_as_float(x > y ? x : y);
  } else {
    return __builtin_amdgcn_fmed3f(a, b, __builtin_inff());
  }
}
template <bool AS_INT>
__device__ __forceinline__ float key_max3(float a, float b, float c) {
  return key_max<AS_INT>(key_max<AS_INT>(a, b), c);  // int: selected as v_max3_i32
}
template <bool AS_INT>
__device__ __forceinline__ float rows4_key_max(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = key_max<AS_INT>(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return key_max<AS_INT>(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// Raw buffer resource over [base, base+bytes): out-of-range loads return 0 (hardware bounds check).
// Built from kernel arguments and blockIdx-derived scalars only, so it stays in SGPRs.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

constexpr float kFp8Offset = 8.807f;  // csrc/qattn/attn_utils.cuh:30: p = exp2(s - m + 8.807) -> p_max = 448
constexpr float kMagic = 12582912.0f;  // 1.5 * 2^23: int32 accumulator bits == float(kMagic + s) for |s| < 2^22
constexpr int kMagicBits = 0x4B400000;
constexpr int kQInt8 = 3;  // QT of the attention kernel: int8 codes; LBFA_F16 / LBFA_BF16 = un-quantised Q and K

// ---- prologue and epilogue shared by the two forward kernels (attn_fwd.hip: fp8 PV, attn_fwd16.hip: fp16 P) -----------------
// Which (q-block, batch, head, kv head) this workgroup takes: XCD remap of the 1-D grid, causal: heaviest q-blocks of a head first.
struct WorkItem {
  int qt, b, h, hk;
};
template <bool CAUSAL>
__device__ __forceinline__ WorkItem work_item(const AttnParams& p) {
  const unsigned w_id = xcd_remap(blockIdx.x, gridDim.x);
  int qt = (int)(w_id % (unsigned)p.nQ);
  const int bh = (int)(w_id / (unsigned)p.nQ);
  if constexpr (CAUSAL) qt = p.nQ - 1 - qt;
  const int b = bh / p.Hq, h = bh % p.Hq;
  return WorkItem{qt, b, h, h / p.group};
}

// The problem a workgroup works on: batch entry b of a dense call, or sequence b of a packed variable-length batch
// (attn_qk_int8_block_varlen.py:125-141).  Offsets in elements, without the head term.
struct Problem {
  int Sq, Sk, nK;
  int64_t q_off, k_off, v_off, o_off;
  int64_t qsc_base, ksc_base;  // scale index of block 0 of head 0
  int64_t lse_base;            // LSE index of query row 0: [B,Hq,Sq], packed [Hq, total_q]
  int vec_b;                   // which q_dot_vec set: one per batch entry, packed: one mean over all tokens
  bool no_work;                // this q-block lies past the end of the sequence: return, whole workgroup, before any barrier
};
__device__ __forceinline__ Problem locate_problem(const AttnParams& p, int b, int h, int qt) {
  Problem r;
  r.Sq = p.Sq; r.Sk = p.Sk; r.nK = p.nK;
  r.q_off = (int64_t)b * p.qb; r.k_off = (int64_t)b * p.kb; r.v_off = (int64_t)b * p.vb; r.o_off = (int64_t)b * p.ob;
  r.qsc_base = (int64_t)b * p.qsc_b; r.ksc_base = (int64_t)b * p.ksc_b;
  r.lse_base = ((int64_t)b * p.Hq + h) * p.Sq;
  r.vec_b = b;
  r.no_work = false;
  if (p.cu_q != nullptr) {
    const int q0 = p.cu_q[b], k0 = p.cu_k[b];
    r.lse_base = (int64_t)h * p.lse_hs + q0;
    r.vec_b = 0;
    // max_seqlen_q / max_seqlen_k (p.Sq / p.Sk) size the grid and the padded scale rows: a sequence longer than the
    // caller's maximum is cut there, so that every access stays inside the buffers sized from those maxima
    r.Sq = min(p.cu_q[b + 1] - q0, p.Sq);
    r.Sk = min(p.cu_k[b + 1] - k0, p.Sk);
    r.no_work = qt * 128 >= r.Sq;
    r.nK = (r.Sk + 63) >> 6;
    r.q_off = (int64_t)q0 * p.qs;
    r.k_off = (int64_t)k0 * p.ks;
    r.v_off = (int64_t)k0 * p.vs;
    r.o_off = (int64_t)q0 * p.os;
    if (p.cu_qscale != nullptr) {
      r.qsc_base = (int64_t)p.cu_qscale[b] * p.qsc_b;
      r.ksc_base = (int64_t)p.cu_kscale[b] * p.ksc_b;
    }
  }
  return r;
}

// LDS-DMA fetch of tile j of one operand: NCH passes of 256 threads x 16 bytes, written linearly from lds_dst (wave-uniform, + 16
// bytes per lane, implicit).  The descriptor is re-based per tile with scalar arithmetic and covers what is left of the operand's
// `bytes` (< 2 GiB, checked by the C ABI), so rows past the end read as zeros with no per-lane guard; the look-ahead past either
// end (!in_range) gets a window of 0 bytes.  goff: the thread's loop-invariant source offset (swizzle included), gstep: bytes
// between a thread's chunks.
typedef __attribute__((address_space(3))) void* lds_void_ptr;
template <int NCH>
__device__ __forceinline__ void fetch_tile(const char* base, int bytes, int tile_stride, int j, bool in_range, char* lds_dst,
                                           unsigned goff, unsigned gstep) {
  const int off = in_range ? j * tile_stride : 0;
  const int rem = in_range ? max(0, bytes - off) : 0;
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(base + off, (unsigned)rem);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_ptr)(lds_dst + i * 4096), 16, (int)goff, (int)(i * gstep), 0, 0);
}

// Processing order of the key tiles.  Non-causal: every other ROUND of Q blocks of a head (kRound = the workgroups one XCD runs
// at a time) walks the key tiles from the last one down (see attn_fwd.hip); the direction depends on the Q block index only.
template <bool CAUSAL, int kRound>
__device__ __forceinline__ bool walks_back(int Sk, int qt) {
  return !CAUSAL && ((Sk & 63) == 0) && (((qt / kRound) & 1) != 0);  // workgroup-uniform
}
__device__ __forceinline__ int tile_at(bool rev, int nK, int i) { return rev ? nK - 1 - i : i; }  // i-th tile processed

// Scale grid of the exact bias folding (see attn_fwd.hip): the largest k_scale of this (batch, kv head) - lane l has tile l's in
// ks_first - and log2 of the power of two G chosen from the largest dequantisation scale.
__device__ __forceinline__ float max_k_scale(const float* ksc, int ksc_blk, int nK, int lane, float ks_first) {
  float ks_max = ks_first;
  for (int i = lane + 64; i < nK; i += 64) ks_max = fmaxf(ks_max, ksc[i * ksc_blk]);
  return fmaxf(wave_max_nonneg(ks_max), 1e-30f);  // scales are positive (the quantiser floors amax)
}
__device__ __forceinline__ int grid_exponent(float sc_max) {
  return __builtin_amdgcn_readfirstlane((int)((__float_as_uint(1.25f * kMagic * sc_max) >> 23) & 0xff) - 127 + 1 - 21);
}
// lane l: the raw k_scale of tile j0 + l (0 past the end)
__device__ __forceinline__ float k_scale_of_lane(const float* ksc, int ksc_blk, int nK, int j0, int lane, float ks_first) {
  const int jt = j0 + lane;
  return j0 == 0 ? ks_first : (jt < nK ? ksc[jt * ksc_blk] : 0.f);
}
// ... and the dequantisation scale the tile loop uses for it: un-rounded for a `wide` wave, else on the grid of step g = 1 / invg.
// At least 1e-30 / one grid step: a block whose scale is < 2^-22 of the largest one (an all-zero K block) must not get sc = 0, or
// a masked key (tv = -inf) would turn into fma(-inf, 0, c1) = NaN
__device__ __forceinline__ float wide_scale(float qsc, float ks_l) { return fmaxf(qsc * ks_l, 1e-30f); }
__device__ __forceinline__ float tile_scale(float qsc, float ks_l, float g, float invg, bool wide) {
  float sc = fmaxf(__builtin_rintf(qsc * ks_l * invg), 1.0f) * g;
  if (wide) sc = wide_scale(qsc, ks_l);  // (a statement, not a select: the select cost the D = 128 causal instances registers)
  return sc;
}

// LSE of one query row from its base-2 value: lse_out = lse2 * lse_scale + corr * lse_corr_scale (src/core.py:344-350), corr = the
// q . km computed in the kernel (QQ) or read from lse_corr
template <bool QQ>
__device__ __forceinline__ void store_lse(const AttnParams& p, int64_t li, float lse2, float row_corr) {
  float ls = lse2 * p.lse_scale;
  if constexpr (QQ) ls += row_corr * p.lse_corr_scale;  // 0 when there is no smoothing vector
  else if (p.lse_corr != nullptr) ls += p.lse_corr[li] * p.lse_corr_scale;
  p.lse[li] = ls;
}

// host: launches the causal or the plain instance of a forward kernel, one workgroup of 256 threads per 128-row Q block
template <typename Kernel>
inline hipError_t launch_fwd(Kernel causal_kernel, Kernel plain_kernel, int causal, const AttnParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(causal ? causal_kernel : plain_kernel, dim3((unsigned)p.B * p.Hq * p.nQ), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace lbfa
