// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of liblowbit_fa_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/lowbit_fa.h"

namespace lbfa {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;

// ---- storage-dtype conversions (raw 16-bit patterns <-> fp32) -------------------------------------
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) { return __uint_as_float(((unsigned)b) << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  // round-to-nearest-even; NaN stays NaN (plain cast lowers to v_cvt_pk_bf16_f32 on gfx950)
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float f16_bits_to_f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ unsigned short f32_to_f16_bits(float f) {
  _Float16 h = (_Float16)f;
  return __builtin_bit_cast(unsigned short, h);
}
template <int DT>
__device__ __forceinline__ float load_cvt(unsigned short b) {
  if constexpr (DT == LBFA_F16) return f16_bits_to_f32(b);
  else return bf16_bits_to_f32(b);
}
template <int DT>
__device__ __forceinline__ unsigned short store_cvt(float f) {
  if constexpr (DT == LBFA_F16) return f32_to_f16_bits(f);
  else return f32_to_bf16_bits(f);
}

// ---- wave-level reductions ------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// max over the wave of NON-NEGATIVE finite floats (no NaN) without the LDS crossbar: four DPP steps inside each row of 16
// lanes, v_permlane32_swap across the halves, row_bcast:15 across neighbouring rows; lane 63 then holds the maximum.
// Returned wave-uniform (SGPR).  ~8 VALU instructions instead of 6 ds_bpermute round trips.
__device__ __forceinline__ float wave_max_nonneg(float v) {
  auto dpp_max = [](float x, auto ctrl) {
    const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, true);  // invalid lanes read 0
    return fmaxf(x, __int_as_float(y));
  };
  v = dpp_max(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
  v = dpp_max(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
  v = dpp_max(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
  v = dpp_max(v, std::integral_constant<int, 0x140>{});  // row_mirror: every lane of a row holds the row's max
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));  // rows 0|2 and 1|3 combined
  v = dpp_max(v, std::integral_constant<int, 0x142>{});     // row_bcast:15 - row k takes lane 15 of row k - 1
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}

// ---- the int8 block quantiser's arithmetic: the one statement that quant_per_block_kernel, the KV-cache append, the decode
// kernel and the in-kernel Q quantisers of the forward kernels share (their codes and scales agree bit for bit) -----------------
// A 16-byte chunk (uint4 or u32x4) = 8 elements of the storage dtype: unpack8 converts all eight; elem16 converts element e, for
// the loops that consume each element as it is converted (the q . km dot products, the V encoder) - unpacking the whole chunk
// in front of them re-orders their instruction streams
template <int DT, typename Chunk>
__device__ __forceinline__ float elem16(Chunk raw, int e) {
  const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
  return load_cvt<DT>((unsigned short)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu)));
}
template <int DT, typename Chunk>
__device__ __forceinline__ void unpack8(const Chunk& raw, float (&v)[8]) {
  const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = load_cvt<DT>((unsigned short)(w[i] & 0xffffu));
    v[2 * i + 1] = load_cvt<DT>((unsigned short)(w[i] >> 16));
  }
}
// bf16 pairs -> fp16 pairs, in place (a 16-byte chunk = 8 elements)
__device__ __forceinline__ u32x4 bf16x8_to_f16x8(u32x4 val) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = __uint_as_float(val[e] << 16), hi = __uint_as_float(val[e] & 0xffff0000u);
    const f16x2 pk = f16x2{(_Float16)lo, (_Float16)hi};
    val[e] = __builtin_bit_cast(unsigned, pk);
  }
  return val;
}
// workgroup amax of four waves from the four LDS floats they posted their maxima to; the barriers are the caller's
__device__ __forceinline__ float amax_collect(const float* w4) { return fmaxf(fmaxf(w4[0], w4[1]), fmaxf(w4[2], w4[3])); }

__device__ __forceinline__ float block_scale(float amax, float qmax) { return fmaxf(amax, 1e-7f) / qmax; }
// y = x / scale must be the correctly rounded fp32 quotient (the codes are bit-exact against the oracle).  A full IEEE division
// per element costs ~12 VALU ops; the divisor is the same for the whole block, so FAST uses Markstein's sequence with the
// correctly rounded reciprocal rcp = 1 / scale: q0 = x*r, e = fma(-q0, s, x) (exact), q1 = fma(e, r, q0) == RN(x/s) for every
// x unless the significand of s is all ones (checked on 1.2e8 adversarial samples; theorem: Markstein 1990), in which case the
// plain division is used: markstein_ok(scale) picks, block-uniform, between two straight-line instances of the encode loop.
__device__ __forceinline__ bool markstein_ok(float scale) {
  return (__builtin_amdgcn_readfirstlane(__float_as_uint(scale)) & 0x7fffffu) != 0x7fffffu;
}
template <bool FAST>
__device__ __forceinline__ int quant_code(float x, float scale, float rcp) {
  float y;
  if constexpr (FAST) {
    const float q0 = x * rcp;
    y = __builtin_fmaf(__builtin_fmaf(-q0, scale, x), rcp, q0);
  } else {
    y = x / scale;
  }
  // round half away from zero (src/triton/quant_per_block.py:174-176): y + 0.5*sign(y), then truncate (v_cvt_i32_f32 truncates)
  return (int)(y + __builtin_copysignf(0.5f, y));
}
// |q| <= 127: v_cvt_pk_i16_i32 keeps the low bytes, v_perm_b32 gathers bytes 0 and 2 of each pair
__device__ __forceinline__ unsigned pack4_i8(const int* q) {
  const unsigned p01 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[0], q[1]));
  const unsigned p23 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[2], q[3]));
  return __builtin_amdgcn_perm(p23, p01, 0x06040200u);
}
// (pairs taken from the top down: the order in which the compiler laid out the spelled-out pack of the row quantisers, whose
// stores sit in a conditional block; the straight-line sites use pack4_i8)
__device__ __forceinline__ uint2 pack8_i8(const int (&q)[8]) {
  const unsigned p67 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[6], q[7]));
  const unsigned p45 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[4], q[5]));
  const unsigned hi = __builtin_amdgcn_perm(p67, p45, 0x06040200u);
  const unsigned p23 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[2], q[3]));
  const unsigned p01 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(q[0], q[1]));
  return make_uint2(__builtin_amdgcn_perm(p23, p01, 0x06040200u), hi);
}
// 16 consecutive elements of a row -> their 16 codes, as the int8 MFMAs take them (one operand of 16 bytes per lane)
template <bool FAST>
__device__ __forceinline__ i32x4 quant_codes16(const float (&x)[16], float scale, float rcp) {
  unsigned w[4];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = quant_code<FAST>(x[4 * g4 + e], scale, rcp);
    w[g4] = pack4_i8(q);
  }
  return i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

// XCD-aware bijective remap of a 1-D grid: hardware deals consecutive workgroup ids round-robin over
// the 8 XCDs, so ids {x, x+8, x+16, ...} share one L2.  Give each such residue class a CONTIGUOUS
// chunk of the logical work list, so that neighbours in the work list (same (batch, kv-head): same
// K/V panel) hit one XCD's L2.  Speed only - any placement is correct.
__device__ __forceinline__ unsigned xcd_remap(unsigned id, unsigned n) {
  const unsigned xcd = id & 7u, j = id >> 3;
  const unsigned q = n >> 3, r = n & 7u;
  const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + j;
}

// ---- launch parameter blocks shared by the kernels and the C-ABI layer ---------------------------
struct QuantParams {
  const unsigned short* x;
  const unsigned short* mean;        // [B, H/mean_group, D] or null
  int8_t* out;
  float* scale;                      // [B,H,nblk]
  const unsigned short* rowdot_vec;  // [B, H/rowdot_group, D] or null
  float* rowdot_out;                 // [B,H,S]
  int64_t xb, xh, xs, ob, oh, os;
  float sm_scale, qmax;
  int B, H, S, nblk, mean_group, rowdot_group;
  // scale index = base(b) + h * scale_h + blk * scale_blk, base(b) = (cu_scale ? cu_scale[b] : b) * scale_b.
  // Dense [B,H,nblk]: (H*nblk, nblk, 1).  The reference's packed layout [sum_blocks, H]
  // (src/triton/quant_per_block_varlen.py:60,101-106): (H, 1, H) with cu_scale.
  int64_t scale_b, scale_h, scale_blk;
  // Packed variable-length batch (src/core.py:356-491): sequence b owns tokens [cu_seqlens[b], cu_seqlens[b+1]) of
  // x / out (batch strides unused), blocks restart at each sequence.  null = dense.
  const int* cu_seqlens;
  const int* cu_scale;
  int d_valid;  // columns >= d_valid of x are padding: not read, codes 0 (head-dim pad of src/core.py:277-287 without a copy)
  int mean_b;  // 1: mean / rowdot_vec are per batch entry; 0: one vector set shared by all (varlen k.mean(dim=0), :453)
  // Fused last step of the mean (lbfa_forward): instead of reading `mean`, every workgroup adds the fp64 partial sums of its
  // (batch, head) itself - [.., mean_nsplit, D] doubles written by mean_partial_kernel, same order and roundings as
  // mean_finalize_kernel - and the workgroup of block 0 stores the result to `mean_out` (for the LSE correction q . km).
  const double* mean_partial;  // null: read `mean`
  unsigned short* mean_out;    // may be null
  int mean_nsplit, mean_S;
  // packed batch only: rowdot_out is [H, total] with head stride rowdot_hs (row r of sequence b at cu_seqlens[b] + r), and
  // sequence lengths are cut at s_cap (the attention kernel's in-kernel Q quantiser cuts at max_seqlen_q; INT_MAX: uncut)
  int64_t rowdot_hs;
  int s_cap;
};

struct AttnParams {
  const int8_t* q;
  const int8_t* k;
  const void* v;
  void* o;
  float* lse;
  const float* q_scale;
  const float* k_scale;
  const float* v_scale;
  int64_t qb, qh, qs, kb, kh, ks, vb, vh, vs, ob, oh, os;
  int B, Hq, Hkv, Sq, Sk, nQ, nK, group;
  // LSE post-processing (src/core.py:344-350): lse_out = (log2(l) + m) * lse_scale + lse_corr[b,h,s] * lse_corr_scale.
  // lbfa_attn_fwd uses (1, null): the raw base-2 value the reference kernel stores.
  const float* lse_corr;
  float lse_scale, lse_corr_scale;
  // scale addressing as in QuantParams; packed variable-length batch when cu_q != null (then cu_k too):
  // (src/triton/attn_qk_int8_block_varlen.py:125-160), Sq / Sk / nQ / nK hold the maxima over the batch.
  int64_t qsc_b, qsc_h, qsc_blk, ksc_b, ksc_h, ksc_blk;
  const int* cu_q;
  const int* cu_k;
  const int* cu_qscale;
  const int* cu_kscale;
  int d_valid;  // channels >= d_valid of V / O are padding: V reads as 0, O is not written (o has d_valid columns)
  float qk_scale;  // un-quantised Q / K only: sm_scale * log2(e), applied to the fp32 scores
  // Q quantised inside the attention kernel (one-call operators): q points at the fp16 / bf16 source (dtype = o's, strides in
  // elements), each workgroup quantises its own 128-row block exactly as quant_per_block_kernel does (same codes and scale),
  // and the LSE correction q . km comes from the same registers (q_dot_vec = km [B,Hkv,D] or null).
  float q_sm_scale, q_qmax;
  const unsigned short* q_dot_vec;
  // packed batch with an LSE: lse is [Hq, total_q] (FA2's varlen softmax_lse), lse_hs = total_q; q_dot_vec is then ONE
  // [Hkv, D] set shared by all sequences.  Unused by the dense path ([B,Hq,Sq]).
  int64_t lse_hs;
};

// attention backward (attn_bwd.hip); strides in elements {batch, head, seq}, last dim contiguous, D in {64, 128}
struct BwdParams {
  const unsigned short *q, *k, *v, *o, *dout;  // fp16 / bf16 inputs
  unsigned short *dq, *dk, *dv;                // gradients, same dtype
  const int8_t *q8, *k8;                       // forward's codes (quantised operators) or null
  const float *q_scale, *k_scale;              // [B,Hq,nQ] / [B,Hkv,nK] contiguous
  const float* lse;    // [B,Hq,Sq] natural-log LSE as the forward returned it
  const float* dlse;   // [B,Hq,Sq] or null
  const unsigned short* km;  // smooth-K mean in the dtype, [B,Hkv,D] (packed batch: [Hkv,D]), or null
  float *lse2, *delta; // [B,Hq,Sq] workspace: base-2 LSE without the correction, rowsum(dO o O) - dLSE
  int64_t qb, qh, qs, kb, kh, ks, vb, vh, vs, ob, oh, os, db, dh, ds;
  int64_t dqb, dqh, dqs, dkb, dkh, dks, dvb, dvh, dvs, q8b, q8h, q8s, k8b, k8h, k8s;
  int B, Hq, Hkv, Sq, Sk, D, nQ, nK, group;
  float sm_scale;    // natural-log softmax scale: dQ = sm_scale dS K, dK = sm_scale dS^T Q
  float qk_scale;    // un-quantised scores: sm_scale * log2(e)
  float corr_scale;  // sm_scale (multiplies the correction q . km)
  // packed batch (lbfa_backward_varlen) when cu_q != null: strides {0, head, token}, Sq / Sk the maxima, lse / dlse /
  // lse2 / delta [Hq, total_q], q8 / k8 [total, H, D], scales [B, H, max_blocks]
  const int *cu_q, *cu_k;
  int total_q, total_k;
};

// int8 KV cache (kvcache.hip): cache tensors are contiguous, [B, Hkv, cap, D] codes / fp16 V, [B, Hkv, cap / 64] scales,
// [B, Hkv, 64, D] raw rows of the open block, [B, Hkv, D] km; the new rows come through strides {batch, head, seq}
struct AppendParams {
  const unsigned short* k_new;
  const unsigned short* v_new;
  const int* new_lens;          // [B] or null (every sequence appends T rows)
  const unsigned short* km;     // storage dtype or null
  int8_t* k_codes;
  float* k_scale;
  unsigned short* v;
  unsigned short* k_tail;
  const int* seqlens;           // [B], read on the device, not advanced
  int64_t kb, kh, ks, vb, vh, vs;
  int B, Hkv, T, cap;
  float qmax;
};
struct RaggedMeanParams {
  const unsigned short* k_new;
  const int* new_lens;
  unsigned short* km;
  int64_t kb, kh, ks;
  int Hkv, T;
};

// decode attention over the cache (attn_decode.hip): M = Sq * group query rows per (batch, kv head), row r = query head
// hk * group + r / Sq, position r % Sq
struct DecodeParams {
  const unsigned short* q;
  const int8_t* k_codes;
  const float* k_scale;
  const unsigned short* v;
  const unsigned short* km;  // null: no LSE correction
  const int* seqlens;
  void* o;
  float* lse;                // [B, Hq, Sq] natural log, or null
  float* ws_acc;             // [B, Hkv, splits, M, D] un-normalised partial O (splits > 1)
  float* ws_ml;              // [B, Hkv, splits, M, 4]: m, l, dtype(q . km), unused
  int64_t qb, qh, qs, ob, oh, os;
  int B, Hq, Hkv, Sq, group, M, cap, max_k, splits, causal;
  float q_sm_scale, q_qmax, corr_scale;
};

// Paged cache: a pool of pages [num_pages, Hkv, page_size, D] behind one block table per sequence slot.  Key j of slot s lives in
// page block_table[s * max_pages + j / page_size], row j % page_size.  Row b of a call addresses slot slots[b] (null: slot b).
// The fields extend the contiguous structs; only the paged instances of the kernels (attn_decode.hip, kvcache.hip) see them.
struct PoolParams {
  const int* block_table;  // [num_slots, max_pages]
  const int* slots;        // [B] or null
  int num_slots, num_pages, page_size, max_pages;
};
struct PagedDecodeParams : DecodeParams, PoolParams {};
struct PagedAppendParams : AppendParams, PoolParams {};  // cap = max_pages * page_size

// cached prefill (attn_prefill.hip): the decode call for any Sq, plus ragged query lengths; nQ = ceil(Sq / 128) Q blocks per
// (batch, query head), `splits` key slices of the tiles each Q block can see.  The partials are the decode kernel's (same M, same
// rows), so launch_attn_decode_combine takes these structs as the DecodeParams they extend.
struct PrefillParams : DecodeParams {
  const int* q_lens;  // [B] or null (every sequence owns all Sq rows)
  int nQ;
};
struct PagedPrefillParams : PagedDecodeParams {
  const int* q_lens;
  int nQ;
};


// The fp8 V cache (v_bits = 8): `v` of the block points at e4m3fn codes, one byte per element in the layout of the fp16 V, and
// v_scale holds one fp32 per key and kv head - [B, Hkv, cap], paged [num_pages, Hkv, page_size] - found from the same tile number
// as the codes.  The parameter block of an fp8-V instance is its fp16 sibling's with the scales behind it (float* for the append,
// const float* for the readers); only the *_v8_kernel instances see the field.
template <class Base, class ScalePtr>
struct V8Params : Base {
  ScalePtr v_scale;
};

// The nibble-packed K cache (k_packed): `k_codes` of the block points at two codes per byte, rows of D / 2 bytes in the layout of
// the byte-per-code cache - byte j of a row holds channel 2 j in bits 0..3 and channel 2 j + 1 in bits 4..7, each the two's
// complement 4-bit value of the code (qmax 7: never -8).  A 64-key tile is 32 D contiguous bytes.  Scales, tail, km and V are the
// byte cache's.  The parameter block of a packed-K instance is its sibling's - fp16 or fp8 V - with nothing added: the type alone
// selects the *_k4_kernel / *_k4_v8_kernel instances.
template <class Base>
struct K4Params : Base {};

// What a parameter block of the cache kernels selects, written once: the family it belongs to, whether its keys lie in pages and
// the bits of a cached V element and of a cached K code.  The launchers pick the kernel instance from it and the C-ABI layer what to fill in.  Only the
// blocks listed here have one: anything else - a base of one of them included - does not compile.
enum class CacheOp { kAppend, kDecode, kPrefill };
template <CacheOp OP, bool PAGED>
struct CacheBlockOf {
  static constexpr CacheOp op = OP;
  static constexpr bool paged = PAGED;
  static constexpr int v_bits = 16;
  static constexpr int k_bits = 8;
};
template <class P> struct CacheBlock;
template <> struct CacheBlock<AppendParams> : CacheBlockOf<CacheOp::kAppend, false> {};
template <> struct CacheBlock<PagedAppendParams> : CacheBlockOf<CacheOp::kAppend, true> {};
template <> struct CacheBlock<DecodeParams> : CacheBlockOf<CacheOp::kDecode, false> {};
template <> struct CacheBlock<PagedDecodeParams> : CacheBlockOf<CacheOp::kDecode, true> {};
template <> struct CacheBlock<PrefillParams> : CacheBlockOf<CacheOp::kPrefill, false> {};
template <> struct CacheBlock<PagedPrefillParams> : CacheBlockOf<CacheOp::kPrefill, true> {};
template <class Base, class ScalePtr>
struct CacheBlock<V8Params<Base, ScalePtr>> : CacheBlock<Base> {
  static constexpr int v_bits = 8;
};
template <class Base>
struct CacheBlock<K4Params<Base>> : CacheBlock<Base> {
  static constexpr int k_bits = 4;
};

// The launchers of the three families: one host template each, defined and explicitly instantiated for its eight blocks (contiguous
// or paged, fp16 or fp8 V, byte or packed K) in kvcache.hip / attn_decode.hip / attn_prefill.hip; the packed-K instances are a
// second compilation of the same file (LBFA_K4_UNIT), so that the two halves build side by side.  P is deduced exactly, never converted to a base,
// and a block without an instantiation does not link.
template <class P> hipError_t launch_append(const P& p, int dtype, int D, hipStream_t stream);
template <class P> hipError_t launch_decode(const P& p, int dtype, int D, hipStream_t stream);
template <class P> hipError_t launch_prefill(const P& p, int dtype, int D, hipStream_t stream);
hipError_t launch_attn_decode_combine(const DecodeParams& p, int dtype, int D, hipStream_t stream);  // attn_decode.hip
hipError_t launch_kvcache_mean(const RaggedMeanParams& p, int dtype, int B, int D, hipStream_t stream);  // kvcache.hip

}  // namespace lbfa
