// Where a 64-key tile of the int8 KV cache lives: the policies the kernels that read the cache (attn_decode.hip,
// attn_prefill.hip) are instantiated with - one kernel body each for the contiguous cache and for the paged one, and one text of
// what both do with a tile (attn_cache_tile.inc).
#pragma once
#include "attn_common.h"

namespace lbfa {

typedef short s16x4v __attribute__((ext_vector_type(4)));
constexpr float kLog2e = 1.44269504f;  // the literal of src/core.py:347; the natural-log LSE is a correctly rounded division by it

// Contiguous cache: k_codes int8 / v fp16 (fp8 V cache: e4m3 codes, see below) [B, Hkv, cap, D], k_scale fp32 [B, Hkv, cap / 64].  Tile t of (b, hk) is tile t behind
// the bases of that (b, hk); seqlens and km are indexed by the row of the call.
struct ContiguousKV {
  typedef DecodeParams Params;
  typedef int tile_t;  // what names a tile to the loads, see locate()
  static constexpr bool kTable = false;
  int slot;
  const int8_t* codes;
  const unsigned short* v;
  const float* scale;
  __device__ __forceinline__ ContiguousKV(const Params& p, int b, int hk, int D) {
    const int64_t bh = (int64_t)b * p.Hkv + hk;
    slot = b;
    codes = p.k_codes + bh * (int64_t)p.cap * D;
    v = p.v + bh * (int64_t)p.cap * D;
    scale = p.k_scale + bh * (p.cap >> 6);
  }
  // first key of (b, hk) in an array with one entry per key: the codes and the scales of the fp8 V cache
  static __device__ __forceinline__ int64_t key0(const Params& p, int b, int hk) { return ((int64_t)b * p.Hkv + hk) * (int64_t)p.cap; }
  __device__ __forceinline__ int fetch(int) const { return 0; }
  __device__ __forceinline__ tile_t locate(int t, int) const { return t; }
};

// Paged cache: a pool k_codes int8 / v fp16 [num_pages, Hkv, page_size, D], k_scale fp32 [num_pages, Hkv, page_size / 64]; key j of
// the sequence in slot s lives in page block_table[s * max_pages + j / page_size], row j % page_size.  page_size is a multiple of
// 64, so a tile - 64 D bytes of codes, 128 D bytes of V, one scale - is contiguous inside one page.  Tile t of the sequence is
// tile `gt` of the POOL seen as [num_pages, Hkv, page_size / 64] tiles of 64 keys: codes, V and scale of a tile are all found from
// that one 64-bit number.  b is the ROW of the call (q, o, lse, workspace); seqlens, km and the block table belong to its slot.
// Slot and page ids are device data the host cannot check: both are clamped into [0, num_slots) / [0, num_pages) (wave-uniform
// scalar work), so a corrupt table gives a wrong answer, never an address outside the pool.  fetch() is the table load,
// locate() the arithmetic on its result: the loop fetches the page id of the tile AFTER the look-ahead tile, so that no K / V
// load waits behind a fresh table load.  All of it depends on blockIdx and the loop counter only: scalar registers, one scalar
// divide per tile (page_size is any multiple of 64, not only a power of two).
struct PagedKV {
  typedef PagedDecodeParams Params;
  typedef int64_t tile_t;
  static constexpr bool kTable = true;
  int slot;
  const int8_t* codes;
  const unsigned short* v;
  const float* scale;
  const int* tbl;
  int tpp, hk, Hkv, num_pages;  // tpp: tiles per page
  __device__ __forceinline__ PagedKV(const Params& p, int b, int hk_, int) {
    const int sl = p.slots != nullptr ? p.slots[b] : b;
    slot = __builtin_amdgcn_readfirstlane(min(max(sl, 0), p.num_slots - 1));
    codes = p.k_codes;
    v = p.v;
    scale = p.k_scale;
    tbl = p.block_table + (int64_t)slot * p.max_pages;
    tpp = p.page_size >> 6;
    hk = hk_;
    Hkv = p.Hkv;
    num_pages = p.num_pages;
  }
  static __device__ __forceinline__ int64_t key0(const Params&, int, int) { return 0; }  // tiles are numbered in the pool
  __device__ __forceinline__ int fetch(int t) const { return tbl[t / tpp]; }
  __device__ __forceinline__ tile_t locate(int t, int pg) const {
    pg = __builtin_amdgcn_readfirstlane(min(max(pg, 0), num_pages - 1));
    return ((int64_t)pg * Hkv + hk) * tpp + t % tpp;
  }
};


// ---- the fp8 V cache (v_bits = 8): V as e4m3fn codes [.., key, D] with ONE fp32 scale per key and kv head, written by the
// append kernel (kvcache.hip) and never re-quantised.  What a reader sees is V^ = fp16_rne(fp32(decode(code)) * scale): one fp32
// multiply and one round-to-nearest-even conversion per element, fp16 subnormals kept.  The readers turn a tile into V^ on its
// way into the LDS image the fp16 V tile has; everything behind the image is the fp16 code.
// What a thread keeps of the V tile that is on its way: NC 16-byte chunks and - fp8 V - NS scales
template <int NC, int NS>
struct VStage {
  uint4 c[NC];
  float s[NS];
};
template <int NC>
struct VStage<NC, 0> {
  uint4 c[NC];
};
// 16 codes of one key (a 16-byte chunk) -> their 16 V^ as two 16-byte chunks of fp16
__device__ __forceinline__ void e4m3x16_to_vhat(const uint4& codes, float scale, uint4& lo, uint4& hi) {
  const unsigned w[4] = {codes.x, codes.y, codes.z, codes.w};
  unsigned o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    const f16x2 pa = f16x2{(_Float16)(a[0] * scale), (_Float16)(a[1] * scale)};
    const f16x2 pb = f16x2{(_Float16)(b[0] * scale), (_Float16)(b[1] * scale)};
    o[2 * i] = __builtin_bit_cast(unsigned, pa);
    o[2 * i + 1] = __builtin_bit_cast(unsigned, pb);
  }
  lo = make_uint4(o[0], o[1], o[2], o[3]);
  hi = make_uint4(o[4], o[5], o[6], o[7]);
}

// A tile of the fp8 V cache is 64 D contiguous code bytes and 64 contiguous scales; chunk `cidx` of it is 16 channels of key
// cidx / (D / 16).  The two steps of a reader, called by load_v / store_v of attn_cache_tile.inc (thread tix of the NT that share the tile
// takes chunks u * NT + tix):
// fetch a chunk with the scale of its key ...
template <int D>
__device__ __forceinline__ void load_v8_chunk(const uint8_t* tile, const float* scales, int cidx, uint4& codes, float& scale) {
  codes = *reinterpret_cast<const uint4*>(tile + cidx * 16);
  scale = scales[cidx / (D / 16)];
}
// ... and write its V^ as the two 16-byte chunks the fp16 tile has at that place of the [64][VROW] LDS image.  Keys at or past
// `valid_keys` may hold any code and any scale (NaN): they enter the product as zeros.
template <int D, int VROW>
__device__ __forceinline__ void store_vhat_chunk(unsigned char* image, int cidx, const uint4& codes, float scale, int valid_keys) {
  const int r = cidx / (D / 16), ch = cidx % (D / 16);
  uint4 lo, hi;
  e4m3x16_to_vhat(codes, scale, lo, hi);
  const bool in = r < valid_keys;
  *reinterpret_cast<uint4*>(image + r * VROW + ch * 32) = in ? lo : make_uint4(0, 0, 0, 0);
  *reinterpret_cast<uint4*>(image + r * VROW + ch * 32 + 16) = in ? hi : make_uint4(0, 0, 0, 0);
}


// ---- the nibble-packed K cache (K4Params, lbfa_common.h): what a reader does with the packed words -----------------------------
// The 8 bytes a lane fetches for one key hold its 16 channels c .. c + 15 as two words; the low nibbles of word 0 are channels
// c + {0, 2, 4, 6}, its high nibbles c + {1, 3, 5, 7}, word 1 the same 8 channels on.  k4_widen turns them into the int8 operand of
// the score MFMA in THAT channel order - {even of word 0, odd of word 0, even of word 1, odd of word 1} - as 16 * code: a nibble in
// the top half of a byte IS 16 * code as int8 (|16 * code| <= 112), one shift and two masks per word and no sign extension.  An
// integer dot product does not care in which order its channels are added, so Q's 16 codes per lane are put into the same order
// once (k4_q_order), and the int32 score, 16 * (q . k) exactly, is shifted right by 4: the bits of the byte cache's score.
__device__ __forceinline__ i32x4 k4_widen(u32x2 w) {
  return i32x4{(int)((w.x << 4) & 0xF0F0F0F0u), (int)(w.x & 0xF0F0F0F0u), (int)((w.y << 4) & 0xF0F0F0F0u), (int)(w.y & 0xF0F0F0F0u)};
}
__device__ __forceinline__ i32x4 k4_q_order(i32x4 q) {
  return i32x4{(int)__builtin_amdgcn_perm((unsigned)q[1], (unsigned)q[0], 0x06040200u),
               (int)__builtin_amdgcn_perm((unsigned)q[1], (unsigned)q[0], 0x07050301u),
               (int)__builtin_amdgcn_perm((unsigned)q[3], (unsigned)q[2], 0x06040200u),
               (int)__builtin_amdgcn_perm((unsigned)q[3], (unsigned)q[2], 0x07050301u)};
}

}  // namespace lbfa
