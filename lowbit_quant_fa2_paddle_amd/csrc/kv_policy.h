// Where a 64-key tile of the int8 KV cache lives: the policies the kernels that read the cache (attn_decode.hip,
// attn_prefill.hip) are instantiated with - one kernel body each for the contiguous cache and for the paged one.
#pragma once
#include "attn_common.h"

namespace lbfa {

typedef short s16x4v __attribute__((ext_vector_type(4)));
constexpr float kLog2e = 1.44269504f;  // the literal of src/core.py:347; the natural-log LSE is a correctly rounded division by it

// Contiguous cache: k_codes int8 / v fp16 [B, Hkv, cap, D], k_scale fp32 [B, Hkv, cap / 64].  Tile t of (b, hk) is tile t behind
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
  __device__ __forceinline__ int fetch(int t) const { return tbl[t / tpp]; }
  __device__ __forceinline__ tile_t locate(int t, int pg) const {
    pg = __builtin_amdgcn_readfirstlane(min(max(pg, 0), num_pages - 1));
    return ((int64_t)pg * Hkv + hk) * tpp + t % tpp;
  }
};

}  // namespace lbfa
