// Split-KV decode attention over the PAGED int8 KV cache, gfx950: attn_decode_kernel (attn_decode.hip - layout of a tile, lane
// roles and arithmetic are described there) with one table look-up per 64-key tile.
//
// Pool: k_codes int8 / v fp16 [num_pages, Hkv, page_size, D], k_scale fp32 [num_pages, Hkv, page_size / 64]; key j of the sequence
// in slot s lives in page block_table[s * max_pages + j / page_size], row j % page_size.  page_size is a multiple of 64, so a
// tile - 64 D bytes of codes, 128 D bytes of V, one scale - is contiguous inside one page and the tile's arithmetic does not know
// that it moved: same products in the same order per slice, the same partials for attn_decode_combine_kernel (whose workspace is
// indexed by row of the call: nothing paged in it), results bit-identical to the contiguous cache for the same number of slices.
// The look-up - slot of the row, page of the tile, both clamped into [0, num_slots) / [0, num_pages) because the host cannot
// check device data - is wave-uniform scalar work.
//
// This is a COPY of attn_decode_kernel's text, not a shared body: with one __device__ body behind a PAGED flag the compiler moved
// instructions of all twelve contiguous instances (an operand swap in the prologue's adds, other register assignments), and
// that kernel has to stay the parent's instruction for instruction.  A change to the arithmetic of one belongs in the other too;
// tests/test_gpu_paged_kvcache.py holds the two to torch.equal.
#include "attn_common.h"

namespace lbfa {

hipError_t launch_attn_decode_combine(const DecodeParams& p, int dtype, int D, hipStream_t stream);  // attn_decode.hip

namespace {
typedef short s16x4v __attribute__((ext_vector_type(4)));
constexpr float kLog2e = 1.44269504f;  // as attn_decode.hip
}  // namespace

template <int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_paged_decode_kernel(PagedDecodeParams p) {
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D / 8;        // 16-byte chunks of a V tile per lane
  typedef int64_t tile_t;           // what names a tile to the loads, see locate()
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * VROW];
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x, i16 = lane & 15, g = lane >> 4;
  // b is the ROW of the call (q, o, lse, workspace); seqlens, km and the block table belong to its slot.  Slot and page ids are
  // device data the host cannot check: both are clamped into range (wave-uniform scalar work), so a corrupt table gives a wrong
  // answer, never an address outside the pool.
  int sl = p.slots != nullptr ? p.slots[b] : b;
  sl = __builtin_amdgcn_readfirstlane(min(max(sl, 0), p.num_slots - 1));
  const int n = min(max(p.seqlens[sl], 0), p.max_k);
  const int ntiles = (n + 63) >> 6;
  const int tps = (ntiles + p.splits - 1) / p.splits;
  const int t0 = split * tps, t1 = min(t0 + tps, ntiles);
  const int64_t bh = (int64_t)b * p.Hkv + hk;
  const int64_t sh = (int64_t)sl * p.Hkv + hk;  // (slot, kv head): km

  // ---- query rows of this lane: load, quantise, q . km ---------------------------------------------------------------
  int row[MB], hq[MB], sq[MB], lim[MB];
  bool valid[MB];
  i32x4 qf[MB][KS];
  float qsc[MB], corr[MB];
  float* srow = reinterpret_cast<float*>(smem);  // per-row max |q * sm_scale|, before the V tiles use the memory
  {
    float xq[MB][KS][16];
    float amax[MB], dot[MB];
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      row[rb] = 16 * rb + i16;
      valid[rb] = row[rb] < p.M;
      const int hl = valid[rb] ? row[rb] / p.Sq : 0;
      sq[rb] = valid[rb] ? row[rb] - hl * p.Sq : 0;
      hq[rb] = hk * p.group + hl;
      lim[rb] = p.causal ? n - p.Sq + 1 + sq[rb] : n;
      amax[rb] = 0.f;
      dot[rb] = 0.f;
      const unsigned short* qp = p.q + (int64_t)b * p.qb + (int64_t)hq[rb] * p.qh + (int64_t)sq[rb] * p.qs + 16 * g;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        uint4 raw[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (valid[rb]) {
          raw[0] = *reinterpret_cast<const uint4*>(qp + 64 * s);
          raw[1] = *reinterpret_cast<const uint4*>(qp + 64 * s + 8);
        }
        uint4 kmr[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (p.km != nullptr) {
          kmr[0] = *reinterpret_cast<const uint4*>(p.km + sh * D + 64 * s + 16 * g);
          kmr[1] = *reinterpret_cast<const uint4*>(p.km + sh * D + 64 * s + 16 * g + 8);
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          // (spelled out, not elem16 / quant_codes16 as in the forward kernels: behind either helper the compiler swaps the operands
          // of an add in this kernel's LSE epilogue, and the kernel has to stay the parent's instruction for instruction)
          const unsigned w[4] = {raw[hf].x, raw[hf].y, raw[hf].z, raw[hf].w};
          const unsigned mw[4] = {kmr[hf].x, kmr[hf].y, kmr[hf].z, kmr[hf].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = load_cvt<DT>((unsigned short)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu)));
            const float mv = load_cvt<DT>((unsigned short)((e & 1) ? (mw[e >> 1] >> 16) : (mw[e >> 1] & 0xffffu)));
            dot[rb] += v * mv;
            const float x = v * p.q_sm_scale;
            xq[rb][s][hf * 8 + e] = x;
            amax[rb] = fmaxf(amax[rb], fabsf(x));
          }
        }
      }
      amax[rb] = fmaxf(amax[rb], __shfl_xor(amax[rb], 16, 64));
      amax[rb] = fmaxf(amax[rb], __shfl_xor(amax[rb], 32, 64));
      dot[rb] += __shfl_xor(dot[rb], 16, 64);
      dot[rb] += __shfl_xor(dot[rb], 32, 64);
      corr[rb] = load_cvt<DT>(store_cvt<DT>(dot[rb]));  // the correction is a storage-dtype matmul (src/core.py:294-304)
      if (g == 0) srow[row[rb]] = amax[rb];
    }
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      float am = 0.f;
      const int r0 = row[rb] - sq[rb];  // first row of this row's query head
      if (valid[rb])
        for (int j = 0; j < p.Sq; ++j) am = fmaxf(am, srow[r0 + j]);
      const float scale = block_scale(am, p.q_qmax);
      qsc[rb] = scale;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        unsigned wd[4];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          int qv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) qv[e] = quant_code<false>(xq[rb][s][4 * g4 + e], scale, 0.f);  // the plain division
          wd[g4] = pack4_i8(qv);
        }
        qf[rb][s] = i32x4{(int)wd[0], (int)wd[1], (int)wd[2], (int)wd[3]};
      }
    }
    __syncthreads();  // srow is dead: the memory becomes the V tile
  }

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

  // Where tile t of the sequence lives: tile `gt` of the POOL seen as [num_pages, Hkv, page_size / 64] tiles of 64 keys - codes, V
  // and scale of a tile are all found from that one 64-bit number, and nothing else in a tile's computation knows where the tile
  // lives.  fetch() is the table load, locate() the arithmetic on its result: the loop fetches the page id of the tile AFTER the
  // look-ahead tile, so that no K / V load waits behind a fresh table load.  All of it depends on blockIdx and the loop counter
  // only: scalar registers, one scalar divide per tile (page_size is any multiple of 64, not only a power of two).
  const int8_t* kbase = p.k_codes + (int64_t)i16 * D + 16 * g;
  const unsigned short* vbase = p.v;
  const float* ksc = p.k_scale;
  const int tpp = p.page_size >> 6;  // tiles per page
  const int* tbl = p.block_table + (int64_t)sl * p.max_pages;
  auto fetch = [&](int t) __attribute__((always_inline)) -> int { return tbl[t / tpp]; };
  auto locate = [&](int t, int pg) __attribute__((always_inline)) -> tile_t {
    pg = __builtin_amdgcn_readfirstlane(min(max(pg, 0), p.num_pages - 1));
    return ((int64_t)pg * p.Hkv + hk) * tpp + t % tpp;
  };
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
    for (int u = 0; u < VCH; ++u) vr[u] = *reinterpret_cast<const uint4*>(vt + (u * 64 + lane) * 8);  // the tile is contiguous
  };
  auto store_v = [&](int t, const uint4 (&vr)[VCH]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < VCH; ++u) {
      const int cidx = u * 64 + lane, r = cidx / (D / 8), ch = cidx % (D / 8);
      // rows past the end may hold anything (0 * NaN): they enter the product as zeros
      const uint4 val = (t * 64 + r < n) ? vr[u] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(smem + r * VROW + ch * 16) = val;
    }
  };
  auto compute = [&](int t, tile_t gt, const i32x4 (&kf)[4][KS]) __attribute__((always_inline)) {
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
          const int key = t * 64 + kb * 16 + 4 * g + r;
          float s2 = (float)sacc[r] * qsc[rb] * kscale;
          s2 = key < lim[rb] ? s2 : -__builtin_inff();
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

  // ---- tile loop: K of tile t + 1 lands in the other register set, V of tile t + 1 in registers, while tile t is computed.
  // The look-ahead index is clamped to the slice (the last tile is requested twice, from cache) so no load sits in a branch.
  // 64 rows at D = 128 hold 128 accumulator registers: no room for a second tile, that instance loads and computes in turn.
  constexpr bool AHEAD = !(MB == 4 && D == 128);
  if constexpr (AHEAD) {
    if (t0 < t1) {
      i32x4 ka[4][KS], kb_[4][KS];
      uint4 vr[VCH];
      tile_t ga = locate(t0, fetch(t0)), gb;
      int pn = fetch(min(t0 + 1, t1 - 1));  // page id of the NEXT look-ahead tile, on its way one step early
      load_k(ga, ka);
      load_v(ga, vr);
      store_v(t0, vr);
      __syncthreads();
      for (int t = t0; t < t1; t += 2) {
        const int ta = min(t + 1, t1 - 1);
        gb = locate(ta, pn);
        pn = fetch(min(t + 2, t1 - 1));
        load_k(gb, kb_);
        load_v(gb, vr);
        compute(t, ga, ka);
        __syncthreads();
        if (t + 1 >= t1) break;
        store_v(ta, vr);
        __syncthreads();
        const int tb = min(t + 2, t1 - 1);
        ga = locate(tb, pn);
        pn = fetch(min(t + 3, t1 - 1));
        load_k(ga, ka);
        load_v(ga, vr);
        compute(t + 1, gb, kb_);
        __syncthreads();
        store_v(tb, vr);
        __syncthreads();
      }
    }
  } else {
    int pn = t0 < t1 ? fetch(t0) : 0;
    for (int t = t0; t < t1; ++t) {
      i32x4 ka[4][KS];
      uint4 vr[VCH];
      const tile_t ga = locate(t, pn);
      pn = fetch(min(t + 1, t1 - 1));
      load_k(ga, ka);
      load_v(ga, vr);
      store_v(t, vr);
      __syncthreads();
      compute(t, ga, ka);
      __syncthreads();
    }
  }

  // ---- epilogue ----------------------------------------------------------------------------------------------------------
  if (p.splits == 1) {
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (!valid[rb]) continue;
      const float l = l_run[rb];
      const float inv = l > 0.f ? 1.0f / l : 0.f;  // no visible key: zeros, LSE -inf (as the varlen operator)
      unsigned short* op = reinterpret_cast<unsigned short*>(p.o) + (int64_t)b * p.ob + (int64_t)hq[rb] * p.oh + (int64_t)sq[rb] * p.os + 4 * g;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const f32x4 a = acc[rb][cb];
        const unsigned w0 = (unsigned)store_cvt<DT>(a[0] * inv) | ((unsigned)store_cvt<DT>(a[1] * inv) << 16);
        const unsigned w1 = (unsigned)store_cvt<DT>(a[2] * inv) | ((unsigned)store_cvt<DT>(a[3] * inv) << 16);
        *reinterpret_cast<uint2*>(op + 16 * cb) = make_uint2(w0, w1);
      }
      if (p.lse != nullptr && g == 0) {
        const float lse2 = l > 0.f ? __builtin_amdgcn_logf(l) + m_run[rb] : -__builtin_inff();
        p.lse[((int64_t)b * p.Hq + hq[rb]) * p.Sq + sq[rb]] = lse2 / kLog2e + corr[rb] * p.corr_scale;
      }
    }
  } else {
    const int64_t slot = (bh * p.splits + split) * p.M;
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (!valid[rb]) continue;
      float* ap = p.ws_acc + (slot + row[rb]) * D + 4 * g;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) *reinterpret_cast<f32x4*>(ap + 16 * cb) = acc[rb][cb];
      if (g == 0) *reinterpret_cast<f32x4*>(p.ws_ml + (slot + row[rb]) * 4) = f32x4{m_run[rb], l_run[rb], corr[rb], 0.f};
    }
  }
}

// ---- host-side launcher (called from lbfa_api.hip) -----------------------------------------------------------------------
hipError_t launch_attn_paged_decode(const PagedDecodeParams& p, int dtype, int D, hipStream_t stream) {
  dim3 grid(p.splits, p.Hkv, p.B);
  const int mb = (p.M + 15) / 16;
#define LBFA_DEC(DT, DD, MB) hipLaunchKernelGGL((attn_paged_decode_kernel<DT, DD, MB>), grid, dim3(64), 0, stream, p)
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

}  // namespace lbfa
