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
#include "attn_common.h"
#include "kv_policy.h"

namespace lbfa {

template <class KV, int DT, int D, int MB>
__global__ __launch_bounds__(64) void attn_decode_kernel(typename KV::Params p) {
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D / 8;        // 16-byte chunks of a V tile per lane
  typedef typename KV::tile_t tile_t;
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * VROW];
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x, i16 = lane & 15, g = lane >> 4;
  const KV kv(p, b, hk, D);
  const int n = min(max(p.seqlens[kv.slot], 0), p.max_k);
  const int ntiles = (n + 63) >> 6;
  const int tps = (ntiles + p.splits - 1) / p.splits;
  const int t0 = split * tps, t1 = min(t0 + tps, ntiles);
  const int64_t bh = (int64_t)b * p.Hkv + hk;         // (row of the call, kv head): the partials
  const int64_t sh = (int64_t)kv.slot * p.Hkv + hk;   // (slot, kv head): km

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
          // (the text of elem16 / quant_codes16 of lbfa_common.h, spelled out: the same operations in the same order.  Moving onto
          // the helpers changes the operand order of 16 adds in the compiled kernel and nothing else; it is a step of its own)
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

  const int8_t* kbase = kv.codes + (int64_t)i16 * D + 16 * g;
  const unsigned short* vbase = kv.v;
  const float* ksc = kv.scale;
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
  // The schedule is written in two forms.  Without a table (ContiguousKV) a tile is named by the loop counter.  With one
  // (PagedKV) the tile's name is carried from locate() to the loads and to compute(), and the page id of the tile after the
  // look-ahead tile is fetched one step early.  The first is the second with fetch() = nothing and locate(t) = t, but the
  // compiler schedules that fold differently: measured 5 % slower on one slice of 32K keys at B = 8 (801 -> 845 us), so the
  // plain form stays for the layout that needs no table.  Everything a tile computes is in load_k / load_v / store_v / compute.
  constexpr bool AHEAD = !(MB == 4 && D == 128);
  if constexpr (!KV::kTable) {
    if constexpr (AHEAD) {
      if (t0 < t1) {
        i32x4 ka[4][KS], kb_[4][KS];
        uint4 vr[VCH];
        load_k(t0, ka);
        load_v(t0, vr);
        store_v(t0, vr);
        __syncthreads();
        for (int t = t0; t < t1; t += 2) {
          const int ta = min(t + 1, t1 - 1);
          load_k(ta, kb_);
          load_v(ta, vr);
          compute(t, t, ka);
          __syncthreads();
          if (t + 1 >= t1) break;
          store_v(ta, vr);
          __syncthreads();
          const int tb = min(t + 2, t1 - 1);
          load_k(tb, ka);
          load_v(tb, vr);
          compute(t + 1, t + 1, kb_);
          __syncthreads();
          store_v(tb, vr);
          __syncthreads();
        }
      }
    } else {
      for (int t = t0; t < t1; ++t) {
        i32x4 ka[4][KS];
        uint4 vr[VCH];
        load_k(t, ka);
        load_v(t, vr);
        store_v(t, vr);
        __syncthreads();
        compute(t, t, ka);
        __syncthreads();
      }
    }
  } else {
    if constexpr (AHEAD) {
      if (t0 < t1) {
        i32x4 ka[4][KS], kb_[4][KS];
        uint4 vr[VCH];
        tile_t ga = kv.locate(t0, kv.fetch(t0)), gb;
        int pn = kv.fetch(min(t0 + 1, t1 - 1));  // page id of the NEXT look-ahead tile, on its way one step early
        load_k(ga, ka);
        load_v(ga, vr);
        store_v(t0, vr);
        __syncthreads();
        for (int t = t0; t < t1; t += 2) {
          const int ta = min(t + 1, t1 - 1);
          gb = kv.locate(ta, pn);
          pn = kv.fetch(min(t + 2, t1 - 1));
          load_k(gb, kb_);
          load_v(gb, vr);
          compute(t, ga, ka);
          __syncthreads();
          if (t + 1 >= t1) break;
          store_v(ta, vr);
          __syncthreads();
          const int tb = min(t + 2, t1 - 1);
          ga = kv.locate(tb, pn);
          pn = kv.fetch(min(t + 3, t1 - 1));
          load_k(ga, ka);
          load_v(ga, vr);
          compute(t + 1, gb, kb_);
          __syncthreads();
          store_v(tb, vr);
          __syncthreads();
        }
      }
    } else {
      int pn = t0 < t1 ? kv.fetch(t0) : 0;
      for (int t = t0; t < t1; ++t) {
        i32x4 ka[4][KS];
        uint4 vr[VCH];
        const tile_t ga = kv.locate(t, pn);
        pn = kv.fetch(min(t + 1, t1 - 1));
        load_k(ga, ka);
        load_v(ga, vr);
        store_v(t, vr);
        __syncthreads();
        compute(t, ga, ka);
        __syncthreads();
      }
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

// ---- host-side launchers (called from lbfa_api.hip) ----------------------------------------------------------------------
template <class KV>
static hipError_t launch_decode(const typename KV::Params& p, int dtype, int D, hipStream_t stream) {
  dim3 grid(p.splits, p.Hkv, p.B);
  const int mb = (p.M + 15) / 16;
#define LBFA_DEC(DT, DD, MB) hipLaunchKernelGGL((attn_decode_kernel<KV, DT, DD, MB>), grid, dim3(64), 0, stream, p)
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
hipError_t launch_attn_decode(const DecodeParams& p, int dtype, int D, hipStream_t stream) {
  return launch_decode<ContiguousKV>(p, dtype, D, stream);
}
hipError_t launch_attn_paged_decode(const PagedDecodeParams& p, int dtype, int D, hipStream_t stream) {
  return launch_decode<PagedKV>(p, dtype, D, stream);
}

}  // namespace lbfa
