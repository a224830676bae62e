// Body of attn_decode_kernel / attn_decode_v8_kernel (attn_decode.hip), included as text inside each with the kernel's template parameters, its parameter
// block `p`, `constexpr int VB` (bits of a cached V element: 16 or 8) and `constexpr int KB` (bits of a cached K code: 8, or 4 for the
// nibble-packed cache) in scope.  See attn_decode.hip.
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D * VB / 128;  // 16-byte chunks of a V tile per lane
  typedef VStage<VCH, VB == 8 ? VCH : 0> vstage_t;  // fp8 V: and the scale of each chunk's key
  typedef std::conditional_t<KB == 4, u32x2, i32x4> kfrag_t;  // a lane's 16 codes of one key as they are loaded
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
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = elem16<DT>(raw[hf], e);
            dot[rb] += v * elem16<DT>(kmr[hf], e);
            const float x = v * p.q_sm_scale;
            xq[rb][s][hf * 8 + e] = x;
            amax[rb] = fmaxf(amax[rb], fabsf(x));
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
        qf[rb][s] = quant_codes16<false>(xq[rb][s], scale, 0.f);  // the plain division
        if constexpr (KB == 4) qf[rb][s] = k4_q_order(qf[rb][s]);
      }
    }
    __syncthreads();  // srow is dead: the memory becomes the V tile
  }

  // ---- the tile: running state, bases, load_k / load_v / store_v / compute, shared with the prefill body -------------------------
  constexpr int NT = 64;  // a V tile belongs to the wave
  const int tix = lane;
  auto q_scale = [&](int rb) __attribute__((always_inline)) { return qsc[rb]; };  // one block of Sq rows per query head
#include "attn_cache_tile.inc"

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
        kfrag_t ka[4][KS], kb_[4][KS];
        vstage_t vr;
        load_k(t0, ka);
        load_v(t0, vr);
        store_v(t0, vr);
        __syncthreads();
        for (int t = t0; t < t1; t += 2) {
          const int ta = min(t + 1, t1 - 1);
          load_k(ta, kb_);
          load_v(ta, vr);
          compute(t, t, ka, std::true_type{});
          __syncthreads();
          if (t + 1 >= t1) break;
          store_v(ta, vr);
          __syncthreads();
          const int tb = min(t + 2, t1 - 1);
          load_k(tb, ka);
          load_v(tb, vr);
          compute(t + 1, t + 1, kb_, std::true_type{});
          __syncthreads();
          store_v(tb, vr);
          __syncthreads();
        }
      }
    } else {
      for (int t = t0; t < t1; ++t) {
        kfrag_t ka[4][KS];
        vstage_t vr;
        load_k(t, ka);
        load_v(t, vr);
        store_v(t, vr);
        __syncthreads();
        compute(t, t, ka, std::true_type{});
        __syncthreads();
      }
    }
  } else {
    if constexpr (AHEAD) {
      if (t0 < t1) {
        kfrag_t ka[4][KS], kb_[4][KS];
        vstage_t vr;
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
          compute(t, ga, ka, std::true_type{});
          __syncthreads();
          if (t + 1 >= t1) break;
          store_v(ta, vr);
          __syncthreads();
          const int tb = min(t + 2, t1 - 1);
          ga = kv.locate(tb, pn);
          pn = kv.fetch(min(t + 3, t1 - 1));
          load_k(ga, ka);
          load_v(ga, vr);
          compute(t + 1, gb, kb_, std::true_type{});
          __syncthreads();
          store_v(tb, vr);
          __syncthreads();
        }
      }
    } else {
      int pn = t0 < t1 ? kv.fetch(t0) : 0;
      for (int t = t0; t < t1; ++t) {
        kfrag_t ka[4][KS];
        vstage_t vr;
        const tile_t ga = kv.locate(t, pn);
        pn = kv.fetch(min(t + 1, t1 - 1));
        load_k(ga, ka);
        load_v(ga, vr);
        store_v(t, vr);
        __syncthreads();
        compute(t, ga, ka, std::true_type{});
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
