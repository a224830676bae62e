// Body of attn_prefill_kernel / attn_prefill_v8_kernel (attn_prefill.hip), included as text inside each with the kernel's template parameters, its parameter
// block `p`, `constexpr int VB` (bits of a cached V element: 16 or 8) and `constexpr int KB` (bits of a cached K code: 8, or 4 for the
// nibble-packed cache) in scope.  See attn_prefill.hip.
  constexpr int MB = 2;             // 16-row blocks per wave
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D * VB / 512;  // 16-byte chunks of a V tile per thread
  typedef VStage<VCH, VB == 8 ? VCH : 0> vstage_t;  // fp8 V: and the scale of each chunk's key
  typedef std::conditional_t<KB == 4, u32x2, i32x4> kfrag_t;  // a lane's 16 codes of one key as they are loaded
  typedef typename KV::tile_t tile_t;
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * VROW];
  __shared__ float wamax[4];
  const int qblk = blockIdx.x / p.splits, split = blockIdx.x - qblk * p.splits;
  const int h = blockIdx.y, b = blockIdx.z, hk = h / p.group;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, g = lane >> 4;
  const KV kv(p, b, hk, D);
  const int n = min(max(p.seqlens[kv.slot], 0), p.max_k);
  const int ql = p.q_lens != nullptr ? min(max(p.q_lens[b], 0), p.Sq) : p.Sq;
  // tiles this Q block can see: below the limit of its last valid row (none: the block lies past the sequence's queries)
  const int last = min(qblk * 128 + 127, ql - 1);
  const int see = last < qblk * 128 ? 0 : (p.causal ? max(n - ql + 1 + last, 0) : n);
  const int ntiles = (see + 63) >> 6;
  const int tps = (ntiles + p.splits - 1) / p.splits;
  const int t0 = split * tps, t1 = min(t0 + tps, ntiles);
  const int64_t sh = (int64_t)kv.slot * p.Hkv + hk;  // (slot, kv head): km

  // ---- query rows of this lane: load, quantise with the block's scale, q . km ------------------------------------------
  int row[MB], lim[MB];
  i32x4 qf[MB][KS];
  float corr[MB];
  float qsc;
  {
    float xq[MB][KS][16];
    float amax = 0.f;
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      row[rb] = qblk * 128 + wave * 32 + 16 * rb + i16;
      const bool valid = row[rb] < ql;
      lim[rb] = valid ? (p.causal ? n - ql + 1 + row[rb] : n) : 0;
      float dot = 0.f;
      const unsigned short* qp = p.q + (int64_t)b * p.qb + (int64_t)h * p.qh + (int64_t)(valid ? row[rb] : 0) * p.qs + 16 * g;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        uint4 raw[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (valid) {
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
            dot += v * elem16<DT>(kmr[hf], e);
            const float x = v * p.q_sm_scale;
            xq[rb][s][hf * 8 + e] = x;
            amax = fmaxf(amax, fabsf(x));
          }
      }
      dot += __shfl_xor(dot, 16, 64);
      dot += __shfl_xor(dot, 32, 64);
      corr[rb] = load_cvt<DT>(store_cvt<DT>(dot));  // the correction is a storage-dtype matmul (src/core.py:294-304)
    }
    amax = wave_max(amax);
    if (lane == 0) wamax[wave] = amax;
    __syncthreads();
    qsc = block_scale(amax_collect(wamax), p.q_qmax);
#pragma unroll
    for (int rb = 0; rb < MB; ++rb)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        qf[rb][s] = quant_codes16<false>(xq[rb][s], qsc, 0.f);  // the plain division
        if constexpr (KB == 4) qf[rb][s] = k4_q_order(qf[rb][s]);
      }
  }
  // the compare against the row limits is needed only in tiles that reach past the smallest limit of this wave's rows
  const int lim_min = wave_min_i32(min(lim[0], lim[1]));

  // ---- the tile: running state, bases, load_k / load_v / store_v / compute, shared with the decode body --------------------------
  constexpr int NT = 256;  // a V tile belongs to the four waves
  const int tix = tid;
  auto q_scale = [&](int) __attribute__((always_inline)) { return qsc; };  // one block of 128 rows: the workgroup's
#include "attn_cache_tile.inc"
  // wave-uniform: a tile wholly below every limit of the wave's rows takes the form without the compare (same bits)
  auto tile = [&](int t, tile_t gt, const kfrag_t (&kf)[4][KS]) __attribute__((always_inline)) {
    if (t * 64 + 64 <= lim_min) compute(t, gt, kf, std::false_type{});
    else compute(t, gt, kf, std::true_type{});
  };

  // ---- tile loop: K of tile t + 1 lands in the other register set, V of tile t + 1 in registers, while tile t is computed.
  // The look-ahead index is clamped to the slice (the last tile is requested twice, from cache) so no load sits in a branch; the
  // page id of the tile after the look-ahead tile is fetched one step early (ContiguousKV: fetch() is nothing, locate(t) = t).
  // All four waves take every barrier: t0, t1 depend on the workgroup only.
  if (t0 < t1) {
    kfrag_t ka[4][KS], kb_[4][KS];
    vstage_t vr;
    tile_t ga = kv.locate(t0, kv.fetch(t0)), gb;
    int pn = kv.fetch(min(t0 + 1, t1 - 1));
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
      tile(t, ga, ka);
      __syncthreads();
      if (t + 1 >= t1) break;
      store_v(ta, vr);
      __syncthreads();
      const int tb = min(t + 2, t1 - 1);
      ga = kv.locate(tb, pn);
      pn = kv.fetch(min(t + 3, t1 - 1));
      load_k(ga, ka);
      load_v(ga, vr);
      tile(t + 1, gb, kb_);
      __syncthreads();
      store_v(tb, vr);
      __syncthreads();
    }
  }

  // ---- epilogue: rows past Sq do not exist; rows in [q_lens[b], Sq) saw no key: zeros, -inf ----------------------------------
  if (p.splits == 1) {
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (row[rb] >= p.Sq) continue;
      const float l = l_run[rb];
      const float inv = l > 0.f ? 1.0f / l : 0.f;  // no visible key: zeros, LSE -inf (as the varlen operator)
      unsigned short* op = reinterpret_cast<unsigned short*>(p.o) + (int64_t)b * p.ob + (int64_t)h * p.oh + (int64_t)row[rb] * p.os + 4 * g;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const f32x4 a = acc[rb][cb];
        const unsigned w0 = (unsigned)store_cvt<DT>(a[0] * inv) | ((unsigned)store_cvt<DT>(a[1] * inv) << 16);
        const unsigned w1 = (unsigned)store_cvt<DT>(a[2] * inv) | ((unsigned)store_cvt<DT>(a[3] * inv) << 16);
        *reinterpret_cast<uint2*>(op + 16 * cb) = make_uint2(w0, w1);
      }
      if (p.lse != nullptr && g == 0) {
        const float lse2 = l > 0.f ? __builtin_amdgcn_logf(l) + m_run[rb] : -__builtin_inff();
        p.lse[((int64_t)b * p.Hq + h) * p.Sq + row[rb]] = lse2 / kLog2e + corr[rb] * p.corr_scale;
      }
    }
  } else {
    const int64_t bh = (int64_t)b * p.Hkv + hk;  // (row of the call, kv head): the partials
    const int64_t slot = (bh * p.splits + split) * p.M + (int64_t)(h - hk * p.group) * p.Sq;
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      if (row[rb] >= p.Sq) continue;
      if (t0 < t1) {  // the combine never reads the acc of a slice whose m is -inf
        float* ap = p.ws_acc + (slot + row[rb]) * D + 4 * g;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) *reinterpret_cast<f32x4*>(ap + 16 * cb) = acc[rb][cb];
      }
      if (g == 0) *reinterpret_cast<f32x4*>(p.ws_ml + (slot + row[rb]) * 4) = f32x4{m_run[rb], l_run[rb], corr[rb], 0.f};
    }
  }
