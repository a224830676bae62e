// Body of attn_decode_kernel / attn_decode_v8_kernel (attn_decode.hip), included as text inside each with the kernel's template parameters, its parameter
// block `p` and `constexpr int VB` (bits of a cached V element: 16 or 8) in scope.  See attn_decode.hip.
  constexpr int KS = D / 64;        // k-steps of the score product
  constexpr int CB = D / 16;        // 16-channel blocks of O^T
  constexpr int VROW = 2 * D + 32;  // bytes per LDS row
  constexpr int VCH = D * VB / 128;  // 16-byte chunks of a V tile per lane
  typedef VStage<VCH, VB == 8 ? VCH : 0> vstage_t;  // fp8 V: and the scale of each chunk's key
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
  const uint8_t* v8base = nullptr;  // fp8 V: the codes and the scales of (b, hk), or of the pool
  const float* vsbase = nullptr;
  if constexpr (VB == 8) {
    const int64_t key0 = KV::key0(p, b, hk);
    v8base = reinterpret_cast<const uint8_t*>(p.v) + key0 * D;
    vsbase = p.v_scale + key0;
  }
  auto load_v = [&](tile_t t, vstage_t& vr) __attribute__((always_inline)) {
    if constexpr (VB == 8) {
      const uint8_t* vt = v8base + (int64_t)t * 64 * D;
#pragma unroll
      for (int u = 0; u < VCH; ++u) load_v8_chunk<D>(vt, vsbase + (int64_t)t * 64, u * 64 + lane, vr.c[u], vr.s[u]);
    } else {
      const unsigned short* vt = vbase + (int64_t)t * 64 * D;
#pragma unroll
      for (int u = 0; u < VCH; ++u) vr.c[u] = *reinterpret_cast<const uint4*>(vt + (u * 64 + lane) * 8);  // the tile is contiguous
    }
  };
  auto store_v = [&](int t, const vstage_t& vr) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < VCH; ++u) {
      if constexpr (VB == 8) {
        store_vhat_chunk<D, VROW>(smem, u * 64 + lane, vr.c[u], vr.s[u], n - t * 64);
      } else {
        const int cidx = u * 64 + lane, r = cidx / (D / 8), ch = cidx % (D / 8);
        // rows past the end may hold anything (0 * NaN): they enter the product as zeros
        const uint4 val = (t * 64 + r < n) ? vr.c[u] : make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(smem + r * VROW + ch * 16) = val;
      }
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
        vstage_t vr;
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
        vstage_t vr;
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
        vstage_t vr;
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
