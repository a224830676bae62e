// What a reader of the KV cache does with one 64-key tile, written once: the running state of the online softmax, the bases of a
// tile, and load_k / load_v / store_v / compute.  Included as text by attn_decode_body.inc and attn_prefill_body.inc (text for the
// reason attn_decode.hip gives), after the Q prologue and in front of the tile loop.  The including body has in scope:
//   the kernel's D, VB, KB, KV, p;  MB, KS, CB, VROW, VCH, vstage_t, kfrag_t, tile_t, smem;  kv, n, b, hk, lane roles i16, g;
//   qf[MB][KS] (the Q codes; packed K: in the channel order of k4_widen) and lim[MB] (first key a row does NOT see);
//   NT, tix     the NT threads (64: a wave, 256: the workgroup) that share a V tile, and this thread's index among them: thread tix
//               takes the 16-byte chunks u * NT + tix, u < VCH, of the tile;
//   q_scale(rb) the Q scale of row block rb.
// compute(t, gt, kf, masked): tile t of the sequence, named gt to the scale load; masked = std::true_type{} applies the key-limit
// compare, std::false_type{} is for a tile wholly below every limit (same bits).
// The three score statements - name the key, form the product, then the compare - stay in this order and as three statements:
// folded or re-ordered they are the same arithmetic, but the compiler schedules every decode instance differently.
// KB = bits of a cached K code.  8: a lane's 16 codes of a key are 16 bytes, the MFMA operand as it is loaded.  4 (the packed
// cache, kv_policy.h): they are 8 bytes, a tile stays packed in its registers (kfrag_t: half of them) until compute widens it, and
// the score accumulator holds 16 times the byte cache's integer, shifted back before the conversion.  Known to load_k and to the
// score product only; everything from `(float)sacc` on is one text.
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
  const int8_t* k4base = nullptr;  // packed K: rows of D / 2 bytes behind the first key of (b, hk), or of the pool
  if constexpr (KB == 4) k4base = p.k_codes + (KV::key0(p, b, hk) + i16) * (D / 2) + 8 * g;
  const unsigned short* vbase = kv.v;
  const float* ksc = kv.scale;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  typedef __attribute__((address_space(3))) s16x4v lds_s16x4;
  lds_byte* const vt_lane = (lds_byte*)smem + (4 * g + (i16 >> 2)) * VROW + (i16 & 3) * 8;

  auto load_k = [&](tile_t t, kfrag_t (&kf)[4][KS]) __attribute__((always_inline)) {
    if constexpr (KB == 4) {
      const int8_t* kt = k4base + (int64_t)t * 32 * D;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const u32x2*>(kt + kb * 8 * D + 32 * s);
    } else {
      const int8_t* kt = kbase + (int64_t)t * 64 * D;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const i32x4*>(kt + kb * 16 * D + 64 * s);
    }
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
      for (int u = 0; u < VCH; ++u) load_v8_chunk<D>(vt, vsbase + (int64_t)t * 64, u * NT + tix, vr.c[u], vr.s[u]);
    } else {
      const unsigned short* vt = vbase + (int64_t)t * 64 * D;
#pragma unroll
      for (int u = 0; u < VCH; ++u) vr.c[u] = *reinterpret_cast<const uint4*>(vt + (u * NT + tix) * 8);  // the tile is contiguous
    }
  };
  auto store_v = [&](int t, const vstage_t& vr) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < VCH; ++u) {
      if constexpr (VB == 8) {
        store_vhat_chunk<D, VROW>(smem, u * NT + tix, vr.c[u], vr.s[u], n - t * 64);
      } else {
        const int cidx = u * NT + tix, r = cidx / (D / 8), ch = cidx % (D / 8);
        // rows past the end may hold anything (0 * NaN): they enter the product as zeros
        const uint4 val = (t * 64 + r < n) ? vr.c[u] : make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(smem + r * VROW + ch * 16) = val;
      }
    }
  };
  auto compute = [&](int t, tile_t gt, const kfrag_t (&kf)[4][KS], auto masked) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(masked)::value;
    const float kscale = ksc[gt];
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      float sc[4][4];
      float tmax = -__builtin_inff();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        i32x4 sacc = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          if constexpr (KB == 4) sacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(k4_widen(kf[kb][s]), qf[rb][s], sacc, 0, 0, 0);
          else sacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf[kb][s], qf[rb][s], sacc, 0, 0, 0);
        }
        if constexpr (KB == 4) sacc = sacc >> 4;  // 16 (q . k), exactly: the byte cache's integer
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = t * 64 + kb * 16 + 4 * g + r;
          float s2 = (float)sacc[r] * q_scale(rb) * kscale;
          if constexpr (MASK) s2 = key < lim[rb] ? s2 : -__builtin_inff();
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
