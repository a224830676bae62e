// Body of kvcache_append_kernel / kvcache_append_v8_kernel (kvcache.hip), included as text inside each with the kernel's template parameters, its parameter
// block `p`, `constexpr int VB` (bits of a cached V element: 16 or 8) and `constexpr int KB` (bits of a stored K code: 8, or 4 for the
// nibble-packed cache) in scope.  See kvcache.hip.
  constexpr int CPR = D / 8;       // 16-byte chunks per row
  constexpr int RPP = 256 / CPR;   // rows per pass
  constexpr int NP = 64 / RPP;     // passes per 64-key block
  __shared__ float wmax[4];
  const int x = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, c = t % CPR, rl = t / CPR;
  int sl, s0, tb;
  if (!Dst::slot(p, b, sl)) return;  // workgroup-uniform
  append_range(p, b, sl, s0, tb);
  if (tb <= 0) return;  // workgroup-uniform
  const int first = s0 >> 6, last = (s0 + tb - 1) >> 6;
  if (x > 0 && first + x >= last) return;
  const int64_t sh = (int64_t)sl * p.Hkv + h;  // (slot, head): k_tail, km
  const unsigned short* knew = p.k_new + (int64_t)b * p.kb + (int64_t)h * p.kh + c * 8;
  const unsigned short* vnew = p.v_new + (int64_t)b * p.vb + (int64_t)h * p.vh + c * 8;
  unsigned short* tail = p.k_tail + sh * 64 * D + c * 8;
  float mean[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) mean[i] = 0.f;
  const bool has_mean = p.km != nullptr;
  if (has_mean) unpack8<DT>(*reinterpret_cast<const uint4*>(p.km + sh * D + c * 8), mean);
  const int end = s0 + tb;

  // x = 0: block `first`, then block `last` when it is another one; x >= 1: one middle block
  const int npass = (x == 0 && last > first) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const int blk = x > 0 ? first + x : (pass == 0 ? first : last);
    const int r0 = blk << 6;
    int64_t gb;
    if (!Dst::block(p, sl, h, blk, gb)) continue;     // workgroup-uniform, before the barriers of the pass: the block is skipped
    int8_t* codes = p.k_codes + gb * 64 * D + c * 8;  // row r0 of the sequence
    unsigned short* vdst = p.v + gb * 64 * D + c * 8;
    uint4 raw[NP];
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      raw[ps] = make_uint4(0, 0, 0, 0);
      if (row < s0) raw[ps] = *reinterpret_cast<const uint4*>(tail + (int64_t)(row - r0) * D);  // only block `first` has such rows
      else if (row < end) raw[ps] = *reinterpret_cast<const uint4*>(knew + (int64_t)(row - s0) * p.ks);
    }
    float xs[NP][8];
    float amax = 0.f;
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      float v[8];
      unpack8<DT>(raw[ps], v);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float xv = v[i];
        // `k - km` in the storage dtype, rows past the end stay 0: exactly quant_per_block_kernel (sm_scale = 1 for K)
        if (has_mean) xv = (row < end) ? load_cvt<DT>(store_cvt<DT>(xv - mean[i])) : 0.f;
        xs[ps][i] = xv;
        amax = fmaxf(amax, fabsf(xv));
      }
    }
    amax = wave_max_nonneg(amax);
    if ((t & 63) == 0) wmax[t >> 6] = amax;
    __syncthreads();  // also: every read of k_tail (pass 0) is done before pass 1 stores to it
    const float scale = block_scale(amax_collect(wmax), p.qmax);
    if (t == 0) p.k_scale[gb] = scale;
    const bool open = (blk == last) && (end & 63) != 0;  // this block is the open one afterwards: keep its raw rows
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int row = r0 + ps * RPP + rl;
      if constexpr (VB == 8) {
        // the threads of a row take the branch together; the reduction inside runs with all lanes, rows not appended read zeros
        const bool mine = row >= s0 && row < end;
        u32x4 vr = u32x4{0, 0, 0, 0};
        if (mine) vr = *reinterpret_cast<const u32x4*>(vnew + (int64_t)(row - s0) * p.vs);
        float vscale;
        const uint2 vcodes = quant_v_row_e4m3<DT, CPR>(vr, vscale);
        if (mine) {
          *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(p.v) + (gb * 64 + (row - r0)) * D + c * 8) = vcodes;
          if (c == 0) p.v_scale[gb * 64 + (row - r0)] = vscale;
        }
      }
      int q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = quant_code<false>(xs[ps][i], scale, 0.f);  // the plain division
      if constexpr (KB == 4) {
        // packed: the row is D / 2 bytes and this thread's 8 codes (|q| <= 7) are 4 of them, channel 2 j low, 2 j + 1 high
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= (unsigned)((q[2 * j] & 15) | ((q[2 * j + 1] & 15) << 4)) << (8 * j);
        if (row < end) *reinterpret_cast<unsigned*>(reinterpret_cast<uint8_t*>(p.k_codes) + (gb * 64 + (row - r0)) * (D / 2) + c * 4) = w;
      } else {
        if (row < end) *reinterpret_cast<uint2*>(codes + (int64_t)(row - r0) * D) = pack8_i8(q);
      }
      if (row >= s0 && row < end) {
        if (open) *reinterpret_cast<uint4*>(tail + (int64_t)(row - r0) * D) = raw[ps];
        if constexpr (VB == 16) {
          u32x4 vr = *reinterpret_cast<const u32x4*>(vnew + (int64_t)(row - s0) * p.vs);
          if constexpr (DT == LBFA_BF16) vr = bf16x8_to_f16x8(vr);
          *reinterpret_cast<u32x4*>(vdst + (int64_t)(row - r0) * D) = vr;
        }
      }
    }
    __syncthreads();  // wmax is reused by the second pass
  }
