"""Numpy restatement of the int8 KV cache and of split-KV decode attention (test infrastructure, like tests/bwd_reference.py).

* `CacheRef`: the stateful append - raw rows of the open 64-key block kept in a tail, every touched block re-quantised from
  tail + new rows.  tests/test_kvcache_reference_cpu.py shows it equals `oracle.per_block_int8` on the concatenated K bit for bit.
* `split_kv_decode`: what `lbfa_decode` computes - per key slice an online softmax over 64-key tiles, then a fixed-order combine.
* `oracle_decode`: the REFERENCE of every decode test: `oracle.attn_fwd_int8_fp16(..., tail="neg_inf")` on the cache's codes, one
  sequence at a time on its own length; causal (bottom-right aligned) = the non-causal oracle kernel, per query row i, on the first
  n - Sq + 1 + i keys with the shared q scale.
* the bounds of tests/test_gpu_parity.py.
"""
import numpy as np

LOG2E = 1.44269504
BLKK = 64


# ------------------------------------------------------------------------------------------------------------------------
# bounds (tests/test_gpu_parity.py: `_o_close`, and the LSE check of test_operator_int8_fp16_vs_oracle)
# ------------------------------------------------------------------------------------------------------------------------
def o_bound(ref, dtype):
    """|dO| <= 2e-3 + 2e-3 |O| per element; a bf16 output adds one bf16 ulp (2^-7 relative)"""
    rtol = 2e-3 + (2.0 ** -7 if dtype == "bf16" else 0.0)
    return 2e-3 + rtol * np.abs(ref)


def lse_bound(corr, sm_scale, dtype):
    """1e-3 plus one storage-dtype ulp of the correction dtype(q . km) * sm_scale, per element (`corr` = dtype(q . km), or None)"""
    if corr is None:
        return 1e-3
    return 1e-3 + (2.0 ** -10 if dtype == "fp16" else 2.0 ** -7) * np.abs(corr) * sm_scale


def check_o(o, ref, dtype, what=""):
    err = np.abs(o.astype(np.float64) - ref.astype(np.float64))
    bnd = o_bound(ref, dtype)
    worst = float((err / bnd).max()) if err.size else 0.0
    print(f"{what} O: worst element at {worst:.3f} of the bound")
    assert worst <= 1.0, f"{what}: O beyond the bound, worst ratio {worst:.3f}, max err {err.max():.3e}"
    return worst


def check_lse(lse, ref, corr, sm_scale, dtype, what=""):
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(lse) & (lse < 0), inf), f"{what}: -inf rows differ"
    err = np.abs(np.where(inf, 0.0, lse.astype(np.float64)) - np.where(inf, 0.0, ref.astype(np.float64)))
    bnd = lse_bound(corr, sm_scale, dtype)
    worst = float((err / bnd).max()) if err.size else 0.0
    print(f"{what} LSE: worst element at {worst:.3f} of the bound")
    assert worst <= 1.0, f"{what}: LSE beyond the bound, worst ratio {worst:.3f}, max err {err.max():.3e}"
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# the cache
# ------------------------------------------------------------------------------------------------------------------------
def _quant_block(orc, rows, km, dtype, qmax):
    """codes and scale of ONE block of <= 64 raw rows [n, D] (fp32-valued storage dtype): dtype(K - km), amax of the rows
    present floored at 1e-7, round half away from zero - `quant_per_block_kernel` on a single block"""
    x = rows.astype(np.float32)
    if km is not None:
        x = orc.to_storage(x - km.astype(np.float32)[None, :], dtype)
    amax = np.maximum(np.max(np.abs(x)) if x.size else np.float32(0), np.float32(1e-7)).astype(np.float32)
    scale = np.float32(amax / np.float32(qmax))
    y = x / scale
    y = y + np.float32(0.5) * np.where(y >= 0, np.float32(1), np.float32(-1))
    return np.trunc(y).astype(np.int32).astype(np.int8), scale


class CacheRef:
    """State of `lbfa_kvcache_append` in numpy: k_codes [B,H,cap,D] int8, k_scale [B,H,cap/64], v [B,H,cap,D] fp16 values,
    k_tail [B,H,64,D], km [B,H,D] or None, seqlens [B]."""

    def __init__(self, orc, B, H, D, cap, dtype, qmax=127, smooth_k=True):
        assert cap % BLKK == 0
        self.orc, self.B, self.H, self.D, self.cap, self.dtype, self.qmax, self.smooth_k = orc, B, H, D, cap, dtype, qmax, smooth_k
        self.k_codes = np.zeros((B, H, cap, D), np.int8)
        self.k_scale = np.zeros((B, H, cap // BLKK), np.float32)
        self.v = np.zeros((B, H, cap, D), np.float32)
        self.k_tail = np.zeros((B, H, BLKK, D), np.float32)
        self.km = None
        self.seqlens = np.zeros(B, np.int64)

    def append(self, k_new, v_new, new_lens=None):
        """k_new, v_new [B,H,T,D] fp32-valued in the storage dtype; new_lens [B] or None"""
        orc, T = self.orc, k_new.shape[2]
        lens = np.full(self.B, T) if new_lens is None else np.clip(np.asarray(new_lens), 0, T)
        if self.smooth_k and self.km is None:  # first append: storage-dtype mean of its valid rows (zeros for an empty one)
            self.km = np.zeros((self.B, self.H, self.D), np.float32)
            for b in range(self.B):
                if lens[b]:
                    m = np.mean(k_new[b, :, :lens[b]].astype(np.float64), axis=1).astype(np.float32)
                    self.km[b] = orc.to_storage(m, self.dtype)
        for b in range(self.B):
            # the device-side clipping of `append_range` (kvcache.hip): a length outside [0, cap] is clamped, rows that would pass
            # the capacity are dropped
            s0 = min(max(int(self.seqlens[b]), 0), self.cap)
            tb = min(int(lens[b]), self.cap - s0)
            if tb <= 0:
                continue
            end = s0 + tb
            first, last = s0 // BLKK, (end - 1) // BLKK
            for h in range(self.H):
                km = self.km[b, h] if self.smooth_k else None
                for blk in range(first, last + 1):
                    r0, r1 = blk * BLKK, min(blk * BLKK + BLKK, end)
                    old = self.k_tail[b, h, :max(s0 - r0, 0)]                       # rows of the open block already there
                    new = k_new[b, h, max(r0 - s0, 0):r1 - s0]
                    rows = np.concatenate([old, new], axis=0)
                    codes, scale = _quant_block(orc, rows, km, self.dtype, self.qmax)
                    self.k_codes[b, h, r0:r1] = codes
                    self.k_scale[b, h, blk] = scale
                    if blk == last and end % BLKK:
                        self.k_tail[b, h, :r1 - r0] = rows                         # the new open block
                self.v[b, h, s0:end] = v_new[b, h, :tb].astype(np.float16).astype(np.float32)
            self.seqlens[b] = end


def dense_k_codes(orc, k, km, dtype, qmax):
    """the dense quantiser on a whole K [B,H,S,D] (`oracle.per_block_int8`, the 1e-7 floor of the HIP path): codes, scales"""
    q_dummy = np.zeros((k.shape[0], k.shape[1], 1, k.shape[3]), np.float32)
    _, _, k_i8, k_scale = orc.per_block_int8(q_dummy, k, None if km is None else km[:, :, None, :], 1.0, dtype,
                                             q_qmax=127.0, k_qmax=float(qmax), amax_floor=1e-7)
    return k_i8, k_scale


# ------------------------------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------------------------------
def quant_q(orc, q, sm_scale, qmax):
    """q [B,Hq,Sq,D] (Sq <= 128): one block per (b, h), sm_scale * log2(e) folded in as ONE fp32 -> codes, scale [B,Hq]"""
    q_i8, q_scale = orc.quant_per_block(q, np.float32(float(sm_scale) * LOG2E), float(qmax), 128, 1e-7)
    return q_i8, q_scale[:, :, 0]


def lse_correction(orc, q, km, dtype):
    """dtype(q . km) [B,Hq,Sq] (src/core.py:294-304), km [B,Hkv,D] or None"""
    if km is None:
        return None
    g = q.shape[1] // km.shape[1]
    kmq = np.repeat(km, g, axis=1)
    return orc.to_storage(np.einsum("bhsd,bhd->bhs", q.astype(np.float32), kmq.astype(np.float32)), dtype)


def natural_lse(lse2, corr, sm_scale):
    lse = lse2 / np.float32(LOG2E)
    return lse if corr is None else lse + corr * np.float32(sm_scale)


def split_kv_decode(orc, q_i8, q_scale, k_i8, k_scale, v16, seqlens, *, causal, num_splits, out_dtype):
    """The decode kernel in numpy.  k_i8 [B,Hkv,cap,D], k_scale [B,Hkv,cap/64], v16 [B,Hkv,cap,D] -> o [B,Hq,Sq,D] rounded to
    out_dtype, lse2 [B,Hq,Sq] (base 2; -inf where a query sees no key)."""
    B, Hq, Sq, D = q_i8.shape
    Hkv = k_i8.shape[1]
    g = Hq // Hkv
    o = np.zeros((B, Hq, Sq, D), np.float32)
    lse2 = np.full((B, Hq, Sq), -np.inf, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            n = int(seqlens[b])
            ntiles = (n + BLKK - 1) // BLKK
            tps = (ntiles + num_splits - 1) // num_splits
            lim = (n - Sq + 1 + np.arange(Sq)) if causal else np.full(Sq, n)
            for h in range(Hq):
                hk = h // g
                qf = q_i8[b, h].astype(np.float32)
                parts = []
                for s in range(num_splits):
                    m = np.full(Sq, -np.inf, np.float32)
                    l = np.zeros(Sq, np.float32)
                    acc = np.zeros((Sq, D), np.float32)
                    for t in range(s * tps, min((s + 1) * tps, ntiles)):
                        keys = np.arange(t * BLKK, (t + 1) * BLKK)
                        qk = (qf @ k_i8[b, hk, keys].astype(np.float32).T).astype(np.float32)
                        qk = qk * q_scale[b, h] * k_scale[b, hk, t]
                        qk = np.where(keys[None, :] < lim[:, None], qk, np.float32(-np.inf))
                        m_new = np.maximum(m, qk.max(axis=1))
                        m_use = np.where(np.isinf(m_new), np.float32(0), m_new)
                        alpha = np.exp2(m - m_use).astype(np.float32)
                        p = np.exp2(qk - m_use[:, None]).astype(np.float32)
                        l = l * alpha + p.sum(axis=1, dtype=np.float32)
                        vt = np.where((keys < n)[:, None], v16[b, hk, keys], np.float32(0))
                        acc = acc * alpha[:, None] + p.astype(np.float16).astype(np.float32) @ vt.astype(np.float32)
                        m = m_new
                    parts.append((m, l, acc))
                if num_splits == 1:
                    m, l, acc = parts[0]
                else:  # fixed-order combine: 256 / D groups add contiguous runs of slices in order, then the groups in order
                    m = np.full(Sq, -np.inf, np.float32)
                    for ms, _, _ in parts:
                        m = np.maximum(m, ms)
                    ng = 256 // D
                    chunk = (num_splits + ng - 1) // ng
                    l = acc = None
                    for gi in range(ng):
                        lg = np.zeros(Sq, np.float32)
                        ag = np.zeros((Sq, D), np.float32)
                        for ms, ls, accs in parts[gi * chunk:(gi + 1) * chunk]:
                            w = np.where(np.isinf(ms), np.float32(0), np.exp2(ms - np.where(np.isinf(m), np.float32(0), m))).astype(np.float32)
                            lg = lg + ls * w
                            ag = ag + accs * w[:, None]
                        l, acc = (lg, ag) if l is None else (l + lg, acc + ag)
                inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
                o[b, h] = acc * inv[:, None]
                lse2[b, h] = np.where(l > 0, np.log2(np.where(l > 0, l, np.float32(1))) + m, np.float32(-np.inf))
    return orc.to_storage(o, out_dtype), lse2


def oracle_decode(orc, q_i8, q_scale, k_i8, k_scale, v16, seqlens, *, causal, out_dtype):
    """The reference: the oracle's int8 / fp16 kernel with -inf tails on each sequence's own keys (see the module docstring)."""
    B, Hq, Sq, D = q_i8.shape
    o = np.zeros((B, Hq, Sq, D), np.float32)
    lse2 = np.full((B, Hq, Sq), -np.inf, np.float32)

    def run(b, rows, n):
        ob, lb = orc.attn_fwd_int8_fp16(q_i8[b:b + 1, :, rows], k_i8[b:b + 1, :, :n], v16[b:b + 1, :, :n],
                                        q_scale[b:b + 1, :, None], k_scale[b:b + 1, :, :(n + BLKK - 1) // BLKK], causal=False,
                                        out_dtype=out_dtype, return_lse=True, tail="neg_inf")
        o[b, :, rows] = ob[0]
        lse2[b, :, rows] = lb[0]

    for b in range(B):
        n = int(seqlens[b])
        if not causal:
            if n > 0:
                run(b, slice(None), n)
            continue
        for i in range(Sq):
            ni = n - Sq + 1 + i
            if ni > 0:
                run(b, slice(i, i + 1), ni)
    return o, lse2
