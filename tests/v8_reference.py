"""Numpy model of the fp8 V cache (`v_bits=8`; test infrastructure, like tests/kvcache_reference.py), on the oracle's e4m3 codec.

* `quant_v_rows`: the quantiser of one appended row over its D channels, all in fp32: x = fp32(v), amax = max(max |x|, 1e-7),
  scale = amax / 448, code = e4m3fn_rne(x / scale).  A row depends on nothing but itself.
* `dequant_v`: what a reader sees, V^ = fp16_rne(fp32(decode(code)) * scale): one fp32 multiply, one conversion.
* `v_error_bound`: |V^ - V| <= (2^-4 + 2^-10) |V| + 2^-10 scale + 2^-24 per element, for finite input.  Where it comes from:
  y = x / scale is within 2^-24 |y| of the quotient; e4m3 rounds a normal y (|y| >= 2^-6) by at most 2^-4 |y| and a subnormal
  one by at most 2^-10; the product with scale is rounded to fp32 (2^-24 relative) and to fp16 (2^-11 relative, or 2^-25
  absolute below the fp16 normals) - the lower-order terms fit into the 2^-10 |V| and the 2^-24.
* `CacheRefV8`: `kvcache_reference.CacheRef` (the K state and the fp16 V are its) with the fp8 V state next to it.
"""
import numpy as np

import kvcache_reference as kr

E4M3_MAX = np.float32(448.0)
AMAX_FLOOR = np.float32(1e-7)  # the K quantiser's


def quant_v_rows(orc, v, dtype):
    """v [..., D] fp32-valued in the storage dtype `dtype` -> codes uint8 [..., D] (e4m3fn bit patterns), scale fp32 [...]"""
    x = orc.to_storage(np.asarray(v, np.float32), dtype)
    amax = np.maximum(np.max(np.abs(x), axis=-1), AMAX_FLOOR).astype(np.float32)
    scale = (amax / E4M3_MAX).astype(np.float32)
    y = (x / scale[..., None]).astype(np.float32)
    return orc.e4m3fn_encode(orc.e4m3fn_round(y)), scale


def scaled(orc, v, dtype):
    """x / scale of `quant_v_rows`, fp32 - what the conversion is given"""
    x = orc.to_storage(np.asarray(v, np.float32), dtype)
    amax = np.maximum(np.max(np.abs(x), axis=-1), AMAX_FLOOR).astype(np.float32)
    return (x / (amax / E4M3_MAX).astype(np.float32)[..., None]).astype(np.float32)


def dequant_v(orc, codes, scale):
    """V^ as fp16 values: fp16_rne(fp32(decode(code)) * scale), fp16 subnormals kept"""
    with np.errstate(all="ignore"):  # garbage rows (NaN codes, inf scales) are the caller's to ignore
        return (orc.e4m3fn_decode(codes).astype(np.float32) * np.asarray(scale, np.float32)[..., None]).astype(np.float32).astype(np.float16)


def v_error_bound(v, scale):
    return (2.0 ** -4 + 2.0 ** -10) * np.abs(np.asarray(v, np.float64)) + 2.0 ** -10 * np.asarray(scale, np.float64)[..., None] + 2.0 ** -24


class CacheRefV8(kr.CacheRef):
    """State of `lbfa_kvcache_append_v8` in numpy: everything of `CacheRef` (K state; `v` is the fp16 cache's V), plus v_codes
    uint8 [B,H,cap,D] and v_scale fp32 [B,H,cap] of the valid rows.  `vhat()` is the V a reader sees (fp32-valued fp16)."""

    def __init__(self, orc, B, H, D, cap, dtype, qmax=127, smooth_k=True):
        super().__init__(orc, B, H, D, cap, dtype, qmax, smooth_k)
        self.v_codes = np.zeros((B, H, cap, D), np.uint8)
        self.v_scale = np.zeros((B, H, cap), np.float32)

    def append(self, k_new, v_new, new_lens=None):
        before = self.seqlens.copy()
        super().append(k_new, v_new, new_lens)
        for b in range(self.B):
            s0, end = min(max(int(before[b]), 0), self.cap), int(self.seqlens[b])
            if end > s0 and end != before[b]:
                self.v_codes[b, :, s0:end], self.v_scale[b, :, s0:end] = quant_v_rows(self.orc, v_new[b, :, :end - s0], self.dtype)

    def vhat(self):
        return dequant_v(self.orc, self.v_codes, self.v_scale).astype(np.float32)
