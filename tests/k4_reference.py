"""Numpy model of the nibble-packed int4 K cache (`k_packed=True`; test infrastructure, like tests/kvcache_reference.py).

The format (include/lowbit_fa.h): a row of D codes in [-7, 7] is D / 2 bytes; byte j holds channel 2 j in bits 0..3 and channel
2 j + 1 in bits 4..7, each nibble the two's-complement 4-bit value of the code.  -8 (nibble 8) is never produced.

* `pack` / `unpack`: the layout, on the last axis.
* `CacheRefK4`: `kvcache_reference.CacheRef` with qmax 7 - the byte-per-code `k_bits=4` cache - and `k_packed`, its codes packed.
* `oracle_decode` / `oracle_prefill`: readers of the packed state - unpack, then the existing references.  An integer score does not
  depend on the order of its channels, so a reader of the packed cache is a reader of the byte cache.
"""
import types

import numpy as np

import kvcache_reference as kr
import prefill_reference as pr


def pack(codes):
    """int8 [..., D] with every code in [-8, 7] -> uint8 [..., D / 2]"""
    c = np.asarray(codes)
    assert c.dtype == np.int8 and c.shape[-1] % 2 == 0 and c.min(initial=0) >= -8 and c.max(initial=0) <= 7
    n = c.astype(np.uint8) & np.uint8(15)
    return (n[..., 0::2] | (n[..., 1::2] << np.uint8(4))).astype(np.uint8)


def unpack(packed):
    """uint8 [..., n] -> int8 [..., 2 n]"""
    p = np.asarray(packed)
    assert p.dtype == np.uint8
    out = np.empty(p.shape[:-1] + (2 * p.shape[-1],), np.int8)
    for half, nib in ((0, p & np.uint8(15)), (1, p >> np.uint8(4))):
        out[..., half::2] = nib.astype(np.int16) - 16 * (nib >> np.uint8(3)).astype(np.int16)
    return out


class CacheRefK4(kr.CacheRef):
    """State of `lbfa_kvcache_append_k4` in numpy: `CacheRef` with qmax 7; `k_packed` is what `k_codes` of the packed cache holds"""

    def __init__(self, orc, B, H, D, cap, dtype, smooth_k=True):
        super().__init__(orc, B, H, D, cap, dtype, 7, smooth_k)

    @property
    def k_packed(self):
        return pack(self.k_codes)


def oracle_decode(orc, q_i8, q_scale, k_packed, k_scale, v16, seqlens, *, causal, out_dtype):
    return kr.oracle_decode(orc, q_i8, q_scale, unpack(k_packed), k_scale, v16, seqlens, causal=causal, out_dtype=out_dtype)


def oracle_prefill(orc, q_i8, q_scale, k_packed, k_scale, v16, seqlens, q_lens, *, causal, out_dtype):
    ref = types.SimpleNamespace(k_codes=unpack(k_packed), k_scale=k_scale, v=v16, seqlens=np.asarray(seqlens))
    return pr.oracle_prefill(orc, q_i8, q_scale, ref, q_lens, causal=causal, out_dtype=out_dtype)
