"""Long and large, for the nibble-packed K cache: what tests/test_gpu_prefill_long.py asks of the fp8 V cache, asked of
`k_packed=True`.

* 131072 keys through paged decode and cached prefill (2048 scrambled pages of 64, the pool full of garbage) equal the
  byte-per-code `k_bits=4` cache bit for bit, in the chosen slices and in one, causal and not;
* a packed pool whose `k_codes` pass 2^32 bytes, pages handed out from the top: the sequence lives past byte 2^32 of the packed
  codes (and past 2^33 of the fp8 V codes) - `t * 32 * D` of the readers and `gb * 64 * (D / 2)` of the append in 64 bits.
"""
import numpy as np
import pytest

import k4_reference as k4
from test_gpu_paged_kvcache import TDT, _gen, _rand, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    for name, x, y in zip(("O", "LSE"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs"
        assert torch.isfinite(x).all(), f"{what}: {name} is not finite"


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _garbage(cache):
    cache.k_codes.fill_(0x88), cache.k_scale.fill_(float("inf"))
    if cache.v_bits == 8:
        cache.v.fill_(0xFF), cache.v_scale.fill_(float("nan"))
    else:
        cache.v.fill_(float("nan"))
    return cache


def test_long_context_equals_the_byte_cache(dev):
    """131072 keys, one sequence on one kv head: decode of 2 x 2 rows and prefill of 130 queries (two Q blocks) of 2 heads"""
    import lowbit_quant_fa2_paddle_amd as lb
    T, D, G, dtype = 131072, 128, 2, "fp16"
    gen = _gen(dev, 9)
    k, v = _rand(gen, (1, 1, T, D), dtype, dev, bias=0.5), _rand(gen, (1, 1, T, D), dtype, dev)
    qd, qp = _rand(gen, (1, G, 2, D), dtype, dev), _rand(gen, (1, G, 130, D), dtype, dev)
    byte = lb.LowbitKVCache(1, 1, D, T, TDT[dtype], dev, k_bits=4).append(k, v)
    order = np.random.default_rng(13).permutation(2048 + 5).tolist()
    paged = _garbage(lb.LowbitPagedKVCache(2048 + 5, 64, 1, D, 1, 2048, TDT[dtype], dev, k_bits=4, k_packed=True, page_order=order))
    paged.append(k, v)
    got = paged.gather(0)
    assert np.array_equal(k4.unpack(got[0].cpu().numpy()), byte.k_codes[0].cpu().numpy()) and torch.equal(_bits(got[1]), _bits(byte.k_scale[0]))
    for causal in (False, True):
        for ns in (0, 1):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
            what = f"131072 keys causal={causal} splits={ns}"
            _same(lb.lowbit_fa_decode(qd, paged, **kw), lb.lowbit_fa_decode(qd, byte, **kw), what + " decode")
            _same(lb.lowbit_fa_prefill(qp, paged, **kw), lb.lowbit_fa_prefill(qp, byte, **kw), what + " prefill")
    del byte, paged
    _free()


def test_packed_page_offsets_are_formed_in_64_bits(dev):
    """65538 pages of 1024 keys, D = 128, one kv head: 64 KiB of packed codes a page, 2^32 + 2^17 bytes in all (fp8 V: twice that,
    `v_scale` 2^28 bytes - about 12.3 GiB).  Pages come from the top: the 1100 keys live past byte 2^32 of `k_codes`.  Append, decode
    and prefill against a small contiguous byte-per-code cache."""
    import lowbit_quant_fa2_paddle_amd as lb
    page, D, Hkv, G, dtype, n = 1024, 128, 1, 4, "fp16", 1100
    num_pages = (1 << 32) // (page * D // 2) + 2
    paged = _garbage(lb.LowbitPagedKVCache(num_pages, page, Hkv, D, 1, 2, TDT[dtype], dev, k_bits=4, k_packed=True, v_bits=8,
                                           page_order=list(range(num_pages - 1, -1, -1))))
    assert paged.k_codes.numel() > 1 << 32 and paged.k_codes.dtype == torch.uint8
    gen = _gen(dev, 39)
    k, v = _rand(gen, (1, Hkv, n, D), dtype, dev, bias=0.5), 3.0 * _rand(gen, (1, Hkv, n, D), dtype, dev)
    byte = lb.LowbitKVCache(1, Hkv, D, n, TDT[dtype], dev, k_bits=4, v_bits=8).append(k, v)
    paged.append(k, v)
    assert paged.allocator.pages[0] == [num_pages - 1, num_pages - 2] and (num_pages - 2) * page * (D // 2) >= 1 << 32
    kc, ks, vc, vs = paged.gather(0)
    assert np.array_equal(k4.unpack(kc[:, :n].cpu().numpy()), byte.k_codes[0, :, :n].cpu().numpy())
    assert torch.equal(_bits(ks[:, :(n + 63) // 64]), _bits(byte.k_scale[0, :, :(n + 63) // 64]))
    assert torch.equal(vc[:, :n], byte.v[0, :, :n]) and torch.equal(_bits(vs[:, :n]), _bits(byte.v_scale[0, :, :n]))
    for pg in (0, 1, num_pages - 3):  # nothing landed at a wrapped offset
        assert torch.all(paged.k_codes[pg] == 0x88) and torch.all(paged.v[pg] == 0xFF) and torch.isnan(paged.v_scale[pg]).all(), pg
    qd, qp = _rand(gen, (1, G * Hkv, 2, D), dtype, dev), _rand(gen, (1, G * Hkv, 130, D), dtype, dev)
    for ns in (1, 3):
        kw = dict(is_causal=True, return_lse=True, num_splits=ns)
        _same(lb.lowbit_fa_decode(qd, paged, **kw), lb.lowbit_fa_decode(qd, byte, **kw), f"decode splits={ns}")
        _same(lb.lowbit_fa_prefill(qp, paged, **kw), lb.lowbit_fa_prefill(qp, byte, **kw), f"prefill splits={ns}")
    del paged
    _free()
