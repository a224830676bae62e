"""Long and large, for cached prefill and the fp8 V cache: what tests/test_gpu_kvcache_decode.py (131072 keys) and
tests/test_gpu_paged_kvcache.py (2048 scrambled pages, a pool past 2^32 bytes) ask of fp16 decode, asked of `lowbit_fa_prefill`
and of the `v_bits = 8` readers and writers, plus a CONTIGUOUS cache whose second sequence starts 2^31 elements in.

* 131072 keys through prefill: sampled rows against the oracle's kernel on the cache's own codes, the paged cache and the fp8
  twin bit for bit;
* an fp8 pool whose V codes exceed 2^32 bytes, pages handed out from the top;
* a contiguous cache of capacity 2^24 with B = 2: sequence 1 starts 2^31 elements into the codes and V and 2^24 scales into
  `v_scale` - `bh * cap * D`, `key0 * D` and `vsbase + t * 64` past 32 bits.
"""
import types

import numpy as np
import pytest

import kvcache_reference as kr
import prefill_reference as pr
import v8_reference as v8
from test_gpu_paged_kvcache import TDT, _gen, _paged, _rand, _state_equal, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    for name, x, y in zip(("O", "LSE"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs"


def _np(t):
    return t.detach().float().cpu().numpy()


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _garbage_v8(cache):
    cache.k_codes.fill_(127), cache.k_scale.fill_(float("inf")), cache.v.fill_(0xFF), cache.v_scale.fill_(float("nan"))
    return cache


def test_prefill_long_context(oracle, dev):
    """131072 keys, one sequence, 130 queries (two Q blocks) of 2 heads on one kv head: 2048 tiles in the chosen 128 slices and in
    one, causal and not.  Rows 0, 63, 127, 128, 129 against the oracle's single pass over each row's visible keys (the cache's own
    codes: their equality with the dense quantiser is tested in tests/test_gpu_kvcache_decode.py); the paged cache through 2048
    scrambled pages of 64 and the fp8 twin (against the fp16 cache holding V^) bit for bit."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    T, D, G, Sq, dtype, rows = 131072, 128, 2, 130, "fp16", [0, 63, 127, 128, 129]
    assert _lib.load().lbfa_prefill_num_splits(1, G, Sq, T) == 128
    gen = _gen(dev, 7)
    k, v = _rand(gen, (1, 1, T, D), dtype, dev, bias=0.5), _rand(gen, (1, 1, T, D), dtype, dev)
    q = _rand(gen, (1, G, Sq, D), dtype, dev)
    dense = lb.LowbitKVCache(1, 1, D, T, TDT[dtype], dev).append(k, v)
    paged = _paged(dev, num_pages=2048 + 5, page=64, Hkv=1, D=D, max_seqs=1, max_pages=2048, dtype=dtype, seed=11).append(k, v)
    _state_equal(paged, 0, dense, 0, T, "131072 keys")
    dense8 = lb.LowbitKVCache(1, 1, D, T, TDT[dtype], dev, v_bits=8).append(k, v)
    vhat = v8.dequant_v(oracle, dense8.v.cpu().numpy(), dense8.v_scale.cpu().numpy())
    holds_vhat = lb.LowbitKVCache(1, 1, D, T, TDT[dtype], dev).append(k, v)
    holds_vhat.v.copy_(torch.from_numpy(vhat).to(dev))
    assert not torch.equal(holds_vhat.v, dense.v)
    # the reference
    sm = D ** -0.5
    qn = _np(q)
    q_i8, q_scale = pr.quant_q_blocks(oracle, qn, [Sq], sm, 127)
    ref = types.SimpleNamespace(k_codes=dense.k_codes.cpu().numpy(), k_scale=dense.k_scale.cpu().numpy(), v=_np(dense.v),
                                seqlens=np.array([T]))
    corr = kr.lse_correction(oracle, qn, _np(dense.km), dtype)[0][:, rows]
    for causal in (False, True):
        o_ref, lse2_ref = pr.oracle_prefill_rows(oracle, q_i8, q_scale, ref, 0, rows, q_len=Sq, causal=causal, out_dtype=dtype)
        lse_ref = kr.natural_lse(lse2_ref, corr, sm)
        for ns in (0, 1):
            what = f"131072 keys causal={causal} splits={ns}"
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
            o, lse = lb.lowbit_fa_prefill(q, dense, **kw)
            assert torch.isfinite(o).all() and torch.isfinite(lse).all(), what
            kr.check_o(_np(o)[0][:, rows], o_ref, dtype, what)
            kr.check_lse(lse.cpu().numpy()[0][:, rows], lse_ref, corr, sm, dtype, what)
            _same(lb.lowbit_fa_prefill(q, paged, **kw), (o, lse), what + " paged")
            _same(lb.lowbit_fa_prefill(q, dense8, **kw), lb.lowbit_fa_prefill(q, holds_vhat, **kw), what + " fp8 V against V^")
    del dense, paged, dense8, holds_vhat
    _free()


def test_fp8_page_offsets_are_formed_in_64_bits(dev):
    """The fp8 form of tests/test_gpu_paged_kvcache.py::test_page_offsets_are_formed_in_64_bits: a pool whose V CODES exceed 2^32
    bytes (32770 pages of 1024 keys, D = 128; K codes as large, `v_scale` 2^27 bytes: about 8.2 GiB), pages handed out from the top.
    The short sequence lives past byte 2^32 of both code tensors.  Append, decode and prefill against a small contiguous fp8 cache."""
    import lowbit_quant_fa2_paddle_amd as lb
    page, D, Hkv, G, dtype, n = 1024, 128, 1, 4, "fp16", 1100
    num_pages = (1 << 32) // (page * D) + 2
    paged = _garbage_v8(lb.LowbitPagedKVCache(num_pages, page, Hkv, D, 1, 2, TDT[dtype], dev, v_bits=8,
                                              page_order=list(range(num_pages - 1, -1, -1))))
    assert paged.v.numel() * paged.v.element_size() > 1 << 32 and paged.v.dtype == torch.uint8
    gen = _gen(dev, 37)
    k, v = _rand(gen, (1, Hkv, n, D), dtype, dev, bias=0.5), 3.0 * _rand(gen, (1, Hkv, n, D), dtype, dev)
    dense = lb.LowbitKVCache(1, Hkv, D, n, TDT[dtype], dev, v_bits=8).append(k, v)
    paged.append(k, v)
    assert paged.allocator.pages[0] == [num_pages - 1, num_pages - 2] and (num_pages - 2) * page * D >= 1 << 32
    kc, ks, vc, vs = paged.gather(0)
    assert torch.equal(kc[:, :n], dense.k_codes[0, :, :n]) and torch.equal(_bits(ks[:, :(n + 63) // 64]), _bits(dense.k_scale[0, :, :(n + 63) // 64]))
    assert torch.equal(vc[:, :n], dense.v[0, :, :n]) and torch.equal(_bits(vs[:, :n]), _bits(dense.v_scale[0, :, :n]))
    for pg in (0, num_pages - 3):  # nothing landed at a wrapped offset
        assert torch.all(paged.v[pg] == 0xFF) and torch.isnan(paged.v_scale[pg]).all() and torch.all(paged.k_codes[pg] == 127), pg
    qd, qp = _rand(gen, (1, G * Hkv, 2, D), dtype, dev), _rand(gen, (1, G * Hkv, 130, D), dtype, dev)
    for ns in (1, 3):
        kw = dict(is_causal=True, return_lse=True, num_splits=ns)
        _same(lb.lowbit_fa_decode(qd, paged, **kw), lb.lowbit_fa_decode(qd, dense, **kw), f"decode splits={ns}")
        _same(lb.lowbit_fa_prefill(qp, paged, **kw), lb.lowbit_fa_prefill(qp, dense, **kw), f"prefill splits={ns}")
    del paged
    _free()


K_FILL, V16_FILL, V8_FILL, SCALE_FILL = 0x5A, 77.0, 0xA5, 1234.5  # what rows nobody appended hold


@pytest.mark.parametrize("v_bits", [16, 8])
def test_contiguous_cache_past_2_31_elements(dev, v_bits):
    """B = 2, Hkv = 1, D = 128, capacity 2^24: sequence 1 starts 2^31 elements into the codes and V, 2^18 into `k_scale` and (fp8)
    2^24 into `v_scale`.  130 keys are appended in two steps; append, decode and prefill must equal a capacity-192 cache bit for
    bit, and the rows just before sequence 1's start keep their fill value.  Peak device memory: about 12 GiB with fp16 V (4 GiB
    of codes, 8 GiB of V), about 8 GiB with fp8 V (4 + 4 GiB and 2^27 bytes of scales)."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, Hkv, D, G, cap, n, dtype = 2, 1, 128, 2, 1 << 24, 130, "fp16"
    assert Hkv * cap * D == 1 << 31
    gen = _gen(dev, 41 + v_bits)
    k, v = _rand(gen, (B, Hkv, n, D), dtype, dev, bias=0.5), 3.0 * _rand(gen, (B, Hkv, n, D), dtype, dev)
    big = lb.LowbitKVCache(B, Hkv, D, cap, TDT[dtype], dev, v_bits=v_bits)
    small = lb.LowbitKVCache(B, Hkv, D, 192, TDT[dtype], dev, v_bits=v_bits)
    assert big.k_codes.numel() == 1 << 32 and big.v.numel() == 1 << 32
    big.k_codes.fill_(K_FILL), big.k_scale.fill_(SCALE_FILL), big.v.fill_(V8_FILL if v_bits == 8 else V16_FILL)
    if v_bits == 8:
        big.v_scale.fill_(SCALE_FILL)
    new_lens = torch.tensor([70, 66], dtype=torch.int32, device=dev)
    for cache in (big, small):
        cache.append(k[:, :, :70], v[:, :, :70], new_lens=new_lens)
        cache.append(k[:, :, 70:], v[:, :, 70:])
    assert big.seqlens.tolist() == small.seqlens.tolist() == [130, 126]
    names = ("k_codes", "k_scale", "v") + (("v_scale",) if v_bits == 8 else ())
    for b, m in enumerate(big.seqlens.tolist()):
        for name in names:
            rows = (m + 63) // 64 if name == "k_scale" else m
            assert torch.equal(_bits(getattr(big, name)[b, :, :rows]), _bits(getattr(small, name)[b, :, :rows])), (b, name)
    for name in ("k_tail", "km", "seqlens"):
        assert torch.equal(_bits(getattr(big, name)), _bits(getattr(small, name))), name
    # the rows before sequence 1's start (the end of sequence 0's slab) and behind its keys hold what they held
    assert torch.all(big.k_codes[0, :, -4096:] == K_FILL) and torch.all(big.k_codes[1, :, 192:4096] == K_FILL)
    assert torch.all(big.k_scale[0, :, -64:] == SCALE_FILL) and torch.all(big.k_scale[1, :, 3:64] == SCALE_FILL)
    assert torch.all(big.v[0, :, -4096:] == (V8_FILL if v_bits == 8 else V16_FILL)) and torch.all(big.v[1, :, 126:4096] == (V8_FILL if v_bits == 8 else V16_FILL))
    if v_bits == 8:
        assert torch.all(big.v_scale[0, :, -4096:] == SCALE_FILL) and torch.all(big.v_scale[1, :, 126:4096] == SCALE_FILL)
    qd, qp = _rand(gen, (B, G * Hkv, 2, D), dtype, dev), _rand(gen, (B, G * Hkv, 130, D), dtype, dev)
    for ns in (1, 3):
        kw = dict(is_causal=True, return_lse=True, num_splits=ns)
        _same(lb.lowbit_fa_decode(qd, big, **kw), lb.lowbit_fa_decode(qd, small, **kw), f"decode splits={ns}")
        _same(lb.lowbit_fa_prefill(qp, big, **kw), lb.lowbit_fa_prefill(qp, small, **kw), f"prefill splits={ns}")
        out = lb.lowbit_fa_prefill(qp, big, **kw)
        assert torch.isfinite(out[0]).all() and not torch.isnan(out[1]).any()
    del big
    _free()
