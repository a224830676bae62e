"""GPU tests of the paged int8 KV cache (`LowbitPagedKVCache`, lbfa_kvcache_paged_append) and of block-table decode attention
(`lowbit_fa_decode` on it, lbfa_decode_paged).

The yardstick is the contiguous cache (`LowbitKVCache`), which tests/test_gpu_kvcache_decode.py ties to the dense quantiser and
to the oracle: the same appends must leave bit-identical state, the same decode must give `torch.equal` O and LSE for the same
`num_splits` - a page never splits a 64-key tile or quantiser block, so arithmetic and order are unchanged.  Two decode cases
are also checked against the oracle directly, through the gathered state, so the new kernel has a check that does not pass
through the old one.

Every pool is filled with garbage after construction (codes 127, scales inf, V NaN) and its pages are handed out in a scrambled
order: a read of a row past a sequence's end, or of a page that is not its own, shows up in the result.
"""
import numpy as np
import pytest

import kvcache_reference as kr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
STEPS = [(70, None), (1, [1, 1, 0]), (1, [1, 0, 1]), (63, [63, 10, 0]), (64, [64, 64, 33]), (65, [0, 65, 64]), (200, [200, 1, 150])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from lowbit_quant_fa2_paddle_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _rand(gen, shape, dtype, dev, bias=0.0):
    return (torch.randn(shape, generator=gen, device=dev, dtype=torch.float32) + bias).to(TDT[dtype])


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _nhd(t):
    return t.transpose(1, 2).contiguous()


def _paged(dev, *, num_pages, page, Hkv, D, max_seqs, max_pages, dtype, k_bits=8, seed=0, order=None, smooth_k=True):
    """a paged cache full of garbage whose pages come in a scrambled order"""
    import lowbit_quant_fa2_paddle_amd as lb
    if order is None:
        order = np.random.default_rng(seed).permutation(num_pages).tolist()
    cache = lb.LowbitPagedKVCache(num_pages, page, Hkv, D, max_seqs, max_pages, TDT[dtype], dev, k_bits=k_bits, smooth_k=smooth_k,
                                  page_order=order)
    cache.k_codes.fill_(127)
    cache.k_scale.fill_(float("inf"))
    cache.v.fill_(float("nan"))
    return cache


def _state_equal(paged, slot, dense, b, n, what):
    """the first n keys of `slot` through its table == those of sequence b of the contiguous cache, bit for bit"""
    codes, scales, v = paged.gather(slot)
    nb = (n + 63) // 64
    assert codes.shape[1] >= n, what
    assert torch.equal(codes[:, :n], dense.k_codes[b, :, :n]), (what, "codes")
    assert torch.equal(scales[:, :nb].view(torch.int32), dense.k_scale[b, :, :nb].view(torch.int32)), (what, "scales")
    assert torch.equal(v[:, :n].view(torch.int16), dense.v[b, :, :n].view(torch.int16)), (what, "v")
    assert int(paged.seqlens[slot]) == int(dense.seqlens[b]) == n, (what, "seqlens")
    if dense.km is not None:
        assert torch.equal(paged.km[slot].view(torch.int16), dense.km[b].view(torch.int16)), (what, "km")


# ------------------------------------------------------------------------------------------------------------------------
# 1. append equals the contiguous cache
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k_bits,D,page", [("fp16", 8, 64, 64), ("bf16", 4, 128, 128), ("fp16", 8, 80, 192)])
def test_append_equals_contiguous_after_every_step(dev, dtype, k_bits, D, page):
    import lowbit_quant_fa2_paddle_amd as lb
    B, H = 3, 2
    total = sum(T for T, _ in STEPS)
    max_pages = -(-total // page)
    gen = _gen(dev, 11 + D + k_bits)
    dense = lb.LowbitKVCache(B, H, D, total, TDT[dtype], dev, k_bits=k_bits)
    paged = _paged(dev, num_pages=B * max_pages + 2, page=page, Hkv=H, D=D, max_seqs=B, max_pages=max_pages, dtype=dtype,
                   k_bits=k_bits, seed=page)
    n = [0] * B
    for step, (T, lens) in enumerate(STEPS):
        k, v = _rand(gen, (B, H, T, D), dtype, dev, bias=0.5), _rand(gen, (B, H, T, D), dtype, dev)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        if step % 2:
            dense.append(_nhd(k), _nhd(v), tensor_layout="NHD", new_lens=tl)
            paged.append(_nhd(k), _nhd(v), tensor_layout="NHD", new_lens=tl)
        else:
            dense.append(k, v, new_lens=tl)
            paged.append(k, v, new_lens=tl)
        for b in range(B):
            n[b] += T if lens is None else lens[b]
            _state_equal(paged, b, dense, b, n[b], f"step {step} sequence {b}")
    assert n == [399, 211, 318]
    assert paged.num_free_pages == 2 and paged.max_seqlen() == total
    with pytest.raises(ValueError, match="capacity"):
        paged.append(k, v)
    assert paged.num_free_pages == 2 and paged.max_seqlen() == total


# ------------------------------------------------------------------------------------------------------------------------
# 2. decode equals the contiguous cache bit for bit (and, twice, the oracle)
# ------------------------------------------------------------------------------------------------------------------------
def _fill_both(dev, *, Hkv, D, page, dtype, lens, k_bits=8, seed=0, extra_pages=1, max_seqs=None, dense_cap=None, max_pages=None):
    """the same two ragged appends (a prefill, then the rest) into a contiguous and a paged cache"""
    import lowbit_quant_fa2_paddle_amd as lb
    B, T = len(lens), max(lens)
    gen = _gen(dev, seed)
    max_pages = max_pages or -(-T // page)
    dense = lb.LowbitKVCache(B, Hkv, D, dense_cap or T, TDT[dtype], dev, k_bits=k_bits)
    paged = _paged(dev, num_pages=B * max_pages + extra_pages, page=page, Hkv=Hkv, D=D, max_seqs=max_seqs or B, max_pages=max_pages,
                   dtype=dtype, k_bits=k_bits, seed=seed)
    k, v = _rand(gen, (B, Hkv, T, D), dtype, dev, bias=0.5), _rand(gen, (B, Hkv, T, D), dtype, dev)
    t0 = max(1, T // 2)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    slots = None if max_seqs is None else list(range(B))
    for cache, kw in ((dense, {}), (paged, dict(slots=slots))):
        cache.append(k[:, :, :t0], v[:, :, :t0], new_lens=torch.clamp(lt, max=t0), **kw)
        if T > t0:
            cache.append(k[:, :, t0:], v[:, :, t0:], new_lens=torch.clamp(lt - t0, min=0), **kw)
    assert torch.equal(paged.seqlens[:B], lt) and torch.equal(dense.seqlens, lt)
    return dense, paged, gen


DECODE_CASES = [
    dict(Sq=1, G=8, Hkv=2, D=128, page=64, dtype="fp16", lens=[0, 1, 63, 640, 333]),
    dict(Sq=4, G=4, Hkv=2, D=64, page=128, dtype="fp16", lens=[0, 1, 50, 128, 321]),
    dict(Sq=16, G=4, Hkv=1, D=128, page=192, dtype="fp16", lens=[130, 700]),   # 64 rows: the instance without look-ahead
    dict(Sq=16, G=4, Hkv=1, D=64, page=64, dtype="fp16", lens=[449, 2]),
    dict(Sq=1, G=4, Hkv=2, D=80, page=256, dtype="fp16", lens=[77, 300]),       # padded head dim
    dict(Sq=4, G=8, Hkv=1, D=128, page=64, dtype="bf16", lens=[257, 64]),
    dict(Sq=1, G=1, Hkv=2, D=64, page=64, dtype="fp16", lens=[192, 65], q_bits=4, k_bits=4),
    # the instances (dtype x head dim x 1 / 2 / 4 row blocks) the cases above leave out
    dict(Sq=8, G=4, Hkv=1, D=64, page=128, dtype="fp16", lens=[200, 65]),       # fp16, D 64, 2 row blocks
    dict(Sq=2, G=16, Hkv=1, D=128, page=64, dtype="fp16", lens=[129, 300]),     # fp16, D 128, 2 row blocks
    dict(Sq=1, G=8, Hkv=2, D=128, page=192, dtype="bf16", lens=[5, 450]),       # bf16, D 128, 1 row block
    dict(Sq=16, G=4, Hkv=1, D=128, page=64, dtype="bf16", lens=[321, 66]),      # bf16, D 128, 4 row blocks (no look-ahead)
    dict(Sq=16, G=4, Hkv=1, D=64, page=128, dtype="bf16", lens=[70, 260]),      # bf16, D 64, 4 row blocks
    dict(Sq=4, G=8, Hkv=1, D=64, page=64, dtype="bf16", lens=[258, 1]),         # bf16, D 64, 2 row blocks
    dict(Sq=1, G=2, Hkv=2, D=64, page=256, dtype="bf16", lens=[64, 257]),       # bf16, D 64, 1 row block
]
ORACLE_CASES = (0, 4, 5)  # checked against the oracle as well (5: Sq 4, so the causal mask is not trivial; bf16)


@pytest.mark.parametrize("idx", range(len(DECODE_CASES)), ids=lambda i: "Sq{Sq}G{G}D{D}p{page}{dtype}".format(**DECODE_CASES[i]))
def test_decode_equals_contiguous_bit_for_bit(oracle, dev, idx):
    import lowbit_quant_fa2_paddle_amd as lb
    case = dict(DECODE_CASES[idx])
    Sq, G, Hkv, D, dtype, lens = (case[x] for x in ("Sq", "G", "Hkv", "D", "dtype", "lens"))
    q_bits, k_bits = case.get("q_bits", 8), case.get("k_bits", 8)
    dense, paged, gen = _fill_both(dev, Hkv=Hkv, D=D, page=case["page"], dtype=dtype, lens=lens, k_bits=k_bits, seed=17 + idx)
    B, Hq = len(lens), G * Hkv
    q = _rand(gen, (B, Hq, Sq, D), dtype, dev)
    for b, n in enumerate(lens):
        _state_equal(paged, b, dense, b, n, f"sequence {b}")
    for layout in ("HND", "NHD"):
        tq = q if layout == "HND" else _nhd(q)
        for causal in (False, True):
            for ns in (1, 2, 7, 0):
                what = f"{case} {layout} causal={causal} splits={ns}"
                kw = dict(tensor_layout=layout, is_causal=causal, num_splits=ns, q_bits=q_bits)
                o_ref, lse_ref = lb.lowbit_fa_decode(tq, dense, return_lse=True, **kw)
                o, lse = lb.lowbit_fa_decode(tq, paged, return_lse=True, **kw)
                assert o.shape == tq.shape and o.dtype == tq.dtype and tuple(lse.shape) == (B, Hq, Sq), what
                assert not torch.isnan(o).any(), what + ": a row of another page or past the end was read"
                assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), what + ": O differs from the contiguous cache"
                assert torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32)), what + ": LSE differs"
                o2 = lb.lowbit_fa_decode(tq, paged, **kw)
                assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), what + ": O depends on return_lse"
    if idx not in ORACLE_CASES:
        return
    # the oracle's kernel on the state gathered through the table (tests/test_gpu_kvcache_decode.py does this for the contiguous cache)
    Dp, T, sm_scale = paged.padded_head_dim, max(lens), D ** -0.5
    npg = -(-T // case["page"]) * case["page"]
    k_i8 = np.zeros((B, Hkv, npg, Dp), np.int8)
    k_scale = np.zeros((B, Hkv, npg // 64), np.float32)
    v16 = np.zeros((B, Hkv, npg, Dp), np.float32)
    for b in range(B):
        c, s, v = paged.gather(b)
        k_i8[b], k_scale[b], v16[b] = c.cpu().numpy(), s.cpu().numpy(), v.float().cpu().numpy()
    qn = oracle.to_storage(q.float().cpu().numpy(), dtype)
    qp = np.pad(qn, [(0, 0)] * 3 + [(0, Dp - D)])
    q_i8, q_scale = kr.quant_q(oracle, qp, sm_scale, 127 if q_bits == 8 else 7)
    corr = kr.lse_correction(oracle, qp, paged.km.float().cpu().numpy(), dtype)
    for causal, ns in ((False, 0), (True, 2)):
        what = f"{case} vs oracle causal={causal} splits={ns}"
        o_ref, lse2_ref = kr.oracle_decode(oracle, q_i8, q_scale, k_i8, k_scale, v16, np.array(lens), causal=causal, out_dtype=dtype)
        o, lse = lb.lowbit_fa_decode(q, paged, is_causal=causal, return_lse=True, num_splits=ns, q_bits=q_bits)
        kr.check_o(o.float().cpu().numpy(), o_ref[..., :D], dtype, what)
        kr.check_lse(lse.cpu().numpy(), kr.natural_lse(lse2_ref, corr, sm_scale), corr, sm_scale, dtype, what)


# ------------------------------------------------------------------------------------------------------------------------
# 3. slots
# ------------------------------------------------------------------------------------------------------------------------
def test_slots_select_rows_and_leave_the_others_alone(dev):
    import lowbit_quant_fa2_paddle_amd as lb
    lens, Hkv, G, D, dtype = [100, 70, 300], 2, 4, 128, "fp16"
    dense, paged, gen = _fill_both(dev, Hkv=Hkv, D=D, page=128, dtype=dtype, lens=lens, seed=5, extra_pages=6, dense_cap=400, max_pages=4)
    q = _rand(gen, (3, G * Hkv, 2, D), dtype, dev)
    for ns in (1, 3):
        full, lse_full = lb.lowbit_fa_decode(q, paged, is_causal=True, return_lse=True, num_splits=ns)
        part, lse_part = lb.lowbit_fa_decode(q[[2, 0]], paged, is_causal=True, return_lse=True, num_splits=ns, slots=[2, 0])
        assert torch.equal(part.view(torch.int16), full[[2, 0]].view(torch.int16)), ns
        assert torch.equal(lse_part.view(torch.int32), lse_full[[2, 0]].view(torch.int32)), ns
    # an append to slot 1 alone: slots 0 and 2 keep state and results, slot 1 is what the contiguous cache holds after the same rows
    before = {s: [t.clone() for t in paged.gather(s)] for s in (0, 2)}
    free = paged.num_free_pages
    k1, v1 = _rand(gen, (1, Hkv, 90, D), dtype, dev, bias=0.5), _rand(gen, (1, Hkv, 90, D), dtype, dev)
    paged.append(k1, v1, slots=[1])
    assert paged.num_free_pages == free - 1  # slot 1's bound went from 300 to 390 rows: a fourth page of 128
    for s in (0, 2):
        for a, b_ in zip(before[s], paged.gather(s)):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), s
    after, lse_after = lb.lowbit_fa_decode(q, paged, is_causal=True, return_lse=True, num_splits=3)
    assert torch.equal(after[[0, 2]].view(torch.int16), full[[0, 2]].view(torch.int16))
    assert torch.equal(lse_after[[0, 2]].view(torch.int32), lse_full[[0, 2]].view(torch.int32))
    # slot 1 itself: what the contiguous cache holds after the same rows (its other sequences take none of them)
    dense.append(k1.expand(3, -1, -1, -1).contiguous(), v1.expand(3, -1, -1, -1).contiguous(),
                 new_lens=torch.tensor([0, 90, 0], dtype=torch.int32, device=dev))
    _state_equal(paged, 1, dense, 1, 160, "slot 1 after its own append")
    ref, lse_ref = lb.lowbit_fa_decode(q, dense, is_causal=True, return_lse=True, num_splits=3)
    # (the contiguous call sizes its grid for 390 keys, the paged one too: slot 1's bound)
    assert torch.equal(after.view(torch.int16), ref.view(torch.int16)) and torch.equal(lse_after.view(torch.int32), lse_ref.view(torch.int32))
    assert int(paged.seqlens[1]) == 160 and paged.seqlens.tolist() == [100, 160, 300]


# ------------------------------------------------------------------------------------------------------------------------
# 4. late join, free and reuse
# ------------------------------------------------------------------------------------------------------------------------
def test_late_join_free_and_reuse(dev):
    import lowbit_quant_fa2_paddle_amd as lb
    Hkv, G, D, dtype, page = 2, 4, 64, "bf16", 64
    gen = _gen(dev, 23)
    paged = _paged(dev, num_pages=8, page=page, Hkv=Hkv, D=D, max_seqs=3, max_pages=4, dtype=dtype, seed=4)
    mk = lambda n, T, bias: (_rand(gen, (n, Hkv, T, D), dtype, dev, bias=bias), _rand(gen, (n, Hkv, T, D), dtype, dev))
    q = _rand(gen, (3, G * Hkv, 1, D), dtype, dev)

    def twin(k, v):
        return lb.LowbitKVCache(1, Hkv, D, k.shape[2], TDT[dtype], dev).append(k, v)

    def same_as_twin(slot, k, v, what):
        t = twin(k, v)
        _state_equal(paged, slot, t, 0, k.shape[2], what)
        for ns in (1, 2):
            o_ref, lse_ref = lb.lowbit_fa_decode(q[slot:slot + 1], t, return_lse=True, num_splits=ns)
            o, lse = lb.lowbit_fa_decode(q[slot:slot + 1], paged, return_lse=True, num_splits=ns, slots=[slot])
            assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), what
            assert torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32)), what

    k01, v01 = mk(2, 150, 0.5)
    paged.append(k01, v01, slots=[0, 1])
    assert paged.num_free_pages == 8 - 3 - 3
    # a sequence joins while the others are mid-flight: its own mean, the state and results of a cache it has to itself
    k2, v2 = mk(1, 90, -1.0)
    paged.append(k2, v2, slots=[2])
    assert paged.num_free_pages == 0
    same_as_twin(2, k2, v2, "late join")
    same_as_twin(0, k01[:1], v01[:1], "slot 0 after the join")
    assert not torch.equal(paged.km[2], paged.km[0])
    # out of pages: refused before anything is launched, state intact
    o_before, lse_before = lb.lowbit_fa_decode(q, paged, return_lse=True, num_splits=2)
    table, lens = paged.block_table.clone(), paged.seqlens.clone()
    kx, vx = mk(1, 64, 0.5)
    with pytest.raises(RuntimeError, match="out of pages"):
        paged.append(kx, vx, slots=[0])  # 150 + 64 rows need a fourth page
    assert paged.num_free_pages == 0 and paged.allocator.bound == [150, 150, 90]
    assert torch.equal(paged.block_table, table) and torch.equal(paged.seqlens, lens)
    o_after, lse_after = lb.lowbit_fa_decode(q, paged, return_lse=True, num_splits=2)
    assert torch.equal(o_after.view(torch.int16), o_before.view(torch.int16)) and torch.equal(lse_after.view(torch.int32), lse_before.view(torch.int32))
    # free slot 1, start a shorter sequence there: it gets the freed pages, none of the old keys, and a mean of its own
    held = list(paged.allocator.pages[1])
    others = {s: [t.clone() for t in paged.gather(s)] for s in (0, 2)}
    paged.free(1)
    assert paged.num_free_pages == 3 and int(paged.seqlens[1]) == 0 and paged.allocator.bound[1] == 0
    o_empty, lse_empty = lb.lowbit_fa_decode(q[1:2], paged, return_lse=True, slots=[1])
    assert torch.all(o_empty == 0) and torch.all(torch.isinf(lse_empty) & (lse_empty < 0))
    k1, v1 = mk(1, 130, 2.0)
    paged.append(k1, v1, slots=[1])
    assert paged.allocator.pages[1] == held and paged.num_free_pages == 0
    same_as_twin(1, k1, v1, "reused slot")
    for s in (0, 2):
        for a, b_ in zip(others[s], paged.gather(s)):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), s
    o_end, lse_end = lb.lowbit_fa_decode(q, paged, return_lse=True, num_splits=2)
    assert torch.equal(o_end[[0, 2]].view(torch.int16), o_before[[0, 2]].view(torch.int16))
    assert torch.equal(lse_end[[0, 2]].view(torch.int32), lse_before[[0, 2]].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# 5. long and large
# ------------------------------------------------------------------------------------------------------------------------
def test_long_context_through_2048_scrambled_pages(dev):
    """131072 keys at page 64: 2048 pages in permuted order, 256 chosen slices and one"""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    T, D, G, dtype = 131072, 128, 8, "fp16"
    assert _lib.load().lbfa_decode_num_splits(1, 1, T) == 256
    gen = _gen(dev, 5)
    k, v = _rand(gen, (1, 1, T, D), dtype, dev, bias=0.5), _rand(gen, (1, 1, T, D), dtype, dev)
    q = _rand(gen, (1, G, 1, D), dtype, dev)
    dense = lb.LowbitKVCache(1, 1, D, T, TDT[dtype], dev).append(k, v)
    paged = _paged(dev, num_pages=2048 + 5, page=64, Hkv=1, D=D, max_seqs=1, max_pages=2048, dtype=dtype, seed=9).append(k, v)
    assert paged.num_free_pages == 5
    _state_equal(paged, 0, dense, 0, T, "131072 keys")
    for ns in (0, 1):
        o_ref, lse_ref = lb.lowbit_fa_decode(q, dense, return_lse=True, num_splits=ns)
        o, lse = lb.lowbit_fa_decode(q, paged, return_lse=True, num_splits=ns)
        assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), ns
        assert torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32)), ns


def test_page_offsets_are_formed_in_64_bits(dev):
    """a pool whose V tensor exceeds 2^32 bytes, pages handed out from the top: the short sequence lives past byte 2^32 of V
    and past byte 2^31 of the codes"""
    import lowbit_quant_fa2_paddle_amd as lb
    page, D, Hkv, G, dtype, n = 1024, 128, 1, 4, "fp16", 1100
    num_pages = (1 << 32) // (page * D * 2) + 2
    paged = _paged(dev, num_pages=num_pages, page=page, Hkv=Hkv, D=D, max_seqs=1, max_pages=2, dtype=dtype,
                   order=list(range(num_pages - 1, -1, -1)))
    assert paged.v.numel() * paged.v.element_size() > 1 << 32
    gen = _gen(dev, 31)
    k, v = _rand(gen, (1, Hkv, n, D), dtype, dev, bias=0.5), _rand(gen, (1, Hkv, n, D), dtype, dev)
    q = _rand(gen, (1, G * Hkv, 2, D), dtype, dev)
    dense = lb.LowbitKVCache(1, Hkv, D, n, TDT[dtype], dev).append(k, v)
    paged.append(k, v)
    assert paged.allocator.pages[0] == [num_pages - 1, num_pages - 2]
    assert (num_pages - 2) * page * D * 2 >= 1 << 32
    _state_equal(paged, 0, dense, 0, n, "top of a 4 GiB pool")
    assert torch.all(paged.k_codes[0] == 127) and torch.all(paged.k_codes[num_pages - 3] == 127)  # nothing landed at a wrapped offset
    q130 = _rand(gen, (1, G * Hkv, 130, D), dtype, dev)  # and a prefill read next to the decode read: two Q blocks
    for ns in (1, 3):
        o_ref, lse_ref = lb.lowbit_fa_decode(q, dense, is_causal=True, return_lse=True, num_splits=ns)
        o, lse = lb.lowbit_fa_decode(q, paged, is_causal=True, return_lse=True, num_splits=ns)
        assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), ns
        assert torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32)), ns
        o_ref, lse_ref = lb.lowbit_fa_prefill(q130, dense, is_causal=True, return_lse=True, num_splits=ns)
        o, lse = lb.lowbit_fa_prefill(q130, paged, is_causal=True, return_lse=True, num_splits=ns)
        assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), ("prefill", ns)
        assert torch.equal(lse.view(torch.int32), lse_ref.view(torch.int32)), ("prefill", ns)
    del paged
    torch.cuda.empty_cache()
