"""GPU tests of cached prefill (`lowbit_fa_prefill`, lbfa_prefill / lbfa_prefill_paged): attention of any number of queries to the
int8 KV cache.

* every element of O and of the LSE against `oracle_prefill` (tests/prefill_reference.py: the oracle's int8 / fp16 kernel on the
  numpy cache) within the operator bound of tests/test_gpu_parity.py, on the cases of `prefill_reference.CASES` at their slice
  counts; rows at or past q_lens are exactly 0 and -inf;
* bit for bit: a second run, O with and without the LSE, a strided q, the paged cache (page sizes 64 and 128, scrambled pages, a
  pool full of garbage, a `slots` permutation) against the contiguous one;
* chunked == one-shot, bit for bit with one slice;
* the golden fixtures of the reference's kernels, through a cache filled by one append;
* at M <= 64 prefill and decode both meet the bound of the same oracle output, and - non-causal, the same explicit num_splits -
  equal each other bit for bit.
"""
import numpy as np
import pytest

import kvcache_reference as kr
import prefill_reference as pr
from conftest import golden_inputs, golden_names, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
B, HQ, HKV = pr.B, pr.HQ, pr.HKV  # the common shape: a case that names its own is read through `pr.shape_of`


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from lowbit_quant_fa2_paddle_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dtype]).to(dev)


def _np(t):
    return t.detach().float().cpu().numpy()


def _nhd(t):
    return t.transpose(1, 2).contiguous()


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _same(a, b, what):
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.shape == y.shape and x.dtype == y.dtype, what
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {int((_bits(x) != _bits(y)).sum())} bytes differ"


def _fill(cache, c, case, dev, **kw):
    """the appends of the case (`steps` of prefill_reference.build_case) into a cache"""
    dtype = case["dtype"]
    for a, e, nl in c["steps"]:
        cache.append(_t(c["k"][:, :, a:e], dtype, dev), _t(c["v"][:, :, a:e], dtype, dev),
                     new_lens=torch.tensor(nl, dtype=torch.int32, device=dev), **kw)
    return cache


def _contiguous(c, case, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    B, HQ, HKV = pr.shape_of(case)
    cache = lb.LowbitKVCache(B, HKV, case["D"], c["cap"], TDT[case["dtype"]], dev, k_bits=case.get("k_bits", 8),
                             smooth_k=case.get("smooth_k", True))
    return _fill(cache, c, case, dev)


def _paged(c, case, dev, page, slots):
    """a pool full of garbage whose pages come in a scrambled order; sequence b lives in slot slots[b]"""
    import lowbit_quant_fa2_paddle_amd as lb
    B, HQ, HKV = pr.shape_of(case)
    max_pages = -(-c["cap"] // page)
    num_pages = 3 * max_pages + 2
    order = np.random.default_rng(page + case["Sq"]).permutation(num_pages).tolist()
    cache = lb.LowbitPagedKVCache(num_pages, page, HKV, case["D"], 3, max_pages, TDT[case["dtype"]], dev,
                                  k_bits=case.get("k_bits", 8), smooth_k=case.get("smooth_k", True), page_order=order)
    cache.k_codes.fill_(-128)
    cache.k_scale.fill_(float("inf"))
    cache.v.fill_(float("nan"))
    return _fill(cache, c, case, dev, slots=slots)


def _kw(case, c):
    kw = dict(tensor_layout=case["layout"], q_bits=case.get("q_bits", 8))
    if "sm_scale" in case:
        kw["sm_scale"] = case["sm_scale"]
    if "q_lens" in case:
        kw["q_lens"] = torch.tensor(case["q_lens"], dtype=torch.int32)
    return kw


def _state_is_the_reference(cache, ref, what):
    codes, scales, v = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy(), _np(cache.v)
    assert np.array_equal(cache.seqlens.cpu().numpy(), ref.seqlens), what
    for b, n in enumerate(int(x) for x in ref.seqlens):
        nb = (n + 63) // 64
        assert np.array_equal(codes[b, :, :n], ref.k_codes[b, :, :n]), (what, b, "codes")
        assert np.array_equal(scales[b, :, :nb].view(np.uint32), ref.k_scale[b, :, :nb].view(np.uint32)), (what, b, "scales")
        assert np.array_equal(v[b, :, :n], ref.v[b, :, :n]), (what, b, "v")


# ------------------------------------------------------------------------------------------------------------------------
# 1. every element against the oracle; the bit-for-bit properties of one cache
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_prefill_equals_oracle(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    B, HQ, HKV = pr.shape_of(case)
    c = pr.build_case(oracle, case)
    Sq, D, dtype, layout = case["Sq"], case["D"], case["dtype"], case["layout"]
    cache = _contiguous(c, case, dev)
    _state_is_the_reference(cache, c["ref"], pr.case_id(case))
    tq = _t(c["q"], dtype, dev)
    if layout == "NHD":
        tq = _nhd(tq)
    kw = _kw(case, c)
    for causal in (False, True):
        o_ref, lse_ref = c["oracle"][causal]
        for ns in c["splits"]:
            what = f"{pr.case_id(case)} causal={causal} splits={ns}"
            o, lse = lb.lowbit_fa_prefill(tq, cache, is_causal=causal, return_lse=True, num_splits=ns, **kw)
            assert o.shape == tq.shape and o.dtype == tq.dtype and tuple(lse.shape) == (B, HQ, Sq), what
            on, ln = _np(o if layout == "HND" else o.transpose(1, 2)), lse.cpu().numpy()
            kr.check_o(on, o_ref[..., :D], dtype, what)
            kr.check_lse(ln, lse_ref, c["corr"], c["sm_scale"], dtype, what)
            dead = np.isinf(lse_ref)
            assert np.all(on[dead] == 0), what  # no visible key: zeros
            for b in range(B):  # rows at or past q_lens: exactly 0 and -inf
                assert np.all(on[b, :, c["q_lens"][b]:] == 0) and np.all(np.isneginf(ln[b, :, c["q_lens"][b]:])), what
            _same((o, lse), lb.lowbit_fa_prefill(tq, cache, is_causal=causal, return_lse=True, num_splits=ns, **kw),
                  what + ": two runs differ")
            _same(o, lb.lowbit_fa_prefill(tq, cache, is_causal=causal, num_splits=ns, **kw), what + ": O depends on return_lse")


@pytest.mark.parametrize("idx,page,slots", [(4, 64, [2, 0]), (5, 128, [1, 2]), (8, 64, [0, 2]), (10, 128, [2, 1]), (11, 64, [1, 0]),
                                            (12, 128, [0, 1]), (13, 64, [2, 1]), (3, 128, [1, 0])])
def test_paged_equals_contiguous_bit_for_bit(oracle, dev, idx, page, slots):
    import lowbit_quant_fa2_paddle_amd as lb
    case = pr.CASES[idx]
    c = pr.build_case(oracle, case)
    dtype, layout = case["dtype"], case["layout"]
    dense, paged = _contiguous(c, case, dev), _paged(c, case, dev, page, slots)
    tq = _t(c["q"], dtype, dev)
    if layout == "NHD":
        tq = _nhd(tq)
    kw = _kw(case, c)
    for causal in (False, True):
        for ns in pr.SPLITS:
            what = f"{pr.case_id(case)} page={page} slots={slots} causal={causal} splits={ns}"
            want = lb.lowbit_fa_prefill(tq, dense, is_causal=causal, return_lse=True, num_splits=ns, **kw)
            got = lb.lowbit_fa_prefill(tq, paged, is_causal=causal, return_lse=True, num_splits=ns, slots=slots, **kw)
            assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), what + ": garbage of the pool was read"
            _same(got, want, what)


@pytest.mark.parametrize("idx", [4, 10])
def test_strided_q_equals_contiguous_q(oracle, dev, idx):
    import lowbit_quant_fa2_paddle_amd as lb
    case = pr.CASES[idx]
    B, HQ, HKV = pr.shape_of(case)
    c = pr.build_case(oracle, case)
    cache = _contiguous(c, case, dev)
    tq = _t(c["q"], case["dtype"], dev)
    big = torch.full((B, HQ + 1, case["Sq"] + 3, 2 * case["D"]), float("nan"), dtype=tq.dtype, device=dev)
    view = big[:, 1:, 2:-1, :case["D"]]
    view.copy_(tq)
    assert not view.is_contiguous() and view.stride(-1) == 1
    for causal, ns in ((False, 1), (True, 2), (True, 0)):
        want = lb.lowbit_fa_prefill(tq, cache, is_causal=causal, return_lse=True, num_splits=ns)
        _same(lb.lowbit_fa_prefill(view, cache, is_causal=causal, return_lse=True, num_splits=ns), want, f"strided q, splits={ns}")


# ------------------------------------------------------------------------------------------------------------------------
# 2. chunked == one-shot
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,paged", [("fp16", 64, False), ("bf16", 128, False), ("fp16", 128, True)])
def test_chunked_prefill_equals_one_shot_bit_for_bit(oracle, dev, dtype, D, paged):
    """384 keys in three chunks of 128, the operator called causally after each append; then once with all 384 queries on the
    final cache.  The blocks are complete at every step, so the codes, km, Q blocks and visible tiles are the same: the same rows
    must be equal bit for bit (one slice).  km is fixed by the first append in both runs - it is one cache."""
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(D)
    mk = lambda h, bias: _t(oracle.to_storage(rng.standard_normal((B, h, 384, D), dtype=np.float32) + np.float32(bias), dtype), dtype, dev)
    q, k, v = mk(HQ, 0.0), mk(HKV, 0.5), mk(HKV, 0.0)
    if paged:
        cache = lb.LowbitPagedKVCache(8, 128, HKV, D, B, 3, TDT[dtype], dev, page_order=[5, 2, 7, 0, 3, 6, 1, 4])
    else:
        cache = lb.LowbitKVCache(B, HKV, D, 384, TDT[dtype], dev)
    chunks = []
    for i in range(3):
        sl = slice(128 * i, 128 * i + 128)
        cache.append(k[:, :, sl], v[:, :, sl])
        chunks.append(lb.lowbit_fa_prefill(q[:, :, sl], cache, is_causal=True, return_lse=True, num_splits=1))
    o, lse = lb.lowbit_fa_prefill(q, cache, is_causal=True, return_lse=True, num_splits=1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    for i, (oc, lc) in enumerate(chunks):
        _same((oc, lc), (o[:, :, 128 * i:128 * i + 128], lse[:, :, 128 * i:128 * i + 128]), f"chunk {i}")


# ------------------------------------------------------------------------------------------------------------------------
# 3. the golden fixtures of the reference's kernels, through the cache
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_prefill_vs_reference_golden(oracle, dev, name):
    """One uniform append of the fixture's k, v, then the operator on its q: the Q and K codes are the dense operator's, and the
    output meets the fixture's `o` as tests/test_gpu_parity.py asks of the dense operator - |dO| <= 2e-3 + 2e-3 |O| (+ 2^-7 |O|
    for bf16) on every element."""
    import lowbit_quant_fa2_paddle_amd as lb
    p, g = load_golden(name)
    q, k, v = golden_inputs(oracle, p)
    dtype, layout = p["dtype"], p["layout"]
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    cache = lb.LowbitKVCache(p["B"], p["Hkv"], p["D"], p["Sk"], TDT[dtype], dev, k_bits=8 if p["k_qmax"] == 127 else 4,
                             smooth_k=p["smooth_k"])
    cache.append(tk, tv, tensor_layout=layout)
    for ns in (0, 1, 3):
        o = lb.lowbit_fa_prefill(tq, cache, tensor_layout=layout, is_causal=p["causal"], q_bits=8 if p["q_qmax"] == 127 else 4,
                                 num_splits=ns)
        kr.check_o(_np(o), g["o"], dtype, f"{name} splits={ns}")


# ------------------------------------------------------------------------------------------------------------------------
# 4. M <= 64: prefill and decode, the same oracle output
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.SHORT_CASES, ids=pr.case_id)
def test_short_queries_prefill_and_decode_meet_the_same_oracle(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    B, HQ, HKV = pr.shape_of(case)
    c = pr.build_case(oracle, case)
    Sq, D, dtype, layout = case["Sq"], case["D"], case["dtype"], case["layout"]
    assert Sq * (HQ // HKV) <= 64
    cache = _contiguous(c, case, dev)
    tq = _t(c["q"], dtype, dev)
    if layout == "NHD":
        tq = _nhd(tq)
    for causal in (False, True):
        o_ref, lse_ref = c["oracle"][causal]
        for ns in (0, 1, 3):
            for fn in (lb.lowbit_fa_prefill, lb.lowbit_fa_decode):
                what = f"{fn.__name__} {pr.case_id(case)} causal={causal} splits={ns}"
                o, lse = fn(tq, cache, tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns)
                kr.check_o(_np(o if layout == "HND" else o.transpose(1, 2)), o_ref[..., :D], dtype, what)
                kr.check_lse(lse.cpu().numpy(), lse_ref, c["corr"], c["sm_scale"], dtype, what)


@pytest.mark.parametrize("v_bits", [16, 8])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_short_queries_prefill_equals_decode_bit_for_bit(oracle, dev, D, dtype, v_bits):
    """Where both operators take the call - non-causal, M = Sq * G <= 64, q_lens full - they are the same computation: one Q block
    per query head with the same amax, the tile arithmetic both kernels take from one text (csrc/attn_cache_tile.inc), and, for the
    same explicit num_splits, the same slices of the same four tiles (n = 200: the last one ragged; with 3 slices the third is
    empty) added by the same combine kernel.  Sq 1 / 16 / 32 at G = 2 are the three row-block counts of decode (M = 2, 32, 64)."""
    import lowbit_quant_fa2_paddle_amd as lb
    hkv, grp, n = 2, 2, 200
    rng = np.random.default_rng(1000 * D + v_bits)
    mk = lambda h, rows, bias: _t(oracle.to_storage(rng.standard_normal((B, h, rows, D), dtype=np.float32) + np.float32(bias), dtype),
                                  dtype, dev)
    cache = lb.LowbitKVCache(B, hkv, D, 256, TDT[dtype], dev, v_bits=v_bits).append(mk(hkv, n, 0.5), mk(hkv, n, 0.0))
    for Sq in (1, 16, 32):
        q = mk(hkv * grp, Sq, 0.0)
        for ns in (1, 3):
            what = f"D={D} {dtype} v_bits={v_bits} Sq={Sq} splits={ns}"
            o, lse = lb.lowbit_fa_prefill(q, cache, return_lse=True, num_splits=ns)
            od, ld = lb.lowbit_fa_decode(q, cache, return_lse=True, num_splits=ns)
            assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), what
            for name, x, y in (("O", o, od), ("LSE", lse, ld)):
                bad = torch.nonzero(x != y)
                assert torch.equal(x, y), f"{what}: {name} differs in {len(bad)} elements, the first at {bad[0].tolist()}"


def test_front_end_refusals(dev):
    import lowbit_quant_fa2_paddle_amd as lb
    cache = lb.LowbitKVCache(1, 1, 64, 64, torch.float16, dev)
    kv = torch.zeros(1, 1, 8, 64, dtype=torch.float16, device=dev)
    cache.append(kv, kv)
    q = torch.zeros(1, 5, 130, 64, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="the limit is 64"):  # decode keeps refusing what prefill takes
        lb.lowbit_fa_decode(q, cache)
    o, lse = lb.sageattn_prefill(q, cache, return_lse=True)
    assert o.shape == q.shape and tuple(lse.shape) == (1, 5, 130) and not o.any()  # V is zero
    with pytest.raises(RuntimeError, match="forward-only"):
        lb.lowbit_fa_prefill(q.clone().requires_grad_(), cache)
    with pytest.raises(ValueError, match="q_lens must have one entry per row of q"):
        lb.lowbit_fa_prefill(q, cache, q_lens=torch.tensor([1, 2], dtype=torch.int32))
    assert torch.equal(lb.lowbit_fa_prefill(q, cache, q_lens=[7]), lb.lowbit_fa_prefill(q, cache, q_lens=torch.tensor([7], dtype=torch.int32)))
    assert torch.equal(lb.lowbit_fa_prefill(q, cache, q_lens=np.array([7])), lb.lowbit_fa_prefill(q, cache, q_lens=[7]))
    with pytest.raises(TypeError, match="q_lens must be an integer tensor or sequence"):
        lb.lowbit_fa_prefill(q, cache, q_lens="seven")
    with pytest.raises(ValueError, match="slots address the sequences of a LowbitPagedKVCache"):
        lb.lowbit_fa_prefill(q, cache, slots=[0])
    assert lb.lowbit_fa_prefill(q[:, :, :0], cache).shape == (1, 5, 0, 64)
