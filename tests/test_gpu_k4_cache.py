"""GPU tests of the nibble-packed int4 K cache (`k_packed=True` of `LowbitKVCache` / `LowbitPagedKVCache`; lbfa_*_k4[_v8]): the
+-7 codes of `k_bits=4` two to a byte.  The yardstick is the byte-per-code `k_bits=4` cache given the same appends: an integer
score does not depend on the order of its channels, so everything is `torch.equal`, with no tolerance.

1. state: after every append of a ragged schedule `unpacked_k_codes()`, k_scale, k_tail, km, v / v_scale and seqlens equal the byte
   cache's, the packed bytes equal the numpy packer (tests/k4_reference.py) of its codes, the paged cache agrees through `gather`;
2. all 225 (low, high) nibble pairs in one pinned 64-key block whose scale is 1: the state is K itself, decode is the byte cache's;
3. decode and cached prefill, differential: every kernel instance, lengths 0 .. 333, 1 / 2 / 7 / chosen slices, causal or not, HND
   and NHD, q_bits 8 and 4, v_bits 16 and 8, contiguous and paged;
4. one decode and one prefill against the oracle's kernel on the unpacked numpy state, within the unchanged `check_o` / `check_lse`;
5. hostile memory: rows at or past the length and unused pages hold 0x88 (the code pair the quantiser never writes) or random
   bytes, scales there are NaN / inf;
6. containment: guard bands around `k_codes`, rows outside [s0, end) keep their bytes, the siblings' device-side defences.
Shapes stay at B <= 5, Hkv <= 3 and at most 700 keys.
"""
import numpy as np
import pytest

import k4_reference as k4
import kvcache_reference as kr
import prefill_reference as pr
from guarded import GuardArena

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LENS_A, LENS_B = [0, 1, 63, 64, 333], [65, 130, 333, 0, 64]  # together: 0, 1, 63, 64, 65, 130, 333


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


def _rand(orc, rng, shape, dtype, bias=0.0, mul=1.0):
    return orc.to_storage(rng.standard_normal(shape, dtype=np.float32) * np.float32(mul) + np.float32(bias), dtype)


def _nhd(t):
    return t.transpose(1, 2).contiguous()


def _padded(D):
    return 64 if D <= 64 else 128


def _pad(a, D):
    return np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, _padded(D) - D)])


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def same_bits(a, b, what):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), f"{what}: tensor {i} differs"


def _fill(cache, k, v, lens, dtype, dev):
    """two ragged appends (half the rows, then the rest) that leave the lengths `lens`"""
    lens, T = np.asarray(lens), k.shape[2]
    t0 = max(1, T // 2)
    tk, tv = _t(k, dtype, dev), _t(v, dtype, dev)
    cache.append(tk[:, :, :t0], tv[:, :, :t0], new_lens=torch.tensor(np.minimum(lens, t0), dtype=torch.int32, device=dev))
    if T > t0:
        cache.append(_nhd(tk[:, :, t0:]), _nhd(tv[:, :, t0:]), tensor_layout="NHD",
                     new_lens=torch.tensor(np.maximum(lens - t0, 0), dtype=torch.int32, device=dev))
    assert cache.seqlens.tolist() == lens.tolist()
    return cache


def _same_kv(orc, B, Hkv, D, dtype, lens, seed):
    rng = np.random.default_rng(seed)
    T = max(lens)
    return _rand(orc, rng, (B, Hkv, T, D), dtype, bias=0.5), _rand(orc, rng, (B, Hkv, T, D), dtype, mul=2.0), rng


def _trio(lb, orc, dev, *, B, Hkv, D, dtype, lens, page, seed, v_bits=16, garbage=None):
    """the three caches of a differential test, filled with the same appends: contiguous packed, contiguous byte-per-code
    (`k_bits=4`), paged packed (scrambled pages, spare pages in the pool).  `garbage`: a function applied to each fresh packed cache."""
    k, v, rng = _same_kv(orc, B, Hkv, D, dtype, lens, seed)
    T = max(lens)
    max_pages = -(-T // page)
    order = np.random.default_rng(seed + page).permutation(B * max_pages + 2).tolist()
    kw = dict(k_bits=4, v_bits=v_bits)
    c4 = lb.LowbitKVCache(B, Hkv, D, T, TDT[dtype], dev, k_packed=True, **kw)
    p4 = lb.LowbitPagedKVCache(B * max_pages + 2, page, Hkv, D, B, max_pages, TDT[dtype], dev, page_order=order, k_packed=True, **kw)
    if garbage is not None:
        garbage(c4), garbage(p4)
    c4, p4 = _fill(c4, k, v, lens, dtype, dev), _fill(p4, k, v, lens, dtype, dev)
    cb = _fill(lb.LowbitKVCache(B, Hkv, D, T, TDT[dtype], dev, **kw), k, v, lens, dtype, dev)
    return c4, cb, p4, rng


# ------------------------------------------------------------------------------------------------------------------------
# 1. state
# ------------------------------------------------------------------------------------------------------------------------
STEPS = [(70, None), (1, [1, 1, 0]), (1, [1, 0, 1]), (63, [63, 10, 0]), (64, [64, 64, 33]), (65, [0, 65, 64]), (200, [200, 1, 150])]
K_STATE = ("k_scale", "k_tail", "km", "seqlens")


@pytest.mark.parametrize("dtype,D,v_bits", [("fp16", 64, 16), ("bf16", 128, 8), ("fp16", 80, 16)])
def test_state_equals_the_byte_cache_after_every_append(oracle, dev, dtype, D, v_bits):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(29 + D)
    B, H, Dp, total = 3, 2, _padded(D), sum(T for T, _ in STEPS)
    kw = dict(k_bits=4, v_bits=v_bits)
    c4 = lb.LowbitKVCache(B, H, D, 600, TDT[dtype], dev, k_packed=True, **kw)
    cb = lb.LowbitKVCache(B, H, D, 600, TDT[dtype], dev, **kw)
    assert c4.k_packed and not cb.k_packed and c4.k_qmax == 7
    assert c4.k_codes.dtype == torch.uint8 and tuple(c4.k_codes.shape) == (B, H, 640, Dp // 2)
    assert cb.k_codes.dtype == torch.int8 and tuple(cb.k_codes.shape) == (B, H, 640, Dp)
    paged = []
    for page in (64, 192):
        # exactly the pages the schedule reserves: the page(s) a freed slot gives back are handed out again
        n_pages = B * -(-total // page)
        order = np.random.default_rng(page).permutation(n_pages).tolist()
        p = lb.LowbitPagedKVCache(n_pages, page, H, D, B, -(-640 // page), TDT[dtype], dev, page_order=order, k_packed=True, **kw)
        assert p.k_codes.dtype == torch.uint8 and tuple(p.k_codes.shape) == (n_pages, H, page, Dp // 2)
        junk = _t(_rand(oracle, rng, (1, H, 100, D), dtype, mul=50.0), dtype, dev)
        p.append(junk, junk, slots=[1])  # one slot filled, freed and reused: stale bytes in the pages it gets
        p.free(1)
        assert p.num_free_pages == n_pages and p.k_codes.any()
        paged.append(p)
    for step, (T, lens) in enumerate(STEPS):
        k = _rand(oracle, rng, (B, H, T, D), dtype, bias=0.5)
        v = _rand(oracle, rng, (B, H, T, D), dtype, mul=float(rng.choice([1e-3, 1.0, 40.0])))
        tk, tv = _t(k, dtype, dev), _t(v, dtype, dev)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        for cache in [c4, cb] + paged:
            if step % 2:
                cache.append(_nhd(tk), _nhd(tv), tensor_layout="NHD", new_lens=tl)
            else:
                cache.append(tk, tv, new_lens=tl)
        what = f"{dtype} D={D} step {step}"
        # the whole tensors: both caches started as zeros and an append writes the same rows of both
        codes = cb.k_codes.cpu().numpy()
        assert codes.min() >= -7 and codes.max() <= 7, what
        assert torch.equal(c4.unpacked_k_codes(), cb.k_codes), (what, "unpacked_k_codes")
        assert np.array_equal(c4.k_codes.cpu().numpy(), k4.pack(codes)), (what, "the packed bytes are not the numpy packer's")
        for name in K_STATE + (("v", "v_scale") if v_bits == 8 else ("v",)):
            same_bits(getattr(c4, name), getattr(cb, name), f"{what}: {name}")
        for p in paged:
            assert torch.equal(p.seqlens, c4.seqlens), what
            for b, n in enumerate(c4.seqlens.tolist()):
                got = p.gather(b)
                w = f"{what} page {p.page_size} sequence {b}"
                assert got[0].dtype == torch.uint8 and got[0].shape[-1] == Dp // 2, w
                same_bits(got[0][:, :n], c4.k_codes[b, :, :n], w + ": packed codes")
                same_bits(got[1][:, :(n + 63) // 64], c4.k_scale[b, :, :(n + 63) // 64], w + ": k scales")
                same_bits(got[2][:, :n], c4.v[b, :, :n], w + ": v")
                if v_bits == 8:
                    same_bits(got[3][:, :n], c4.v_scale[b, :, :n], w + ": v scales")
            same_bits(p.km, c4.km, what + ": km")
    # the debugging aids understand the format
    assert torch.equal(c4.dequantized_k(), cb.dequantized_k()) and tuple(c4.dequantized_k().shape) == (B, H, 640, D)
    assert tuple(paged[0].unpacked_k_codes().shape) == (paged[0].num_pages, H, 64, Dp)


# ------------------------------------------------------------------------------------------------------------------------
# 2. every pair of nibbles
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_all_225_nibble_pairs(oracle, dev, dtype, D):
    """one 64-key block, smooth_k=False, K integers in -7 .. 7 with a 7 among them: scale = 7 / 7 = 1 and the codes are K.  Pair
    p of the block (row-major, D / 2 pairs a row) is (low, high) = (p // 15 % 15 - 7, p % 15 - 7): all 225 of them."""
    import lowbit_quant_fa2_paddle_amd as lb
    pairs = np.arange(64 * D // 2)
    K = np.empty((1, 1, 64, D), np.float32)
    K[0, 0, :, 0::2] = (pairs // 15 % 15 - 7).reshape(64, D // 2)
    K[0, 0, :, 1::2] = (pairs % 15 - 7).reshape(64, D // 2)
    seen = {(int(a), int(b)) for a, b in zip(K[0, 0, :, 0::2].ravel(), K[0, 0, :, 1::2].ravel())}
    assert len(seen) == 225 and K.max() == 7 and K.min() == -7
    rng = np.random.default_rng(3)
    V = _rand(oracle, rng, (1, 1, 64, D), dtype)
    kw = dict(k_bits=4, smooth_k=False)
    c4 = lb.LowbitKVCache(1, 1, D, 64, TDT[dtype], dev, k_packed=True, **kw).append(_t(K, dtype, dev), _t(V, dtype, dev))
    cb = lb.LowbitKVCache(1, 1, D, 64, TDT[dtype], dev, **kw).append(_t(K, dtype, dev), _t(V, dtype, dev))
    assert torch.all(c4.k_scale == 1.0) and torch.all(cb.k_scale == 1.0)
    assert np.array_equal(c4.unpacked_k_codes().cpu().numpy(), K.astype(np.int8))
    assert np.array_equal(c4.k_codes.cpu().numpy(), k4.pack(K.astype(np.int8)))
    assert np.array_equal(k4.unpack(c4.k_codes.cpu().numpy()), K.astype(np.int8))
    for Sq, G in ((1, 1), (16, 4)):
        tq = _t(_rand(oracle, rng, (1, G, Sq, D), dtype, mul=2.0), dtype, dev)
        for q_bits in (8, 4):
            for causal in (False, True):
                kwd = dict(is_causal=causal, return_lse=True, q_bits=q_bits, num_splits=1)
                same_bits(lb.lowbit_fa_decode(tq, c4, **kwd), lb.lowbit_fa_decode(tq, cb, **kwd), f"nibble pairs Sq={Sq} q_bits={q_bits}")


# ------------------------------------------------------------------------------------------------------------------------
# 3. decode and cached prefill against the byte cache
# ------------------------------------------------------------------------------------------------------------------------
# every kernel instance: 2 dtypes x 2 head dims x (1, 2, 4 row blocks: M = 8, 32, 64) x (fp16, fp8 V), and a padded head dim
DECODE_CASES = [dict(dtype=dt, D=D, Sq=Sq, G=G, Hkv=2 if (D + Sq) % 3 else 3, lens=LENS_A if i % 2 == 0 else LENS_B)
                for i, (dt, D, (Sq, G)) in enumerate((dt, D, sg) for dt in ("fp16", "bf16") for D in (64, 128)
                                                     for sg in ((1, 8), (4, 8), (16, 4)))]
DECODE_CASES.append(dict(dtype="fp16", D=80, Sq=2, G=4, Hkv=2, lens=LENS_B))


def _case_id(c):
    return f"{c['dtype']}D{c['D']}Sq{c['Sq']}G{c['G']}Hkv{c['Hkv']}n{'_'.join(map(str, c['lens']))}"


@pytest.mark.parametrize("case", DECODE_CASES, ids=_case_id)
def test_decode_equals_the_byte_cache(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    dtype, D, Sq, G, Hkv, lens = (case[k] for k in ("dtype", "D", "Sq", "G", "Hkv", "lens"))
    B = len(lens)
    for v_bits in (16, 8):
        c4, cb, p4, rng = _trio(lb, oracle, dev, B=B, Hkv=Hkv, D=D, dtype=dtype, lens=lens, page=128, seed=33 + D + Sq, v_bits=v_bits)
        tq = _t(_rand(oracle, rng, (B, G * Hkv, Sq, D), dtype), dtype, dev)
        for causal in (False, True):
            for i, ns in enumerate((1, 2, 7, 0)):
                layout, q_bits = ("HND", "NHD")[(i + causal) % 2], (8, 4)[i // 2 ^ causal]  # all four pairs, per mask
                q = tq if layout == "HND" else _nhd(tq)
                kw = dict(is_causal=causal, return_lse=True, num_splits=ns, tensor_layout=layout, q_bits=q_bits)
                what = f"{_case_id(case)} v_bits={v_bits} causal={causal} splits={ns} {layout} q_bits={q_bits}"
                got = lb.lowbit_fa_decode(q, c4, **kw)
                same_bits(got, lb.lowbit_fa_decode(q, cb, **kw), what + " contiguous")
                same_bits(lb.lowbit_fa_decode(q, p4, **kw), got, what + " paged")
                assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), what


PREFILL_CASES = [dict(dtype="fp16", D=64, Sq=129, lens=[65, 333, 64], q_lens=[129, 0, 77]),
                 dict(dtype="bf16", D=128, Sq=200, lens=[333, 63, 130], q_lens=[200, 150, 0]),
                 dict(dtype="bf16", D=64, Sq=65, lens=[333, 1, 0], q_lens=[1, 65, 64]),
                 dict(dtype="fp16", D=128, Sq=1, lens=[65, 333, 0], q_lens=[1, 1, 1])]
P_HQ, P_HKV = 4, 2


def _pcase_id(c):
    return f"{c['dtype']}D{c['D']}Sq{c['Sq']}n{'_'.join(map(str, c['lens']))}q{'_'.join(map(str, c['q_lens']))}"


@pytest.mark.parametrize("case", PREFILL_CASES, ids=_pcase_id)
def test_prefill_equals_the_byte_cache(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    dtype, D, Sq, lens, q_lens = (case[k] for k in ("dtype", "D", "Sq", "lens", "q_lens"))
    B = len(lens)
    for v_bits in (16, 8):
        c4, cb, p4, rng = _trio(lb, oracle, dev, B=B, Hkv=P_HKV, D=D, dtype=dtype, lens=lens, page=64, seed=43 + D + Sq, v_bits=v_bits)
        tq = _t(_rand(oracle, rng, (B, P_HQ, Sq, D), dtype), dtype, dev)
        ql = torch.tensor(q_lens, dtype=torch.int32, device=dev)
        for causal in (True, False):
            for i, ns in enumerate((1, 2, 7, 0)):
                layout, q_bits = ("HND", "NHD")[(i + causal) % 2], (8, 4)[i // 2 ^ causal]
                q = tq if layout == "HND" else _nhd(tq)
                kw = dict(is_causal=causal, return_lse=True, num_splits=ns, q_lens=ql, tensor_layout=layout, q_bits=q_bits)
                what = f"{_pcase_id(case)} v_bits={v_bits} causal={causal} splits={ns} {layout} q_bits={q_bits}"
                got = lb.lowbit_fa_prefill(q, c4, **kw)
                same_bits(got, lb.lowbit_fa_prefill(q, cb, **kw), what + " contiguous")
                same_bits(lb.lowbit_fa_prefill(q, p4, **kw), got, what + " paged")
                assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), what


# ------------------------------------------------------------------------------------------------------------------------
# 4. the oracle's kernel on the unpacked numpy state
# ------------------------------------------------------------------------------------------------------------------------
def test_decode_equals_oracle(oracle, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    case = DECODE_CASES[4]  # fp16 D=128 M=32
    dtype, D, Sq, G, Hkv, lens = (case[k] for k in ("dtype", "D", "Sq", "G", "Hkv", "lens"))
    B, sm = len(lens), D ** -0.5
    k, v, _ = _same_kv(oracle, B, Hkv, D, dtype, lens, 79)
    c4 = _fill(lb.LowbitKVCache(B, Hkv, D, max(lens), TDT[dtype], dev, k_bits=4, k_packed=True), k, v, lens, dtype, dev)
    q = _rand(oracle, np.random.default_rng(D + Sq), (B, G * Hkv, Sq, D), dtype)
    q_i8, q_scale = kr.quant_q(oracle, q, sm, 127)
    corr = kr.lse_correction(oracle, q, _np(c4.km), dtype)
    for causal in (False, True):
        o_ref, lse2 = k4.oracle_decode(oracle, q_i8, q_scale, c4.k_codes.cpu().numpy(), c4.k_scale.cpu().numpy(), _np(c4.v), np.array(lens),
                                       causal=causal, out_dtype=dtype)
        lse_ref = kr.natural_lse(lse2, corr, sm)
        for ns in (1, 0):
            what = f"{_case_id(case)} causal={causal} splits={ns}"
            o, lse = lb.lowbit_fa_decode(_t(q, dtype, dev), c4, is_causal=causal, return_lse=True, num_splits=ns)
            kr.check_o(_np(o), o_ref, dtype, what)
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, what)


def test_prefill_equals_oracle(oracle, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    case = PREFILL_CASES[0]
    dtype, D, Sq, lens, q_lens = (case[k] for k in ("dtype", "D", "Sq", "lens", "q_lens"))
    B, sm = len(lens), D ** -0.5
    k, v, _ = _same_kv(oracle, B, P_HKV, D, dtype, lens, 5)
    c4 = _fill(lb.LowbitKVCache(B, P_HKV, D, max(lens), TDT[dtype], dev, k_bits=4, k_packed=True), k, v, lens, dtype, dev)
    q = _rand(oracle, np.random.default_rng(6), (B, P_HQ, Sq, D), dtype)
    q_i8, q_scale = pr.quant_q_blocks(oracle, q, q_lens, sm, 127)
    corr = kr.lse_correction(oracle, q, _np(c4.km), dtype)
    o_ref, lse2 = k4.oracle_prefill(oracle, q_i8, q_scale, c4.k_codes.cpu().numpy(), c4.k_scale.cpu().numpy(), _np(c4.v), lens, q_lens,
                                    causal=True, out_dtype=dtype)
    lse_ref = kr.natural_lse(lse2, corr, sm)
    lse_ref = np.where(np.isinf(lse2), -np.inf, lse_ref).astype(np.float32)
    for ns in (1, 3):
        o, lse = lb.lowbit_fa_prefill(_t(q, dtype, dev), c4, is_causal=True, return_lse=True, num_splits=ns,
                                      q_lens=torch.tensor(q_lens, dtype=torch.int32, device=dev))
        kr.check_o(_np(o), o_ref, dtype, f"prefill splits={ns}")
        kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, f"prefill splits={ns}")


# ------------------------------------------------------------------------------------------------------------------------
# 5. hostile memory
# ------------------------------------------------------------------------------------------------------------------------
HOSTILE_LENS = [1, 63, 64, 65, 130]


def _garbage(codes, scale_fill):
    def fill(cache):
        """K: 0x88 (the pair of -8s no quantiser writes) or random bytes, scales NaN / inf, tail NaN; V NaN (fp8: the NaN code and
        the same scales) - everywhere, every page"""
        if codes == "random":
            g = torch.Generator(device="cpu").manual_seed(5)
            cache.k_codes.copy_(torch.randint(0, 256, tuple(cache.k_codes.shape), generator=g, dtype=torch.uint8))
        else:
            cache.k_codes.fill_(0x88)
        cache.k_scale.fill_(scale_fill), cache.k_tail.fill_(float("nan"))
        if cache.v_bits == 8:
            cache.v.fill_(0xFF), cache.v_scale.fill_(scale_fill)
        else:
            cache.v.fill_(float("nan"))
        return cache
    return fill


@pytest.mark.parametrize("dtype,D,v_bits,codes,scale_fill", [("fp16", 64, 16, "0x88", float("nan")), ("bf16", 128, 8, "random", float("inf")),
                                                            ("fp16", 128, 16, "random", float("nan"))])
def test_packed_cache_in_hostile_memory(oracle, dev, dtype, D, v_bits, codes, scale_fill):
    import lowbit_quant_fa2_paddle_amd as lb
    B, lens = len(HOSTILE_LENS), HOSTILE_LENS
    args = dict(B=B, Hkv=2, D=D, dtype=dtype, lens=lens, page=64, seed=53 + D, v_bits=v_bits)
    h4, _, hp4, rng = _trio(lb, oracle, dev, garbage=_garbage(codes, scale_fill), **args)
    clean, _, _, _ = _trio(lb, oracle, dev, **args)
    what = f"hostile packed cache {dtype} D={D}"
    bad_scale = torch.isnan if scale_fill != scale_fill else torch.isinf
    for b, n in enumerate(lens):  # the valid rows are the clean cache's, the garbage behind them is still there
        same_bits(h4.k_codes[b, :, :n], clean.k_codes[b, :, :n], what + ": codes")
        same_bits(hp4.gather(b)[0][:, :n], clean.k_codes[b, :, :n], what + ": paged codes")
        assert bad_scale(h4.k_scale[b, :, (n + 63) // 64:]).all(), (what, b)
        if codes == "0x88":
            assert torch.all(h4.k_codes[b, :, n:] == 0x88) and torch.all(hp4.gather(b)[0][:, n:] == 0x88), (what, b)
    spare = torch.tensor(hp4.allocator.free_pages, device=dev)
    assert len(spare) and bad_scale(hp4.k_scale[spare]).all() and hp4.k_codes[spare].any(), what
    for Sq, causal in ((1, False), (3, True)):
        tq = _t(_rand(oracle, rng, (B, 4, Sq, D), dtype), dtype, dev)
        for ns in (1, 3):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
            w = f"{what} decode Sq={Sq} splits={ns}"
            want = lb.lowbit_fa_decode(tq, clean, **kw)
            for cache in (h4, hp4):
                got = lb.lowbit_fa_decode(tq, cache, **kw)
                assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), w + ": a row behind the end of a sequence was read"
                same_bits(got, want, w)
    tq = _t(_rand(oracle, rng, (B, 4, 130, D), dtype), dtype, dev)
    ql = torch.tensor([130, 1, 129, 65, 0], dtype=torch.int32, device=dev)
    for causal in (True, False):
        for ns in (1, 3):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns, q_lens=ql)
            w = f"{what} prefill causal={causal} splits={ns}"
            want = lb.lowbit_fa_prefill(tq, clean, **kw)
            for cache in (h4, hp4):
                got = lb.lowbit_fa_prefill(tq, cache, **kw)
                assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), w + ": a row behind the end of a sequence was read"
                same_bits(got, want, w)


# ------------------------------------------------------------------------------------------------------------------------
# 6. containment: everything the append writes of K lies in the rows of the blocks it touches, below `end`
# ------------------------------------------------------------------------------------------------------------------------
STATE = ("k_codes", "k_scale", "v", "k_tail", "km")
PAGED_STATE = STATE + ("seqlens", "block_table")
APPENDS = [(1, None), (63, None), (2, None), (200, [200, 7, 131])]  # T = 1; 63 then 2 (crossing a block); 200 with ragged new_lens
K_FILL = 0x5A  # what rows nobody appended hold: the codes (-6, 5)


def _arena_backed(cache, arena, names):
    for name in names:
        setattr(cache, name, arena.like(getattr(cache, name)))
    return cache


def _ref_filled(orc, B, H, D, cap, dtype):
    ref = k4.CacheRefK4(orc, B, H, D, cap, dtype)
    ref.k_codes[..., 0::2], ref.k_codes[..., 1::2] = -6, 5
    assert np.all(ref.k_packed == K_FILL)
    return ref


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_append_writes_only_its_rows(monkeypatch, oracle, dev, dtype, D):
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, cap = 3, 2, 320
    rng = np.random.default_rng(63 + D)
    arena = GuardArena(monkeypatch, dev)
    cache = _arena_backed(lb.LowbitKVCache(B, H, D, cap, TDT[dtype], dev, k_bits=4, k_packed=True), arena, STATE)
    cache.k_codes.fill_(K_FILL)
    ref = _ref_filled(oracle, B, H, D, cap, dtype)
    for T, lens in APPENDS:
        k, v = _rand(oracle, rng, (B, H, T, D), dtype, bias=0.5), _rand(oracle, rng, (B, H, T, D), dtype, mul=2.0)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        with arena:  # the mean's workspace of the first append
            cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=tl)
        ref.append(k, v, lens)
        torch.cuda.synchronize()
        arena.check()
        # EVERY byte of k_codes: rows of a touched block below `end` hold the model's row, all others what they held
        assert np.array_equal(cache.k_codes.cpu().numpy(), ref.k_packed), (dtype, D, T, "k_codes")
        assert np.array_equal(cache.k_scale.cpu().numpy().view(np.uint32), ref.k_scale.view(np.uint32)), (dtype, D, T, "k_scale")
    assert (ref.k_packed != K_FILL).any() and (ref.k_packed[:, :, 300:] == K_FILL).all()  # not vacuous


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_append_at_the_capacity_and_negative_lengths(monkeypatch, oracle, dev, dtype, D):
    """The siblings' defended cases, inside memory the test owns.  Capacity 128, device lengths [125, 128, 60] behind the host's
    back, T = 8: sequence 0 takes rows 125 .. 127 and drops five, sequence 1 none, sequence 2 all eight - unclipped, sequence 0 / 1
    would write into the next (batch, head) slab of k_codes, behind the last of which lies the arena's guard.  Then lengths
    [-5, 0, 0] with new_lens [-1, 9, 3]: clamped to 0, 0, 0 and 0, 8, 3 new rows - unclamped, five rows before slab (0, 0): the
    guard in front.  A read with lengths [-3, 10^6, 70] is the read with [0, 128, 70]."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, cap, T = 3, 2, 128, 8
    rng = np.random.default_rng(73 + D)
    mk = lambda T_: (_rand(oracle, rng, (B, H, T_, D), dtype, bias=0.5), _rand(oracle, rng, (B, H, T_, D), dtype, mul=2.0))
    (k0, v0), (k1, v1) = mk(60), mk(T)
    arena = GuardArena(monkeypatch, dev)
    new = lambda: _arena_backed(lb.LowbitKVCache(B, H, D, cap, TDT[dtype], dev, k_bits=4, k_packed=True), arena, STATE)
    cache, ref = new(), k4.CacheRefK4(oracle, B, H, D, cap, dtype)
    cache.append(_t(k0, dtype, dev), _t(v0, dtype, dev))
    ref.append(k0, v0)
    lens_dev = [125, 128, 60]
    cache.seqlens.copy_(torch.tensor(lens_dev, dtype=torch.int32, device=dev))
    ref.seqlens[:] = lens_dev
    assert cache.max_seqlen == 60  # the host's bound: it lets T = 8 through
    cache.append(_t(k1, dtype, dev), _t(v1, dtype, dev))
    ref.append(k1, v1)
    torch.cuda.synchronize()
    arena.check()
    assert list(ref.seqlens) == [128, 128, 68]

    def whole(what):
        assert np.array_equal(cache.k_codes.cpu().numpy(), ref.k_packed), (what, "k_codes")
        assert np.array_equal(cache.k_scale.cpu().numpy().view(np.uint32), ref.k_scale.view(np.uint32)), (what, "k_scale")

    whole("at the capacity")
    # lengths outside [0, max_seqlen_k] are clamped by the readers
    tq = _t(_rand(oracle, rng, (B, 2 * H, 2, D), dtype), dtype, dev)
    cache.max_seqlen = cap
    cache.seqlens.copy_(torch.tensor([0, 128, 68], dtype=torch.int32, device=dev))
    want = lb.lowbit_fa_decode(tq, cache, return_lse=True, num_splits=2), lb.lowbit_fa_prefill(tq, cache, return_lse=True, num_splits=2)
    cache.seqlens.copy_(torch.tensor([-3, 10 ** 6, 68], dtype=torch.int32, device=dev))
    with arena:
        got = lb.lowbit_fa_decode(tq, cache, return_lse=True, num_splits=2), lb.lowbit_fa_prefill(tq, cache, return_lse=True, num_splits=2)
    torch.cuda.synchronize()
    arena.check()
    same_bits(got[0], want[0], "decode clamps the lengths")
    same_bits(got[1], want[1], "prefill clamps the lengths")
    # negative lengths, on a fresh cache
    cache, ref = new(), k4.CacheRefK4(oracle, B, H, D, cap, dtype)
    cache.seqlens.copy_(torch.tensor([-5, 0, 0], dtype=torch.int32, device=dev))
    ref.seqlens[:] = [-5, 0, 0]
    new_lens = [-1, 9, 3]
    with arena:
        cache.append(_t(k1, dtype, dev), _t(v1, dtype, dev), new_lens=torch.tensor(new_lens, dtype=torch.int32, device=dev))
    ref.append(k1, v1, new_lens)
    torch.cuda.synchronize()
    arena.check()
    whole("negative lengths")
    assert not cache.k_codes[0].any() and cache.k_codes[1, :, :8].any() and not cache.k_codes[1, :, 8:].any()


def _paged_k4_call(lib, name, cache, dev, dtype, **kw):
    """one call of a paged _k4 entry point by ctypes, every argument by keyword, in the order of include/lowbit_fa.h"""
    from lowbit_quant_fa2_paddle_amd import _lib
    order = {"lbfa_kvcache_paged_append_k4": ("k_new", "v_new", "dtype", "new_lens", "km", "k_codes", "k_scale", "v_cache", "k_tail", "seqlens",
                                              "block_table", "slots", "B", "Hkv", "T", "D", "num_slots", "num_pages", "page_size",
                                              "max_pages", "sk", "sv", "k_qmax", "stream"),
             "lbfa_decode_paged_k4": ("q", "dtype", "k_codes", "k_scale", "v_cache", "km", "seqlens", "block_table", "slots", "o", "lse",
                                      "workspace", "workspace_bytes", "B", "Hq", "Hkv", "Sq", "D", "num_slots", "num_pages", "page_size",
                                      "max_pages", "max_k", "num_splits", "sq", "so", "sm_scale", "q_qmax", "causal", "stream")}[name]
    assert len(order) == len(_lib.SIGNATURES[name][1])
    args = dict(dtype=_lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16, km=cache.km.data_ptr(), k_codes=cache.k_codes.data_ptr(),
                k_scale=cache.k_scale.data_ptr(), v_cache=cache.v.data_ptr(), seqlens=cache.seqlens.data_ptr(), Hkv=cache.num_kv_heads,
                D=cache.padded_head_dim, num_slots=cache.max_seqs, num_pages=cache.num_pages, page_size=cache.page_size,
                max_pages=cache.max_pages_per_seq, stream=torch.cuda.current_stream(dev).cuda_stream)
    args.update(kw)
    assert set(args) == set(order), sorted(set(args) ^ set(order))
    vals = [_lib.strides3(args[k]) if isinstance(args[k], tuple) else args[k] for k in order]
    _lib.check(getattr(lib, name)(*vals), lib)


@pytest.mark.parametrize("dtype,D,page", [("fp16", 64, 64), ("bf16", 128, 128)])
def test_paged_append_skips_and_decode_clamps_corrupt_ids(monkeypatch, oracle, dev, dtype, D, page):
    """lbfa_kvcache_paged_append_k4 with slots [-1, 1, num_slots] and, under the blocks the append touches in slot 1's table, the
    pages -1 and num_pages + 1: rows 0 and 2 are skipped and so are both blocks of row 1 - pool and guards stay as they were.
    Unskipped, slot -1 / num_slots lies one slot before / behind the per-slot tensors and page -1 / num_pages + 1 at most two pages
    before / behind the pool tensors: the arena's guard (128 KiB; a page of packed codes is at most 2 x 128 x 64 = 16 KiB, of V
    64 KiB).  lbfa_decode_paged_k4 clamps the same ids: its result is that of slots [0, 1, num_slots - 1] and pages 0 and
    num_pages - 1."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    H, num_slots, max_pages, num_pages, T = 2, 3, 4, 14, 3 * page // 2
    rng = np.random.default_rng(83 + D)
    arena = GuardArena(monkeypatch, dev)
    cache = _arena_backed(lb.LowbitPagedKVCache(num_pages, page, H, D, num_slots, max_pages, TDT[dtype], dev, k_bits=4, k_packed=True),
                          arena, PAGED_STATE)
    assert 2 * H * page * D * 2 <= arena.guard_bytes
    n0 = page + 6  # every slot holds a page and six keys
    k0, v0 = _rand(oracle, rng, (num_slots, H, n0, D), dtype, bias=0.5), _rand(oracle, rng, (num_slots, H, n0, D), dtype)
    k1, v1 = _rand(oracle, rng, (num_slots, H, T, D), dtype, bias=0.5), _rand(oracle, rng, (num_slots, H, T, D), dtype)
    with arena:
        cache.append(_t(k0, dtype, dev), _t(v0, dtype, dev))
    assert n0 // page == 1 and (n0 + T - 1) // page == 2  # the append below covers table entries 1 and 2 of a slot
    table = cache.block_table.clone()
    table[1, 1], table[1, 2] = -1, num_pages + 1
    bad_table = arena.like(table)
    bad_slots = arena.like(torch.tensor([-1, 1, num_slots], dtype=torch.int32, device=dev))
    state = {name: getattr(cache, name).clone() for name in PAGED_STATE}
    tk, tv = _t(k1, dtype, dev), _t(v1, dtype, dev)
    app = dict(k_new=tk.data_ptr(), v_new=tv.data_ptr(), new_lens=None, k_tail=cache.k_tail.data_ptr(), B=num_slots, T=T,
               sk=tuple(tk.stride()[:3]), sv=tuple(tv.stride()[:3]), k_qmax=7)
    _paged_k4_call(lib, "lbfa_kvcache_paged_append_k4", cache, dev, dtype, block_table=bad_table.data_ptr(), slots=bad_slots.data_ptr(), **app)
    torch.cuda.synchronize()
    arena.check()
    for name, t in state.items():
        same_bits(getattr(cache, name), t, f"corrupt ids {dtype} D={D}: {name} changed")

    G, Sq = 2, 3
    tq = _t(_rand(oracle, rng, (num_slots, G * H, Sq, D), dtype), dtype, dev)

    def decode(slot_ids, pg1, pg2, ns):
        tb = cache.block_table.clone()
        tb[1, 0], tb[1, 1] = pg1, pg2
        tb, sl = arena.like(tb), arena.like(torch.tensor(slot_ids, dtype=torch.int32, device=dev))
        o, lse = arena.allocate((num_slots, G * H, Sq, D), TDT[dtype]), arena.allocate((num_slots, G * H, Sq), torch.float32)
        nbytes = lib.lbfa_decode_workspace_bytes(num_slots, G * H, H, Sq, cache.padded_head_dim, n0, ns)
        ws = arena.allocate((max(nbytes, 16),), torch.uint8)
        _paged_k4_call(lib, "lbfa_decode_paged_k4", cache, dev, dtype, q=tq.data_ptr(), block_table=tb.data_ptr(), slots=sl.data_ptr(),
                       o=o.data_ptr(), lse=lse.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes, B=num_slots, Hq=G * H,
                       Sq=Sq, max_k=n0, num_splits=ns, sq=tuple(tq.stride()[:3]), so=tuple(o.stride()[:3]), sm_scale=D ** -0.5,
                       q_qmax=127, causal=1)
        torch.cuda.synchronize()
        arena.check()
        return o, lse

    for ns in (1, 3):
        same_bits(decode([-1, 1, num_slots], -1, num_pages + 1, ns), decode([0, 1, num_slots - 1], 0, num_pages - 1, ns),
                  f"decode clamps {dtype} D={D} splits={ns}")

    # the same append with a sound table and slots [0, 1, 2] does append (the case above was not vacuous)
    good = arena.like(torch.tensor([0, 1, 2], dtype=torch.int32, device=dev))
    table = cache.block_table.clone()
    table[:, 2] = torch.tensor(cache.allocator.free_pages[:num_slots], dtype=torch.int32, device=dev)
    sound = arena.like(table)
    assert len(set(table[:, :3].flatten().tolist())) == 3 * num_slots and int(table.max()) < num_pages
    _paged_k4_call(lib, "lbfa_kvcache_paged_append_k4", cache, dev, dtype, block_table=sound.data_ptr(), slots=good.data_ptr(), **app)
    torch.cuda.synchronize()
    arena.check()
    assert not torch.equal(cache.k_codes, state["k_codes"])


# ------------------------------------------------------------------------------------------------------------------------
# the front end
# ------------------------------------------------------------------------------------------------------------------------
def test_front_end(oracle, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(ValueError, match="k_packed=True needs k_bits=4"):
        lb.LowbitKVCache(1, 1, 64, 64, torch.float16, dev, k_packed=True)
    with pytest.raises(ValueError, match="k_packed=True needs k_bits=4"):
        lb.LowbitPagedKVCache(2, 64, 1, 64, 1, 2, torch.float16, dev, k_bits=8, k_packed=True)
    for cache in (lb.LowbitKVCache(2, 2, 64, 128, torch.float16, dev), lb.LowbitKVCache(2, 2, 64, 128, torch.float16, dev, k_bits=4),
                  lb.LowbitPagedKVCache(4, 64, 2, 64, 2, 2, torch.bfloat16, dev, k_bits=4, k_packed=False)):
        assert not cache.k_packed and cache.k_codes.dtype == torch.int8 and cache.unpacked_k_codes() is cache.k_codes
