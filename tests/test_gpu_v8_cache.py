"""GPU tests of the fp8 V cache (`v_bits=8` of `LowbitKVCache` / `LowbitPagedKVCache`; lbfa_*_v8): V as e4m3 codes with one fp32
scale per key and kv head.

1. state: after every append of a ragged schedule `v` and `v_scale` of the valid rows equal the numpy model (tests/v8_reference.py)
   bit for bit, the K state is `torch.equal` to a `v_bits=16` cache's, and the paged cache agrees through `gather`;
2. decode, differential and tolerance-free: a read of the fp8 cache is `torch.equal` to the same read of a `v_bits=16` cache whose
   `v` was overwritten with V^ = fp16(fp32(decode(code)) * scale) computed in numpy - every kernel instance, 1 / 2 / 7 / chosen
   slices, causal or not, contiguous and paged;
3. decode against the oracle's int8 / fp16 kernel on (cache codes, V^) within the unchanged bars `check_o` / `check_lse`;
4. cached prefill: the same differential test and one oracle check;
5. hostile memory: rows at or past the length and unused pages hold the e4m3 NaN code and NaN / +inf scales;
6. containment: guard bands around `v` and `v_scale`, rows outside [s0, end) keep their bytes, the device-side defences;
7. the front end.
Shapes stay at B <= 5, Hkv <= 3 and at most 700 keys.  The rest is elsewhere: the schedules, packed views, page sizes and slice
counts of the fuzzes meet the fp8 cache in tests/test_gpu_decode_fuzz.py (an fp8 twin of every case) and
tests/test_gpu_prefill_fuzz.py (half of the cases), long contexts and offsets past 2^31 in tests/test_gpu_prefill_long.py.
"""
import numpy as np
import pytest

import kvcache_reference as kr
import prefill_reference as pr
import v8_reference as v8
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


def _vhat_into(orc, c8, c16):
    """overwrite the public `v` of the fp16 cache with V^ of the fp8 cache, computed in numpy from its codes and scales"""
    vhat = v8.dequant_v(orc, c8.v.cpu().numpy(), c8.v_scale.cpu().numpy())
    assert vhat.dtype == np.float16 and c16.v.dtype == torch.float16 and tuple(c16.v.shape) == vhat.shape
    c16.v.copy_(torch.from_numpy(vhat).to(c16.v.device))
    return c16


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


def _quartet(lb, orc, dev, *, B, Hkv, D, dtype, lens, page, seed, garbage=None):
    """the four caches of a differential test, filled with the same appends: contiguous fp8, contiguous fp16 holding V^, paged fp8,
    paged fp16 holding V^ (scrambled pages, spare pages in the pool).  `garbage`: a function applied to each fresh fp8 cache."""
    rng = np.random.default_rng(seed)
    T = max(lens)
    k = _rand(orc, rng, (B, Hkv, T, D), dtype, bias=0.5)
    v = _rand(orc, rng, (B, Hkv, T, D), dtype, mul=3.0)  # |V| up to ~ 15: codes all over the e4m3 range
    max_pages = -(-T // page)
    order = np.random.default_rng(seed + page).permutation(B * max_pages + 2).tolist()
    mk = lambda bits: lb.LowbitKVCache(B, Hkv, D, T, TDT[dtype], dev, v_bits=bits)
    mkp = lambda bits: lb.LowbitPagedKVCache(B * max_pages + 2, page, Hkv, D, B, max_pages, TDT[dtype], dev, page_order=order, v_bits=bits)
    c8, p8 = mk(8), mkp(8)
    if garbage is not None:
        garbage(c8), garbage(p8)
    c8, p8 = _fill(c8, k, v, lens, dtype, dev), _fill(p8, k, v, lens, dtype, dev)
    c16 = _vhat_into(orc, c8, _fill(mk(16), k, v, lens, dtype, dev))
    p16 = _vhat_into(orc, p8, _fill(mkp(16), k, v, lens, dtype, dev))
    return c8, c16, p8, p16, rng


# ------------------------------------------------------------------------------------------------------------------------
# 1. state
# ------------------------------------------------------------------------------------------------------------------------
STEPS = [(70, None), (1, [1, 1, 0]), (1, [1, 0, 1]), (63, [63, 10, 0]), (64, [64, 64, 33]), (65, [0, 65, 64]), (200, [200, 1, 150])]


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128), ("fp16", 80)])
def test_state_equals_the_model_after_every_append(oracle, dev, dtype, D):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(23 + D)
    B, H, Dp, total = 3, 2, _padded(D), sum(T for T, _ in STEPS)
    c8 = lb.LowbitKVCache(B, H, D, 600, TDT[dtype], dev, v_bits=8)
    c16 = lb.LowbitKVCache(B, H, D, 600, TDT[dtype], dev)
    assert c8.v.dtype == torch.uint8 and tuple(c8.v.shape) == (B, H, 640, Dp)
    assert c8.v_scale.dtype == torch.float32 and tuple(c8.v_scale.shape) == (B, H, 640)
    ref = v8.CacheRefV8(oracle, B, H, Dp, 640, dtype)
    paged = []
    for page in (64, 192):
        # exactly the pages the schedule reserves: the page(s) a freed slot gives back are handed out again
        n_pages = B * -(-total // page)
        order = np.random.default_rng(page).permutation(n_pages).tolist()
        p = lb.LowbitPagedKVCache(n_pages, page, H, D, B, -(-640 // page), TDT[dtype], dev, page_order=order, v_bits=8)
        assert p.v.dtype == torch.uint8 and tuple(p.v.shape) == (n_pages, H, page, Dp) and tuple(p.v_scale.shape) == (n_pages, H, page)
        junk = _t(_rand(oracle, rng, (1, H, 100, D), dtype, mul=50.0), dtype, dev)
        p.append(junk, junk, slots=[1])  # one slot filled, freed and reused: stale codes and scales in the pages it gets
        p.free(1)
        assert p.num_free_pages == n_pages
        paged.append(p)
    for step, (T, lens) in enumerate(STEPS):
        k = _rand(oracle, rng, (B, H, T, D), dtype, bias=0.5)
        v = _rand(oracle, rng, (B, H, T, D), dtype, mul=float(rng.choice([1e-3, 1.0, 40.0])))
        tk, tv = _t(k, dtype, dev), _t(v, dtype, dev)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        for cache in [c8, c16] + paged:
            if step % 2:
                cache.append(_nhd(tk), _nhd(tv), tensor_layout="NHD", new_lens=tl)
            else:
                cache.append(tk, tv, new_lens=tl)
        ref.append(_pad(k, D), _pad(v, D), lens)
        what = f"{dtype} D={D} step {step}"
        codes, scales = c8.v.cpu().numpy(), c8.v_scale.cpu().numpy()
        assert np.array_equal(c8.seqlens.cpu().numpy(), ref.seqlens), what
        for b, n in enumerate(int(x) for x in ref.seqlens):
            assert np.array_equal(codes[b, :, :n], ref.v_codes[b, :, :n]), (what, b, "v codes")
            assert np.array_equal(scales[b, :, :n].view(np.uint32), ref.v_scale[b, :, :n].view(np.uint32)), (what, b, "v scales")
            assert not codes[b, :, n:].any() and not scales[b, :, n:].any(), (what, b, "rows past the end were written")
        for name in ("k_codes", "k_scale", "k_tail", "km", "seqlens"):  # all K state is the fp16-V cache's
            assert torch.equal(getattr(c8, name), getattr(c16, name)), (what, name)
        for p in paged:
            assert torch.equal(p.seqlens, c8.seqlens), what
            for b, n in enumerate(c8.seqlens.tolist()):
                kc, ks, vc, vs = p.gather(b)
                w = f"{what} page {p.page_size} sequence {b}"
                same_bits(vc[:, :n], c8.v[b, :, :n], w + ": v codes")
                same_bits(vs[:, :n], c8.v_scale[b, :, :n], w + ": v scales")
                same_bits(kc[:, :n], c8.k_codes[b, :, :n], w + ": k codes")
                same_bits(ks[:, :(n + 63) // 64], c8.k_scale[b, :, :(n + 63) // 64], w + ": k scales")
            same_bits(p.km, c8.km, what + ": km")
    # the debugging aid is V^, within the format's error bound of the appended V
    vd = _np(c8.dequantized_v())
    assert tuple(vd.shape) == (B, H, 640, D) and c8.dequantized_v().dtype == torch.float16
    vh = ref.vhat()
    for b, n in enumerate(int(x) for x in ref.seqlens):
        assert np.array_equal(vd[b, :, :n], vh[b, :, :n, :D]), (b, "dequantized_v is not V^")


# ------------------------------------------------------------------------------------------------------------------------
# 2. / 3. decode
# ------------------------------------------------------------------------------------------------------------------------
# every kernel instance: 2 dtypes x 2 head dims x (1, 2, 4 row blocks: M = 8, 32, 64), and a padded head dim
DECODE_CASES = [dict(dtype=dt, D=D, Sq=Sq, G=G, Hkv=2 if (D + Sq) % 3 else 3, lens=LENS_A if i % 2 == 0 else LENS_B)
                for i, (dt, D, (Sq, G)) in enumerate((dt, D, sg) for dt in ("fp16", "bf16") for D in (64, 128)
                                                     for sg in ((1, 8), (4, 8), (16, 4)))]
DECODE_CASES.append(dict(dtype="fp16", D=80, Sq=2, G=4, Hkv=2, lens=LENS_B))
ORACLE_CASES = [DECODE_CASES[3], DECODE_CASES[7], DECODE_CASES[12]]  # fp16 D=128 M=8, bf16 D=64 M=32, fp16 D=80


def _case_id(c):
    return f"{c['dtype']}D{c['D']}Sq{c['Sq']}G{c['G']}Hkv{c['Hkv']}n{'_'.join(map(str, c['lens']))}"


@pytest.mark.parametrize("case", DECODE_CASES, ids=_case_id)
def test_decode_equals_the_fp16_cache_holding_vhat(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    dtype, D, Sq, G, Hkv, lens = (case[k] for k in ("dtype", "D", "Sq", "G", "Hkv", "lens"))
    B = len(lens)
    c8, c16, p8, p16, rng = _quartet(lb, oracle, dev, B=B, Hkv=Hkv, D=D, dtype=dtype, lens=lens, page=128, seed=31 + D + Sq)
    tq = _t(_rand(oracle, rng, (B, G * Hkv, Sq, D), dtype), dtype, dev)
    for causal in (False, True):
        for ns in (1, 2, 7, 0):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
            what = f"{_case_id(case)} causal={causal} splits={ns}"
            got = lb.lowbit_fa_decode(tq, c8, **kw)
            same_bits(got, lb.lowbit_fa_decode(tq, c16, **kw), what + " contiguous")
            gotp = lb.lowbit_fa_decode(tq, p8, **kw)
            same_bits(gotp, lb.lowbit_fa_decode(tq, p16, **kw), what + " paged")
            same_bits(gotp, got, what + " paged against contiguous")
            assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), what
    # not vacuous: V^ is not V
    assert not torch.equal(lb.lowbit_fa_decode(tq, c8), lb.lowbit_fa_decode(tq, _fill(
        lb.LowbitKVCache(B, Hkv, D, max(lens), TDT[dtype], dev), *_same_kv(oracle, B, Hkv, D, dtype, lens, 31 + D + Sq), lens, dtype, dev)))


def _same_kv(orc, B, Hkv, D, dtype, lens, seed):
    """k, v of `_quartet` for the same seed"""
    rng = np.random.default_rng(seed)
    T = max(lens)
    return _rand(orc, rng, (B, Hkv, T, D), dtype, bias=0.5), _rand(orc, rng, (B, Hkv, T, D), dtype, mul=3.0)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_case_id)
def test_decode_equals_oracle_on_vhat(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    dtype, D, Sq, G, Hkv, lens = (case[k] for k in ("dtype", "D", "Sq", "G", "Hkv", "lens"))
    B, Dp, sm = len(lens), _padded(D), D ** -0.5
    k, v = _same_kv(oracle, B, Hkv, D, dtype, lens, 77 + D)
    c8 = _fill(lb.LowbitKVCache(B, Hkv, D, max(lens), TDT[dtype], dev, v_bits=8), k, v, lens, dtype, dev)
    q = _rand(oracle, np.random.default_rng(D + Sq), (B, G * Hkv, Sq, D), dtype)
    qp = _pad(q, D)
    q_i8, q_scale = kr.quant_q(oracle, qp, sm, 127)
    vhat = v8.dequant_v(oracle, c8.v.cpu().numpy(), c8.v_scale.cpu().numpy()).astype(np.float32)
    corr = kr.lse_correction(oracle, qp, _np(c8.km), dtype)
    for causal in (False, True):
        o_ref, lse2 = kr.oracle_decode(oracle, q_i8, q_scale, c8.k_codes.cpu().numpy(), c8.k_scale.cpu().numpy(), vhat, np.array(lens),
                                       causal=causal, out_dtype=dtype)
        lse_ref = kr.natural_lse(lse2, corr, sm)
        for ns in (1, 0):
            what = f"{_case_id(case)} causal={causal} splits={ns}"
            o, lse = lb.lowbit_fa_decode(_t(q, dtype, dev), c8, is_causal=causal, return_lse=True, num_splits=ns)
            kr.check_o(_np(o), o_ref[..., :D], dtype, what)
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, what)


# ------------------------------------------------------------------------------------------------------------------------
# 4. cached prefill
# ------------------------------------------------------------------------------------------------------------------------
PREFILL_CASES = [dict(dtype="fp16", D=64, Sq=129, lens=[65, 321, 65], q_lens=[129, 0, 77]),
                 dict(dtype="bf16", D=128, Sq=200, lens=[321, 65, 321], q_lens=[200, 150, 0]),
                 dict(dtype="bf16", D=64, Sq=200, lens=[321, 65, 0], q_lens=[1, 200, 64]),
                 dict(dtype="fp16", D=128, Sq=129, lens=[65, 321, 321], q_lens=[128, 129, 0])]
P_HQ, P_HKV = 4, 2


def _pcase_id(c):
    return f"{c['dtype']}D{c['D']}Sq{c['Sq']}n{'_'.join(map(str, c['lens']))}q{'_'.join(map(str, c['q_lens']))}"


@pytest.mark.parametrize("case", PREFILL_CASES, ids=_pcase_id)
def test_prefill_equals_the_fp16_cache_holding_vhat(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    dtype, D, Sq, lens, q_lens = (case[k] for k in ("dtype", "D", "Sq", "lens", "q_lens"))
    B = len(lens)
    c8, c16, p8, p16, rng = _quartet(lb, oracle, dev, B=B, Hkv=P_HKV, D=D, dtype=dtype, lens=lens, page=64, seed=41 + D + Sq)
    tq = _t(_rand(oracle, rng, (B, P_HQ, Sq, D), dtype), dtype, dev)
    ql = torch.tensor(q_lens, dtype=torch.int32, device=dev)
    for causal in (True, False):
        for ns in (1, 3, 0):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns, q_lens=ql)
            what = f"{_pcase_id(case)} causal={causal} splits={ns}"
            got = lb.lowbit_fa_prefill(tq, c8, **kw)
            same_bits(got, lb.lowbit_fa_prefill(tq, c16, **kw), what + " contiguous")
            gotp = lb.lowbit_fa_prefill(tq, p8, **kw)
            same_bits(gotp, lb.lowbit_fa_prefill(tq, p16, **kw), what + " paged")
            same_bits(gotp, got, what + " paged against contiguous")
            assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), what


def test_prefill_equals_oracle_on_vhat(oracle, dev):
    import types

    import lowbit_quant_fa2_paddle_amd as lb
    case = PREFILL_CASES[0]
    dtype, D, Sq, lens, q_lens = (case[k] for k in ("dtype", "D", "Sq", "lens", "q_lens"))
    B, sm = len(lens), D ** -0.5
    k, v = _same_kv(oracle, B, P_HKV, D, dtype, lens, 5)
    c8 = _fill(lb.LowbitKVCache(B, P_HKV, D, max(lens), TDT[dtype], dev, v_bits=8), k, v, lens, dtype, dev)
    q = _rand(oracle, np.random.default_rng(6), (B, P_HQ, Sq, D), dtype)
    q_i8, q_scale = pr.quant_q_blocks(oracle, q, q_lens, sm, 127)
    vhat = v8.dequant_v(oracle, c8.v.cpu().numpy(), c8.v_scale.cpu().numpy()).astype(np.float32)
    ref = types.SimpleNamespace(k_codes=c8.k_codes.cpu().numpy(), k_scale=c8.k_scale.cpu().numpy(), v=vhat, seqlens=np.array(lens))
    corr = kr.lse_correction(oracle, q, _np(c8.km), dtype)
    o_ref, lse2 = pr.oracle_prefill(oracle, q_i8, q_scale, ref, q_lens, causal=True, out_dtype=dtype)
    lse_ref = kr.natural_lse(lse2, corr, sm)
    lse_ref = np.where(np.isinf(lse2), -np.inf, lse_ref).astype(np.float32)
    for ns in (1, 3):
        o, lse = lb.lowbit_fa_prefill(_t(q, dtype, dev), c8, is_causal=True, return_lse=True, num_splits=ns,
                                      q_lens=torch.tensor(q_lens, dtype=torch.int32, device=dev))
        kr.check_o(_np(o), o_ref, dtype, f"prefill splits={ns}")
        kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, f"prefill splits={ns}")


# ------------------------------------------------------------------------------------------------------------------------
# 5. hostile memory
# ------------------------------------------------------------------------------------------------------------------------
HOSTILE_LENS = [1, 63, 64, 65, 130]


def _garbage(scale_fill):
    def fill(cache):
        """K: codes -128, scales +inf, tail NaN; V: the e4m3 NaN code 0xFF and NaN or +inf scales - everywhere, every page"""
        cache.k_codes.fill_(-128), cache.k_scale.fill_(float("inf")), cache.k_tail.fill_(float("nan"))
        cache.v.fill_(0xFF), cache.v_scale.fill_(scale_fill)
        return cache
    return fill


@pytest.mark.parametrize("dtype,D,scale_fill", [("fp16", 64, float("nan")), ("bf16", 128, float("inf")), ("fp16", 128, float("nan"))])
def test_fp8_cache_in_hostile_memory(oracle, dev, dtype, D, scale_fill):
    import lowbit_quant_fa2_paddle_amd as lb
    B, lens = len(HOSTILE_LENS), HOSTILE_LENS
    h8, _, hp8, _, rng = _quartet(lb, oracle, dev, B=B, Hkv=2, D=D, dtype=dtype, lens=lens, page=64, seed=51 + D, garbage=_garbage(scale_fill))
    clean, _, _, _, _ = _quartet(lb, oracle, dev, B=B, Hkv=2, D=D, dtype=dtype, lens=lens, page=64, seed=51 + D)
    what = f"hostile fp8 cache {dtype} D={D}"
    bad_scale = torch.isnan if scale_fill != scale_fill else torch.isinf
    for b, n in enumerate(lens):  # the valid rows are the clean cache's, the garbage behind them is still there
        same_bits(h8.v[b, :, :n], clean.v[b, :, :n], what + ": v codes")
        same_bits(h8.v_scale[b, :, :n], clean.v_scale[b, :, :n], what + ": v scales")
        assert torch.all(h8.v[b, :, n:] == 0xFF) and bad_scale(h8.v_scale[b, :, n:]).all(), (what, b)
        _, _, vc, vs = hp8.gather(b)
        same_bits(vc[:, :n], clean.v[b, :, :n], what + ": paged v codes")
        same_bits(vs[:, :n], clean.v_scale[b, :, :n], what + ": paged v scales")
        assert torch.all(vc[:, n:] == 0xFF) and bad_scale(vs[:, n:]).all(), (what, b)
    spare = torch.tensor(hp8.allocator.free_pages, device=dev)
    assert len(spare) and torch.all(hp8.v[spare] == 0xFF) and bad_scale(hp8.v_scale[spare]).all(), what
    for Sq, causal in ((1, False), (3, True)):
        tq = _t(_rand(oracle, rng, (B, 4, Sq, D), dtype), dtype, dev)
        for ns in (1, 3):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
            w = f"{what} decode Sq={Sq} splits={ns}"
            want = lb.lowbit_fa_decode(tq, clean, **kw)
            for cache in (h8, hp8):
                got = lb.lowbit_fa_decode(tq, cache, **kw)
                assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), w + ": a row behind the end of a sequence was read"
                same_bits(got, want, w)
    # prefill: 130 queries, ragged, over the same lengths (65 keys among them)
    tq = _t(_rand(oracle, rng, (B, 4, 130, D), dtype), dtype, dev)
    ql = torch.tensor([130, 1, 129, 65, 0], dtype=torch.int32, device=dev)
    for causal in (True, False):
        for ns in (1, 3):
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns, q_lens=ql)
            w = f"{what} prefill causal={causal} splits={ns}"
            want = lb.lowbit_fa_prefill(tq, clean, **kw)
            for cache in (h8, hp8):
                got = lb.lowbit_fa_prefill(tq, cache, **kw)
                assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), w + ": a row behind the end of a sequence was read"
                same_bits(got, want, w)


# ------------------------------------------------------------------------------------------------------------------------
# 6. containment: everything the append writes of V lies in [s0, end) of `v` and `v_scale`
# ------------------------------------------------------------------------------------------------------------------------
STATE = ("k_codes", "k_scale", "v", "v_scale", "k_tail", "km")
PAGED_STATE = STATE + ("seqlens", "block_table")
APPENDS = [(1, None), (63, None), (2, None), (200, [200, 7, 131])]  # T = 1; 63 then 2 (crossing a block); 200 with ragged new_lens
V_FILL, SCALE_FILL = 0x5A, 1234.5  # what rows nobody appended hold


def _arena_backed(cache, arena, names):
    for name in names:
        setattr(cache, name, arena.like(getattr(cache, name)))
    return cache


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_append_writes_only_its_rows(monkeypatch, oracle, dev, dtype, D):
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, cap = 3, 2, 320
    rng = np.random.default_rng(61 + D)
    arena = GuardArena(monkeypatch, dev)
    cache = _arena_backed(lb.LowbitKVCache(B, H, D, cap, TDT[dtype], dev, v_bits=8), arena, STATE)
    cache.v.fill_(V_FILL), cache.v_scale.fill_(SCALE_FILL)
    ref = v8.CacheRefV8(oracle, B, H, D, cap, dtype)
    ref.v_codes[:], ref.v_scale[:] = V_FILL, SCALE_FILL
    for T, lens in APPENDS:
        k, v = _rand(oracle, rng, (B, H, T, D), dtype, bias=0.5), _rand(oracle, rng, (B, H, T, D), dtype, mul=2.0)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        with arena:  # the mean's workspace of the first append
            cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=tl)
        ref.append(k, v, lens)
        torch.cuda.synchronize()
        arena.check()
        # EVERY byte of v and v_scale: rows in [s0, end) hold the model's row, all others what they held
        assert np.array_equal(cache.v.cpu().numpy(), ref.v_codes), (dtype, D, T, "v")
        assert np.array_equal(cache.v_scale.cpu().numpy().view(np.uint32), ref.v_scale.view(np.uint32)), (dtype, D, T, "v_scale")
        assert np.array_equal(cache.k_codes.cpu().numpy(), ref.k_codes), (dtype, D, T, "k_codes")


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_append_at_the_capacity_and_negative_lengths(monkeypatch, oracle, dev, dtype, D):
    """The siblings' defended cases (tests/test_gpu_hostile_memory.py), inside memory the test owns.  Capacity 128, device lengths
    [125, 128, 60] behind the host's back, T = 8: sequence 0 takes rows 125 .. 127 and drops five, sequence 1 none, sequence 2 all
    eight - unclipped, sequence 0 / 1 would write into the next (batch, head) slab of v and v_scale, behind the last of which lies
    the arena's guard.  Then lengths [-5, 0, 0] with new_lens [-1, 9, 3]: clamped to 0, 0, 0 and 0, 8, 3 new rows - unclamped, five
    rows before slab (0, 0): the guard in front."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, cap, T = 3, 2, 128, 8
    rng = np.random.default_rng(71 + D)
    mk = lambda T_: (_rand(oracle, rng, (B, H, T_, D), dtype, bias=0.5), _rand(oracle, rng, (B, H, T_, D), dtype, mul=2.0))
    (k0, v0), (k1, v1) = mk(60), mk(T)
    arena = GuardArena(monkeypatch, dev)
    cache = _arena_backed(lb.LowbitKVCache(B, H, D, cap, TDT[dtype], dev, v_bits=8), arena, STATE)
    ref = v8.CacheRefV8(oracle, B, H, D, cap, dtype)
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
        assert np.array_equal(cache.v.cpu().numpy(), ref.v_codes), (what, "v")
        assert np.array_equal(cache.v_scale.cpu().numpy().view(np.uint32), ref.v_scale.view(np.uint32)), (what, "v_scale")
        assert np.array_equal(cache.k_codes.cpu().numpy(), ref.k_codes), (what, "k_codes")
        assert np.array_equal(cache.k_scale.cpu().numpy().view(np.uint32), ref.k_scale.view(np.uint32)), (what, "k_scale")

    whole("at the capacity")
    assert ref.v_scale[0, :, 125:].all() and not ref.v_scale[1, :, 60:].any()  # not vacuous
    # negative lengths, on a fresh cache
    cache = _arena_backed(lb.LowbitKVCache(B, H, D, cap, TDT[dtype], dev, v_bits=8), arena, STATE)
    ref = v8.CacheRefV8(oracle, B, H, D, cap, dtype)
    cache.seqlens.copy_(torch.tensor([-5, 0, 0], dtype=torch.int32, device=dev))
    ref.seqlens[:] = [-5, 0, 0]
    new_lens = [-1, 9, 3]
    with arena:
        cache.append(_t(k1, dtype, dev), _t(v1, dtype, dev), new_lens=torch.tensor(new_lens, dtype=torch.int32, device=dev))
    ref.append(k1, v1, new_lens)
    torch.cuda.synchronize()
    arena.check()
    whole("negative lengths")
    assert not cache.v[0].any() and not cache.v_scale[0].any() and cache.v_scale[1, :, :8].all() and not cache.v_scale[1, :, 8:].any()


def _paged_v8_call(lib, name, cache, dev, dtype, **kw):
    """one call of a paged _v8 entry point by ctypes, every argument by keyword, in the order of include/lowbit_fa.h"""
    from lowbit_quant_fa2_paddle_amd import _lib
    order = {"lbfa_kvcache_paged_append_v8": ("k_new", "v_new", "dtype", "new_lens", "km", "k_codes", "k_scale", "v_cache", "v_scale",
                                              "k_tail", "seqlens", "block_table", "slots", "B", "Hkv", "T", "D", "num_slots",
                                              "num_pages", "page_size", "max_pages", "sk", "sv", "k_qmax", "stream"),
             "lbfa_decode_paged_v8": ("q", "dtype", "k_codes", "k_scale", "v_cache", "v_scale", "km", "seqlens", "block_table", "slots",
                                      "o", "lse", "workspace", "workspace_bytes", "B", "Hq", "Hkv", "Sq", "D", "num_slots", "num_pages",
                                      "page_size", "max_pages", "max_k", "num_splits", "sq", "so", "sm_scale", "q_qmax", "causal",
                                      "stream")}[name]
    args = dict(dtype=_lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16, km=cache.km.data_ptr(), k_codes=cache.k_codes.data_ptr(),
                k_scale=cache.k_scale.data_ptr(), v_cache=cache.v.data_ptr(), v_scale=cache.v_scale.data_ptr(),
                seqlens=cache.seqlens.data_ptr(), Hkv=cache.num_kv_heads, D=cache.padded_head_dim, num_slots=cache.max_seqs,
                num_pages=cache.num_pages, page_size=cache.page_size, max_pages=cache.max_pages_per_seq,
                stream=torch.cuda.current_stream(dev).cuda_stream)
    args.update(kw)
    assert set(args) == set(order), sorted(set(args) ^ set(order))
    vals = [_lib.strides3(args[k]) if isinstance(args[k], tuple) else args[k] for k in order]
    _lib.check(getattr(lib, name)(*vals), lib)


@pytest.mark.parametrize("dtype,D,page", [("fp16", 64, 64), ("bf16", 128, 128)])
def test_paged_append_skips_and_decode_clamps_corrupt_ids(monkeypatch, oracle, dev, dtype, D, page):
    """lbfa_kvcache_paged_append_v8 with slots [-1, 1, num_slots] and, under the blocks the append touches in slot 1's table, the
    pages -1 and num_pages + 1: rows 0 and 2 are skipped and so are both blocks of row 1 - pool, scales and guards stay as they
    were.  Unskipped, slot -1 / num_slots lies one slot before / behind the per-slot tensors and page -1 / num_pages + 1 at most
    two pages before / behind the pool tensors: the arena's guard (128 KiB; a page of codes is at most 2 x 128 x 128 = 32 KiB, of
    scales 1 KiB).  lbfa_decode_paged_v8 clamps the same ids: its result is that of slots [0, 1, num_slots - 1] and pages 0 and
    num_pages - 1."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    H, num_slots, max_pages, num_pages, T = 2, 3, 4, 14, 3 * page // 2
    rng = np.random.default_rng(81 + D)
    arena = GuardArena(monkeypatch, dev)
    cache = _arena_backed(lb.LowbitPagedKVCache(num_pages, page, H, D, num_slots, max_pages, TDT[dtype], dev, v_bits=8), arena, PAGED_STATE)
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
               sk=tuple(tk.stride()[:3]), sv=tuple(tv.stride()[:3]), k_qmax=127)
    _paged_v8_call(lib, "lbfa_kvcache_paged_append_v8", cache, dev, dtype, block_table=bad_table.data_ptr(), slots=bad_slots.data_ptr(), **app)
    torch.cuda.synchronize()
    arena.check()
    for name, t in state.items():
        same_bits(getattr(cache, name), t, f"corrupt ids {dtype} D={D}: {name} changed")

    # decode through the corrupt ids against decode through the clamped ones
    G, Sq = 2, 3
    tq = _t(_rand(oracle, rng, (num_slots, G * H, Sq, D), dtype), dtype, dev)

    def decode(slot_ids, pg1, pg2, ns):
        tb = cache.block_table.clone()
        tb[1, 0], tb[1, 1] = pg1, pg2
        tb, sl = arena.like(tb), arena.like(torch.tensor(slot_ids, dtype=torch.int32, device=dev))
        o, lse = arena.allocate((num_slots, G * H, Sq, D), TDT[dtype]), arena.allocate((num_slots, G * H, Sq), torch.float32)
        nbytes = lib.lbfa_decode_workspace_bytes(num_slots, G * H, H, Sq, cache.padded_head_dim, n0, ns)
        ws = arena.allocate((max(nbytes, 16),), torch.uint8)
        _paged_v8_call(lib, "lbfa_decode_paged_v8", cache, dev, dtype, q=tq.data_ptr(), block_table=tb.data_ptr(), slots=sl.data_ptr(),
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
    _paged_v8_call(lib, "lbfa_kvcache_paged_append_v8", cache, dev, dtype, block_table=sound.data_ptr(), slots=good.data_ptr(), **app)
    torch.cuda.synchronize()
    arena.check()
    assert not torch.equal(cache.v, state["v"]) and not torch.equal(_bits(cache.v_scale), _bits(state["v_scale"]))


# ------------------------------------------------------------------------------------------------------------------------
# 7. the front end
# ------------------------------------------------------------------------------------------------------------------------
def test_front_end(oracle, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 3"):
        lb.LowbitKVCache(1, 1, 64, 64, torch.float16, dev, v_bits=3)
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 3"):
        lb.LowbitPagedKVCache(2, 64, 1, 64, 1, 2, torch.float16, dev, v_bits=3)
    for cache in (lb.LowbitKVCache(2, 2, 64, 128, torch.float16, dev), lb.LowbitKVCache(2, 2, 64, 128, torch.float16, dev, v_bits=16),
                  lb.LowbitPagedKVCache(4, 64, 2, 64, 2, 2, torch.bfloat16, dev)):
        assert cache.v_bits == 16 and cache.v.dtype == torch.float16 and not hasattr(cache, "v_scale")
        assert cache.dequantized_v().dtype == torch.float16
    rng = np.random.default_rng(7)
    for dtype, D, k_bits in (("fp16", 80, 4), ("bf16", 128, 8)):  # k_bits and v_bits are independent
        v = _rand(oracle, rng, (2, 2, 100, D), dtype, mul=5.0)
        k = _rand(oracle, rng, (2, 2, 100, D), dtype)
        c = lb.LowbitKVCache(2, 2, D, 100, TDT[dtype], dev, k_bits=k_bits, v_bits=8).append(_t(k, dtype, dev), _t(v, dtype, dev))
        p = lb.LowbitPagedKVCache(4, 64, 2, D, 2, 2, TDT[dtype], dev, k_bits=k_bits, v_bits=8).append(_t(k, dtype, dev), _t(v, dtype, dev))
        assert c.k_qmax == (7 if k_bits == 4 else 127)
        vd = _np(c.dequantized_v())[:, :, :100]
        assert vd.shape == v.shape
        bound = v8.v_error_bound(v, c.v_scale.cpu().numpy()[:, :, :100])
        ratio = float((np.abs(vd.astype(np.float64) - v) / bound).max())
        print(f"dequantized_v {dtype} D={D}: worst element at {ratio:.3f} of the bound")
        assert ratio <= 1.0
        pd = p.dequantized_v()
        assert tuple(pd.shape) == (4, 2, 64, D)
        for b in range(2):
            rows = torch.cat([pd[pg] for pg in p.allocator.pages[b]], dim=1)[:, :100]
            same_bits(rows, c.dequantized_v()[b, :, :100], f"paged dequantized_v {dtype} sequence {b}")
        o8 = lb.lowbit_fa_decode(_t(k[:, :, :1].repeat(2, axis=1), dtype, dev), c)
        assert o8.shape == (2, 4, 1, D) and torch.isfinite(o8).all()
