"""GPU tests of the int8 KV cache (`LowbitKVCache`, lbfa_kvcache_append) and of split-KV decode attention (`lowbit_fa_decode`,
lbfa_decode).

* the cache after ANY sequence of appends holds, for every valid key, the codes and scales of the dense K quantiser on the
  concatenated K (bit for bit), and V as its fp16 cast;
* decode equals the oracle's int8 / fp16 kernel on the cache's codes (tests/kvcache_reference.py `oracle_decode`) within the
  operator bound of tests/test_gpu_parity.py: |dO| <= 2e-3 + 2e-3 |O| (+ 2^-7 |O| for bf16), LSE within 1e-3 + one storage ulp of
  the smooth-K correction;
* after a prefill only, decode of one query agrees with the dense operator at Sq = 1.
Shapes are the smallest that reach every path: 1 / 2 / 4 row blocks, both head dims, a padded one, ragged lengths with 0, 1,
< 64, = 0 and != 0 mod 64, 1 / 2 / 7 / chosen key slices - and ONE long context (131072 keys), where the slices are many.
"""
import numpy as np
import pytest

import kvcache_reference as kr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


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


def _rand(orc, rng, shape, dtype, dist, bias=0.0):
    x = rng.standard_normal(shape, dtype=np.float32) if dist == "normal" else rng.integers(-100, 100, shape).astype(np.float32)
    return orc.to_storage(x + np.float32(bias), dtype)


def _nhd(t):
    """the same values behind an NHD view: [B, H, T, D] -> [B, T, H, D] contiguous"""
    return t.transpose(1, 2).contiguous()


def _check_cache(orc, cache, k_all, v_all, dtype, qmax, what):
    codes_d, scale_d, v_d = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy(), _np(cache.v)
    km = _np(cache.km) if cache.km is not None else None
    lens = cache.seqlens.cpu().numpy()
    for b in range(len(k_all)):
        n = k_all[b].shape[1]
        assert lens[b] == n, (what, b, lens[b], n)
        if n == 0:
            continue
        codes, scales = kr.dense_k_codes(orc, k_all[b][None], None if km is None else km[b:b + 1], dtype, qmax)
        assert np.array_equal(codes_d[b, :, :n], codes[0]), (what, b, "codes")
        assert np.array_equal(scale_d[b, :, :(n + 63) // 64].view(np.uint32), scales[0].view(np.uint32)), (what, b, "scales")
        assert np.array_equal(v_d[b, :, :n], v_all[b].astype(np.float16).astype(np.float32)), (what, b, "v")


# ------------------------------------------------------------------------------------------------------------------------
# 4. the cache equals the dense quantiser
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k_bits,D,smooth", [("fp16", 8, 64, True), ("bf16", 4, 128, True), ("fp16", 4, 128, False),
                                                   ("bf16", 8, 64, True)])
def test_cache_equals_dense_quantiser_after_every_append(oracle, dev, dtype, k_bits, D, smooth):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(11 + D + k_bits)
    B, H, qmax = 3, 2, 127 if k_bits == 8 else 7
    cache = lb.LowbitKVCache(B, H, D, 600, TDT[dtype], dev, k_bits=k_bits, smooth_k=smooth)
    assert cache.capacity == 640
    k_all = [np.zeros((H, 0, D), np.float32) for _ in range(B)]
    v_all = [np.zeros((H, 0, D), np.float32) for _ in range(B)]
    steps = [(70, None), (1, [1, 1, 0]), (1, [1, 0, 1]), (63, [63, 10, 0]), (64, [64, 64, 33]), (65, [0, 65, 64]), (200, [200, 1, 150])]
    for step, (T, lens) in enumerate(steps):
        k = _rand(oracle, rng, (B, H, T, D), dtype, "normal", bias=0.5)
        v = _rand(oracle, rng, (B, H, T, D), dtype, "normal")
        tk, tv = _t(k, dtype, dev), _t(v, dtype, dev)
        tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        if step % 2:
            cache.append(_nhd(tk), _nhd(tv), tensor_layout="NHD", new_lens=tl)
        else:
            cache.append(tk, tv, new_lens=tl)
        for b in range(B):
            tb = T if lens is None else lens[b]
            k_all[b] = np.concatenate([k_all[b], k[b, :, :tb]], axis=1)
            v_all[b] = np.concatenate([v_all[b], v[b, :, :tb]], axis=1)
        if step == 0 and smooth:  # the mean of a uniform prefill is the dense operators' mean, bit for bit
            assert np.array_equal(_np(cache.km), oracle.mean_seq(k, dtype)[:, :, 0])
        _check_cache(oracle, cache, k_all, v_all, dtype, qmax, f"step {step}")
    assert cache.max_seqlen == sum(T for T, _ in steps)
    # the debugging aid: codes * scale + km is K up to half a quantisation step and the storage rounding of K - km (half an ulp)
    kd = _np(cache.dequantized_k())
    step_sz = cache.k_scale.cpu().numpy().repeat(64, axis=2)[..., None]
    km_abs = np.abs(_np(cache.km))[:, :, None, :] if smooth else np.zeros((B, H, 1, D), np.float32)
    half_ulp = 2.0 ** -11 if dtype == "fp16" else 2.0 ** -8
    for b in range(B):
        n = k_all[b].shape[1]
        bound = 0.5 * step_sz[b, :, :n] + half_ulp * (np.abs(k_all[b]) + km_abs[b]) + 1e-6
        assert np.all(np.abs(kd[b, :, :n] - k_all[b]) <= bound)
    with pytest.raises(ValueError, match="capacity"):
        cache.append(tk, tv)


def test_ragged_first_append_takes_the_mean_of_its_valid_rows(oracle, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(3)
    B, H, D, T, dtype = 4, 2, 80, 150, "fp16"  # a padded head dim: only the new tokens are padded
    lens = [150, 0, 1, 97]
    k = _rand(oracle, rng, (B, H, T, D), dtype, "normal", bias=-0.25)
    v = _rand(oracle, rng, (B, H, T, D), dtype, "normal")
    cache = lb.LowbitKVCache(B, H, D, 256, TDT[dtype], dev)
    cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=torch.tensor(lens, dtype=torch.int32, device=dev))
    ref = kr.CacheRef(oracle, B, H, 128, 256, dtype)
    pad = lambda a: np.pad(a, [(0, 0)] * 3 + [(0, 128 - D)])
    ref.append(pad(k), pad(v), lens)
    assert np.array_equal(_np(cache.km), ref.km)
    assert np.array_equal(cache.seqlens.cpu().numpy(), ref.seqlens)
    for b, n in enumerate(lens):
        assert np.array_equal(cache.k_codes.cpu().numpy()[b, :, :n], ref.k_codes[b, :, :n])
        assert np.array_equal(cache.k_scale.cpu().numpy()[b, :, :(n + 63) // 64], ref.k_scale[b, :, :(n + 63) // 64])
        assert np.array_equal(_np(cache.v)[b, :, :n], ref.v[b, :, :n])
    # one more token each: the open blocks are re-quantised from the tail
    k1, v1 = _rand(oracle, rng, (B, H, 1, D), dtype, "normal"), _rand(oracle, rng, (B, H, 1, D), dtype, "normal")
    cache.append(_t(k1, dtype, dev), _t(v1, dtype, dev))
    ref.append(pad(k1), pad(v1))
    for b, n in enumerate(ref.seqlens):
        assert np.array_equal(cache.k_codes.cpu().numpy()[b, :, :n], ref.k_codes[b, :, :n])
        assert np.array_equal(cache.k_scale.cpu().numpy()[b, :, :(n + 63) // 64], ref.k_scale[b, :, :(n + 63) // 64])


# ------------------------------------------------------------------------------------------------------------------------
# 5. decode equals the oracle
# ------------------------------------------------------------------------------------------------------------------------
def _decode_case(orc, dev, *, Sq, G, Hkv, D, layout, dtype, dist, lens, q_bits=8, k_bits=8, splits=(1, 2, 7, 0), seed=0,
                 causal_modes=(False, True), smooth_k=True, sm_scale=None):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(seed)
    B, Hq, T = len(lens), G * Hkv, max(lens)
    Dp = 64 if D <= 64 else 128
    scale_arg, sm_scale = sm_scale, D ** -0.5 if sm_scale is None else sm_scale
    cache = lb.LowbitKVCache(B, Hkv, D, T, TDT[dtype], dev, k_bits=k_bits, smooth_k=smooth_k)
    k = _rand(orc, rng, (B, Hkv, T, D), dtype, dist, bias=0.5 if dist == "normal" else 0.0)
    v = _rand(orc, rng, (B, Hkv, T, D), dtype, "normal")
    # a prefill, then the rest token by chunk, so the open-block path feeds the decode too
    t0 = max(1, T // 2)
    lens = np.array(lens)
    cache.append(_t(k[:, :, :t0], dtype, dev), _t(v[:, :, :t0], dtype, dev), new_lens=torch.tensor(np.minimum(lens, t0), dtype=torch.int32, device=dev))
    if T > t0:
        cache.append(_t(k[:, :, t0:], dtype, dev), _t(v[:, :, t0:], dtype, dev),
                     new_lens=torch.tensor(np.maximum(lens - t0, 0), dtype=torch.int32, device=dev))
    assert np.array_equal(cache.seqlens.cpu().numpy(), lens)
    q = _rand(orc, rng, (B, Hq, Sq, D), dtype, dist)
    tq = _t(q, dtype, dev)
    if layout == "NHD":
        tq = _nhd(tq)
    # the reference: the oracle's kernel on the cache's own codes (their equality with the dense quantiser is tested above)
    qp = np.pad(q, [(0, 0)] * 3 + [(0, Dp - D)])
    q_i8, q_scale = kr.quant_q(orc, qp, sm_scale, 127 if q_bits == 8 else 7)
    k_i8, k_scale, v16 = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy(), _np(cache.v)
    corr = kr.lse_correction(orc, qp, _np(cache.km) if smooth_k else None, dtype)
    worst = 0.0
    for causal in causal_modes:
        o_ref, lse2_ref = kr.oracle_decode(orc, q_i8, q_scale, k_i8, k_scale, v16, lens, causal=causal, out_dtype=dtype)
        lse_ref = kr.natural_lse(lse2_ref, corr, sm_scale)
        for ns in splits:
            what = f"Sq{Sq} G{G} D{D} {layout} {dtype} {dist} causal={causal} splits={ns}"
            o, lse = lb.lowbit_fa_decode(tq, cache, tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns,
                                         q_bits=q_bits, sm_scale=scale_arg)
            assert o.shape == tq.shape and o.dtype == tq.dtype and tuple(lse.shape) == (B, Hq, Sq)
            on = _np(o if layout == "HND" else o.transpose(1, 2))
            worst = max(worst, kr.check_o(on, o_ref[..., :D], dtype, what))
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm_scale, dtype, what)
            dead = np.isinf(lse_ref)
            assert np.all(on[dead] == 0), what  # no visible key: zeros
            o2, lse2 = lb.lowbit_fa_decode(tq, cache, tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns,
                                           q_bits=q_bits, sm_scale=scale_arg)
            assert torch.equal(o, o2) and torch.equal(lse, lse2), what + ": two runs differ"
            o3 = lb.lowbit_fa_decode(tq, cache, tensor_layout=layout, is_causal=causal, num_splits=ns, q_bits=q_bits, sm_scale=scale_arg)
            assert torch.equal(o, o3), what + ": O depends on return_lse"
    return worst


DECODE_CASES = [
    dict(Sq=1, G=8, Hkv=2, D=128, layout="HND", dtype="fp16", dist="normal", lens=[0, 1, 63, 640, 333]),
    dict(Sq=4, G=4, Hkv=2, D=64, layout="NHD", dtype="fp16", dist="randint", lens=[0, 1, 50, 128, 321]),
    dict(Sq=16, G=1, Hkv=3, D=64, layout="HND", dtype="bf16", dist="normal", lens=[5, 64, 200]),
    dict(Sq=16, G=4, Hkv=1, D=128, layout="HND", dtype="fp16", dist="normal", lens=[130, 700]),        # 64 rows: 4 row blocks
    dict(Sq=1, G=4, Hkv=2, D=80, layout="NHD", dtype="fp16", dist="normal", lens=[77, 300]),           # padded head dim
    dict(Sq=4, G=8, Hkv=1, D=128, layout="NHD", dtype="bf16", dist="randint", lens=[257, 64]),         # 32 rows: 2 row blocks
    dict(Sq=16, G=4, Hkv=1, D=64, layout="HND", dtype="fp16", dist="randint", lens=[449, 2]),          # 64 rows at D = 64
    dict(Sq=1, G=1, Hkv=2, D=64, layout="HND", dtype="fp16", dist="normal", lens=[192, 65], q_bits=4, k_bits=4),
    # geometries of tests/decode_fuzz_cases.py `PINNED`: rows that are no power of two
    dict(Sq=5, G=4, Hkv=2, D=128, layout="HND", dtype="fp16", dist="normal", lens=[449, 2]),           # 20 rows: head 3 in two row blocks
    dict(Sq=5, G=7, Hkv=1, D=64, layout="NHD", dtype="bf16", dist="normal", lens=[449, 2], smooth_k=False),   # 35 rows: 3 row blocks
    dict(Sq=3, G=16, Hkv=1, D=128, layout="HND", dtype="fp16", dist="normal", lens=[449, 1], sm_scale=0.2, k_bits=4),  # 48 rows
]


@pytest.mark.parametrize("case", DECODE_CASES, ids=lambda c: f"Sq{c['Sq']}G{c['G']}D{c['D']}{c['layout']}{c['dtype']}{c['dist']}")
def test_decode_equals_oracle(oracle, dev, case):
    _decode_case(oracle, dev, seed=17, **case)


def test_decode_long_context(oracle, dev):
    """131072 keys, one sequence: 2048 tiles in 256 chosen slices (and in one) against the oracle's single pass"""
    from lowbit_quant_fa2_paddle_amd import _lib
    assert _lib.load().lbfa_decode_num_splits(1, 1, 131072) == 256
    _decode_case(oracle, dev, Sq=1, G=8, Hkv=1, D=128, layout="HND", dtype="fp16", dist="normal", lens=[131072], splits=(0, 1),
                 seed=5, causal_modes=(False,))


# ------------------------------------------------------------------------------------------------------------------------
# 6. end to end: prefill into the cache, one query - the dense operator at Sq = 1
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,Hq,Hkv", [("fp16", 128, 8, 2), ("bf16", 64, 4, 4)])
def test_decode_after_prefill_agrees_with_dense_operator(oracle, dev, dtype, D, Hq, Hkv):
    import lowbit_quant_fa2_paddle_amd as lb
    B, T = 2, 777
    q, k, v = oracle.make_inputs(B, Hq, 1, D, seed=9, dtype=dtype, Hkv=Hkv, Sk=T, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    cache = lb.LowbitKVCache(B, Hkv, D, T, TDT[dtype], dev).append(tk, tv)
    # km, hence every K code, is the dense operator's
    km = oracle.mean_seq(k, dtype)
    assert np.array_equal(_np(cache.km), km[:, :, 0])
    codes, scales = kr.dense_k_codes(oracle, k, km[:, :, 0], dtype, 127)
    assert np.array_equal(cache.k_codes.cpu().numpy()[:, :, :T], codes)
    assert np.array_equal(cache.k_scale.cpu().numpy()[:, :, :(T + 63) // 64], scales)
    o_ref, lse_ref = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, return_lse=True)
    corr = kr.lse_correction(oracle, q, km[:, :, 0], dtype)
    for ns in (0, 1, 3):
        o, lse = lb.lowbit_fa_decode(tq, cache, return_lse=True, num_splits=ns)
        kr.check_o(_np(o), _np(o_ref), dtype, f"vs dense operator, splits={ns}")
        kr.check_lse(lse.cpu().numpy(), lse_ref.cpu().numpy(), corr, D ** -0.5, dtype, f"vs dense operator, splits={ns}")


def test_front_end_refusals(dev):
    import lowbit_quant_fa2_paddle_amd as lb
    cache = lb.LowbitKVCache(1, 1, 64, 64, torch.float16, dev)
    kv = torch.zeros(1, 1, 8, 64, dtype=torch.float16, device=dev)
    cache.append(kv, kv)
    with pytest.raises(ValueError, match="the limit is 64"):
        lb.lowbit_fa_decode(torch.zeros(1, 5, 13, 64, dtype=torch.float16, device=dev), cache)
    with pytest.raises(RuntimeError, match="forward-only"):
        lb.lowbit_fa_decode(torch.zeros(1, 1, 1, 64, dtype=torch.float16, device=dev, requires_grad=True), cache)
    with torch.no_grad():
        o = lb.sageattn_decode(torch.zeros(1, 1, 1, 64, dtype=torch.float16, device=dev, requires_grad=True), cache)
    assert o.shape == (1, 1, 1, 64) and not o.requires_grad
    with pytest.raises(ValueError, match="dtype of the cache"):
        cache.append(kv.bfloat16(), kv.bfloat16())
