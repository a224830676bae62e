"""The numpy restatement of the KV cache and of split-KV decode (tests/kvcache_reference.py) against the existing oracle, on
the CPU: the stateful append equals the dense quantiser bit for bit, and the split-KV arithmetic stays within the operator
bound of the oracle's kernel - so the GPU tests may use either as their reference."""
import numpy as np
import pytest

import kvcache_reference as kr


def _inputs(orc, rng, shape, dtype, dist):
    x = rng.standard_normal(shape, dtype=np.float32) if dist == "normal" else rng.integers(-100, 100, shape).astype(np.float32)
    return orc.to_storage(x, dtype)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("qmax", [127, 7])
def test_stateful_append_equals_dense_quantiser(oracle, dtype, qmax):
    rng = np.random.default_rng(5 + qmax)
    B, H, D, cap = 3, 2, 64, 640
    cache = kr.CacheRef(oracle, B, H, D, cap, dtype, qmax=qmax, smooth_k=True)
    k_all = [np.zeros((H, 0, D), np.float32) for _ in range(B)]
    v_all = [np.zeros((H, 0, D), np.float32) for _ in range(B)]
    chunks = [70, 1, 1, 63, 64, 65, 200, 5, 130]
    for step, T in enumerate(chunks):
        k = _inputs(oracle, rng, (B, H, T, D), dtype, "normal") + np.float32(0.5)
        k = oracle.to_storage(k, dtype)
        v = _inputs(oracle, rng, (B, H, T, D), dtype, "normal")
        lens = None if step == 0 else rng.integers(0, T + 1, B)
        if lens is not None and step % 2:
            lens[step % B] = 0  # a sequence that takes nothing this step
        cache.append(k, v, lens)
        for b in range(B):
            tb = T if lens is None else int(lens[b])
            k_all[b] = np.concatenate([k_all[b], k[b, :, :tb]], axis=1)
            v_all[b] = np.concatenate([v_all[b], v[b, :, :tb]], axis=1)
        for b in range(B):
            n = k_all[b].shape[1]
            assert cache.seqlens[b] == n
            if n == 0:
                continue
            codes, scales = kr.dense_k_codes(oracle, k_all[b][None], cache.km[b:b + 1], dtype, qmax)
            assert np.array_equal(cache.k_codes[b, :, :n], codes[0]), (step, b)
            assert np.array_equal(cache.k_scale[b, :, :(n + 63) // 64].view(np.uint32), scales[0].view(np.uint32)), (step, b)
            assert np.array_equal(cache.v[b, :, :n], v_all[b].astype(np.float16).astype(np.float32))
    # the mean of the first (uniform) append is the dense operators' mean
    k0 = np.stack([k_all[b][:, :chunks[0]] for b in range(B)])
    assert np.array_equal(cache.km, oracle.mean_seq(k0, dtype)[:, :, 0])


def test_append_without_smoothing_and_all_zero_block(oracle):
    cache = kr.CacheRef(oracle, 1, 1, 64, 128, "fp16", smooth_k=False)
    k = np.zeros((1, 1, 70, 64), np.float32)
    cache.append(k, k)
    codes, scales = kr.dense_k_codes(oracle, k, None, "fp16", 127)
    assert np.array_equal(cache.k_codes[:, :, :70], codes) and np.array_equal(cache.k_scale, scales)  # the 1e-7 floor


DECODE_CASES = [
    # Sq, G, Hkv, D, lens, dist
    (1, 8, 1, 128, [4133, 63], "normal"),
    (4, 4, 2, 64, [700, 0, 1], "normal"),
    (16, 1, 2, 64, [64, 129, 640], "randint"),
    (3, 2, 1, 128, [1000, 5], "randint"),
]


@pytest.mark.parametrize("Sq,G,Hkv,D,lens,dist", DECODE_CASES)
@pytest.mark.parametrize("causal", [False, True])
def test_split_kv_restatement_within_operator_bound_of_oracle(oracle, Sq, G, Hkv, D, lens, dist, causal):
    rng = np.random.default_rng(Sq * 100 + G)
    B, Hq, dtype = len(lens), G * Hkv, "fp16"
    cap = (max(lens) + 63) // 64 * 64
    sm_scale = D ** -0.5
    cache = kr.CacheRef(oracle, B, Hkv, D, cap, dtype)
    T = max(lens)
    cache.append(_inputs(oracle, rng, (B, Hkv, T, D), dtype, dist), _inputs(oracle, rng, (B, Hkv, T, D), dtype, "normal"),
                 np.array(lens))
    q = _inputs(oracle, rng, (B, Hq, Sq, D), dtype, dist)
    q_i8, q_scale = kr.quant_q(oracle, q, sm_scale, 127)
    o_ref, lse_ref = kr.oracle_decode(oracle, q_i8, q_scale, cache.k_codes, cache.k_scale, cache.v, cache.seqlens, causal=causal,
                                      out_dtype=dtype)
    for splits in (1, 2, 7):
        o, lse2 = kr.split_kv_decode(oracle, q_i8, q_scale, cache.k_codes, cache.k_scale, cache.v, cache.seqlens, causal=causal,
                                     num_splits=splits, out_dtype=dtype)
        kr.check_o(o, o_ref, dtype, f"splits={splits}")
        kr.check_lse(kr.natural_lse(lse2, None, sm_scale), kr.natural_lse(lse_ref, None, sm_scale), None, sm_scale, dtype,
                     f"splits={splits}")
        # rows that see no key: zeros and -inf
        n = np.array(lens)[:, None] - (Sq - 1 - np.arange(Sq))[None, :] * int(causal)
        dead = np.broadcast_to((n <= 0)[:, None, :], lse2.shape)
        assert np.all(np.isinf(lse2[dead])) and np.all(o[dead] == 0) and np.all(np.isfinite(lse2[~dead]))
