"""The numpy model of the fp8 V cache (tests/v8_reference.py): the row quantiser meets the error bound of include/lowbit_fa.h
on distributions that stress it, never reaches the range where an e4m3 conversion would have to saturate, and - a row depending
on nothing but itself - gives the same state for any append schedule."""
import numpy as np
import pytest

import v8_reference as v8

ROWS, D = 256, 128


def _dist(name, rng):
    if name == "normal":
        return rng.standard_normal((ROWS, D), dtype=np.float32)
    if name == "small":
        return np.float32(1e-3) * rng.standard_normal((ROWS, D), dtype=np.float32)
    if name == "randint":
        return rng.integers(-100, 100, (ROWS, D)).astype(np.float32)
    if name == "lognormal":  # a wide spread of magnitudes inside one row, clipped into the fp16 range
        x = np.exp(rng.normal(0.0, 4.0, (ROWS, D))) * rng.choice([-1.0, 1.0], (ROWS, D))
        return np.clip(x, -60000.0, 60000.0).astype(np.float32)
    if name == "outlier":  # one 60000 among 1e-4 values: everything else lands in the e4m3 subnormals or at zero
        x = np.float32(1e-4) * rng.standard_normal((ROWS, D), dtype=np.float32)
        x[np.arange(ROWS), rng.integers(0, D, ROWS)] = 60000.0
        return x
    raise ValueError(name)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("dist", ["normal", "small", "randint", "lognormal", "outlier"])
def test_quantiser_meets_the_error_bound(oracle, dist, dtype):
    rng = np.random.default_rng(len(dist) * 7 + len(dtype))
    x = oracle.to_storage(_dist(dist, rng), dtype)
    codes, scale = v8.quant_v_rows(oracle, x, dtype)
    assert codes.dtype == np.uint8 and scale.dtype == np.float32 and codes.shape == x.shape and scale.shape == (ROWS,)
    y = v8.scaled(oracle, x, dtype)
    worst_y = float(np.abs(y).max())
    print(f"{dist} {dtype}: worst |x / scale| = {worst_y:.5f}")
    assert worst_y < 464.0  # the last value that still rounds to 448: no conversion depends on saturation
    assert not np.any((codes & 0x7F) == 0x7F)  # no NaN code
    vhat = v8.dequant_v(oracle, codes, scale).astype(np.float64)
    err = np.abs(vhat - x.astype(np.float64))
    ratio = float((err / v8.v_error_bound(x, scale)).max())
    print(f"{dist} {dtype}: worst element at {ratio:.3f} of the bound")
    assert ratio <= 1.0
    # the row maximum is kept to one rounding of 448 * scale
    assert np.all(np.abs(vhat).max(axis=-1) >= np.abs(x).max(axis=-1) * (1 - 2.0 ** -10))


def test_zero_row_and_round_trip(oracle):
    codes, scale = v8.quant_v_rows(oracle, np.zeros((3, 64), np.float32), "fp16")
    assert not codes.any() and np.all(scale == np.float32(1e-7) / np.float32(448.0))
    assert not v8.dequant_v(oracle, codes, scale).any()
    # every finite e4m3 pattern survives decode -> encode, and a row of them with amax 448 (scale 1) is kept exactly
    pats = np.array([p for p in range(256) if (p & 0x7F) != 0x7F], np.uint8)
    vals = oracle.e4m3fn_decode(pats)
    back = oracle.e4m3fn_encode(vals)
    assert np.array_equal(back[vals != 0], pats[vals != 0]) and np.all(oracle.e4m3fn_decode(back) == vals)
    row = np.resize(vals, (2, 256)).astype(np.float32)
    codes, scale = v8.quant_v_rows(oracle, row, "fp16")
    assert np.all(scale == 1.0) and np.array_equal(oracle.e4m3fn_decode(codes), row)
    assert np.array_equal(v8.dequant_v(oracle, codes, scale).astype(np.float32), row)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_any_append_schedule_gives_the_one_shot_state(oracle, dtype):
    rng = np.random.default_rng(5)
    B, H, Dh, cap = 3, 2, 64, 448
    steps = [(70, None), (1, [1, 1, 0]), (1, [1, 0, 1]), (63, [63, 10, 0]), (64, [64, 64, 33]), (65, [0, 65, 64]), (200, [200, 1, 150])]
    ref = v8.CacheRefV8(oracle, B, H, Dh, cap, dtype)
    k_all = [np.zeros((H, 0, Dh), np.float32) for _ in range(B)]
    v_all = [np.zeros((H, 0, Dh), np.float32) for _ in range(B)]
    for T, lens in steps:
        k = oracle.to_storage(rng.standard_normal((B, H, T, Dh), dtype=np.float32), dtype)
        v = oracle.to_storage(rng.standard_normal((B, H, T, Dh), dtype=np.float32) * np.float32(rng.uniform(0.01, 30)), dtype)
        ref.append(k, v, lens)
        for b in range(B):
            tb = T if lens is None else lens[b]
            k_all[b] = np.concatenate([k_all[b], k[b, :, :tb]], axis=1)
            v_all[b] = np.concatenate([v_all[b], v[b, :, :tb]], axis=1)
    for b in range(B):
        n = v_all[b].shape[1]
        assert ref.seqlens[b] == n
        one = v8.CacheRefV8(oracle, 1, H, Dh, cap, dtype)
        one.km = ref.km[b:b + 1]  # the mean belongs to the first append of the schedule
        one.append(k_all[b][None], v_all[b][None])
        assert np.array_equal(one.v_codes[0, :, :n], ref.v_codes[b, :, :n])
        assert np.array_equal(one.v_scale[0, :, :n].view(np.uint32), ref.v_scale[b, :, :n].view(np.uint32))
        assert np.array_equal(one.k_codes[0, :, :n], ref.k_codes[b, :, :n])  # and the K side is CacheRef's
        assert not ref.v_codes[b, :, n:].any() and not ref.v_scale[b, :, n:].any()
        codes, scale = v8.quant_v_rows(oracle, v_all[b], dtype)
        assert np.array_equal(codes, ref.v_codes[b, :, :n]) and np.array_equal(scale, ref.v_scale[b, :, :n])
