"""The numpy model of the nibble-packed K cache (tests/k4_reference.py): the layout pinned by one hand-written row, a round trip
over every pair of nibbles, the quantiser's range with qmax 7, and a reader of the packed state giving what the byte cache gives."""
import numpy as np
import pytest

import k4_reference as k4
import kvcache_reference as kr
import prefill_reference as pr


def test_layout_is_pinned_by_one_row():
    # byte j: channel 2 j in bits 0..3, channel 2 j + 1 in bits 4..7, two's complement nibbles
    row = np.array([1, 2, -1, 0, 7, -7, 0, -1, -3, 5, 6, -6], np.int8)
    want = np.array([0x21, 0x0F, 0x97, 0xF0, 0x5D, 0xA6], np.uint8)
    assert np.array_equal(k4.pack(row), want)
    assert np.array_equal(k4.unpack(want), row)
    assert np.array_equal(k4.unpack(np.array([0x88, 0x80, 0x08], np.uint8)), np.array([-8, -8, 0, -8, -8, 0], np.int8))
    assert k4.pack(np.zeros((2, 3, 8), np.int8)).shape == (2, 3, 4) and k4.unpack(np.zeros((2, 3, 4), np.uint8)).dtype == np.int8
    with pytest.raises(AssertionError):
        k4.pack(np.array([8, 0], np.int8))


def test_round_trip_over_all_nibble_pairs():
    lo, hi = np.meshgrid(np.arange(-7, 8), np.arange(-7, 8), indexing="ij")
    codes = np.stack([lo.ravel(), hi.ravel()], axis=-1).astype(np.int8)  # [225, 2]
    packed = k4.pack(codes)
    assert packed.shape == (225, 1) and len(set(packed.ravel().tolist())) == 225
    assert np.array_equal(packed[:, 0], (lo.ravel() & 15) | ((hi.ravel() & 15) << 4))
    assert np.array_equal(k4.unpack(packed), codes)
    assert not np.any((packed & 0x0F) == 8) and not np.any((packed >> 4) == 8)  # no -8 in either half
    # and every byte survives unpack -> pack, the two -8s included
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(k4.pack(k4.unpack(every)), every)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_the_quantiser_with_qmax_7_never_emits_minus_8(oracle, dtype):
    rng = np.random.default_rng(11)
    ref = k4.CacheRefK4(oracle, 2, 2, 64, 320, dtype)
    for T, mul in ((70, 1.0), (1, 100.0), (63, 1e-3), (130, 5.0)):
        k = oracle.to_storage(rng.standard_normal((2, 2, T, 64), dtype=np.float32) * np.float32(mul) + np.float32(0.5), dtype)
        k[0, 0, 0, :2] = (-60000.0, 60000.0) if T == 1 else k[0, 0, 0, :2]  # an extreme of either sign in one block
        ref.append(k, k)
        assert ref.k_codes.min() >= -7 and ref.k_codes.max() <= 7
    assert ref.k_codes.min() == -7 and ref.k_codes.max() == 7
    assert np.array_equal(k4.unpack(ref.k_packed), ref.k_codes) and ref.k_packed.shape == (2, 2, 320, 32)
    # block by block the codes are the dense quantiser's with qmax 7 (what `k_bits=4` means everywhere else)
    one = k4.CacheRefK4(oracle, 1, 1, 64, 64, dtype, smooth_k=False)
    k = oracle.to_storage(rng.standard_normal((1, 1, 64, 64), dtype=np.float32), dtype)
    one.append(k, k)
    dense, scale = kr.dense_k_codes(oracle, k, None, dtype, 7)
    assert np.array_equal(one.k_codes, dense) and np.array_equal(one.k_scale.view(np.uint32), scale.view(np.uint32))


def test_a_reader_of_the_packed_state_gives_what_the_byte_cache_gives(oracle):
    dtype, B, Hkv, G, D, lens = "fp16", 2, 2, 2, 64, [130, 65]
    rng = np.random.default_rng(4)
    ref = k4.CacheRefK4(oracle, B, Hkv, D, 192, dtype)
    k = oracle.to_storage(rng.standard_normal((B, Hkv, 130, D), dtype=np.float32) + np.float32(0.5), dtype)
    v = oracle.to_storage(rng.standard_normal((B, Hkv, 130, D), dtype=np.float32), dtype)
    ref.append(k, v, lens)
    sm = D ** -0.5
    q = oracle.to_storage(rng.standard_normal((B, G * Hkv, 3, D), dtype=np.float32), dtype)
    q_i8, q_scale = kr.quant_q(oracle, q, sm, 127)
    for causal in (False, True):
        want = kr.oracle_decode(oracle, q_i8, q_scale, ref.k_codes, ref.k_scale, ref.v, np.array(lens), causal=causal, out_dtype=dtype)
        got = k4.oracle_decode(oracle, q_i8, q_scale, ref.k_packed, ref.k_scale, ref.v, np.array(lens), causal=causal, out_dtype=dtype)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    q = oracle.to_storage(rng.standard_normal((B, G * Hkv, 70, D), dtype=np.float32), dtype)
    q_lens = [70, 33]
    q_i8, q_scale = pr.quant_q_blocks(oracle, q, q_lens, sm, 7)
    want = pr.oracle_prefill(oracle, q_i8, q_scale, ref, q_lens, causal=True, out_dtype=dtype)
    got = k4.oracle_prefill(oracle, q_i8, q_scale, ref.k_packed, ref.k_scale, ref.v, ref.seqlens, q_lens, causal=True, out_dtype=dtype)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.isfinite(got[0]).all()
