"""The decode fuzz without a GPU: what its cases cover, and that the unchanged operator bounds are attainable on them.

* Census: over the default range (`PINNED` + seeds 0 ... 31) every kernel instance, every geometry edge and every option occurs.
  The conditions are the point - a generator that misses one is changed, not the condition.
* The reference alone: for every such case the numpy cache (`CacheRef`) after the case's append schedule holds the dense
  quantiser's codes and scales bit for bit, and the numpy model of the kernel (`split_kv_decode`) at the case's three slice
  counts lies inside `o_bound` / `lse_bound` of `oracle_decode` on every element.  So the GPU test asks nothing of the kernel
  that plain fp32 arithmetic in the kernel's order does not deliver.
* The fp8 twin (`v_bits = 8`) of every case: `CacheRefV8` after the same schedule holds `quant_v_rows`' codes and scales and the
  same K state, and the numpy model on V^ lies inside the same bounds of the oracle on V^.
"""
import numpy as np
import pytest

import decode_fuzz_cases as fz
import kvcache_reference as kr
import v8_reference as v8

CASES = fz.default_cases()


def test_census_of_the_default_range():
    strata = {(c["dtype"], c["Dp"], c["mb"]) for c in CASES}
    assert strata == {(t, d, m) for t in ("fp16", "bf16") for d in (64, 128) for m in (1, 2, 3, 4)}
    assert sum(fz.straddles(c) for c in CASES) >= 8
    assert sum(max(c["splits"]) > 256 for c in CASES) >= 2
    assert sum(any(fz.combine_run(c, s) > 8 and fz.combine_run(c, s) % 8 for s in c["splits"]) for c in CASES) >= 2
    assert {(c["q_bits"], c["k_bits"]) for c in CASES} == {(8, 8), (4, 4), (8, 4), (4, 8)}
    assert any(not c["smooth_k"] for c in CASES) and any(c["sm_scale"] is not None for c in CASES)
    assert any(0 in c["lens"] for c in CASES)
    assert any(n and n % 64 == 0 for c in CASES for n in c["lens"])
    assert any(fz.has_blind_rows(c) for c in CASES)
    assert any(c["q_view"] is not None and any(c["q_view"]) for c in CASES)
    assert any(a["packed"] for c in CASES for a in c["appends"])
    assert {c["page"] for c in CASES} == set(fz.PAGES)
    # the schedules: 1 ... 4 appends, single-token ones, uniform and ragged first appends, both layouts
    assert {len(c["appends"]) for c in CASES} >= {1, 2, 3, 4}
    assert any(a["T"] == 1 for c in CASES for a in c["appends"])
    assert {c["appends"][0]["new_lens"] is None for c in CASES} == {True, False}
    assert {a["layout"] for c in CASES for a in c["appends"]} == {"HND", "NHD"}
    assert {c["is_causal"] for c in CASES} == {True, False} and {c["return_lse"] for c in CASES} == {True, False}
    assert len({c["name"] for c in CASES}) == len(CASES)


def test_pinned_cases_are_the_geometry_edges():
    geo = {(c["Sq"], c["G"]) for c in fz.PINNED}
    assert geo >= {(5, 4), (5, 7), (7, 6), (3, 16), (7, 9), (13, 1), (11, 3)}
    assert any(not c["smooth_k"] for c in fz.PINNED) and any(c["sm_scale"] == 0.2 for c in fz.PINNED)
    assert {(8, 4), (4, 8)} <= {(c["q_bits"], c["k_bits"]) for c in fz.PINNED}
    assert any(c["dtype"] == "bf16" and (c["q_bits"], c["k_bits"]) == (4, 4) and c["Sq"] > 1 for c in fz.PINNED)
    for s in (22, 300):
        assert {c["Dp"] for c in fz.PINNED if s in c["splits"]} == {64, 128}
    assert {c["dtype"] for c in fz.PINNED} == {"fp16", "bf16"}
    # a slice past the 256th that holds keys: one tile per slice, more than 256 tiles
    assert any(max(c["splits"]) > 256 and -(-max(c["lens"]) // 64) > 256 for c in fz.PINNED)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_numpy_kernel_model_within_the_bounds_on_every_case(oracle, case):
    """Worst element over the default range (`PINNED` + seeds 0 ... 31, three slice counts each): O at 0.698 of `o_bound`
    (seed11, bf16; the worst pinned case is mb3-M35 at 300 slices, 0.657), LSE at 0.001 of `lse_bound`."""
    c = case
    q, kv = fz.make_data(oracle, c)
    ref = fz.replay(oracle, c, kv)
    # the stateful append against the dense quantiser on the concatenated K
    for b, (k_all, v_all) in enumerate(fz.concatenated(c, kv)):
        n = k_all.shape[1]
        assert n == c["lens"][b]
        if n == 0:
            continue
        km = None if ref.km is None else ref.km[b:b + 1]
        codes, scales = kr.dense_k_codes(oracle, fz._pad(k_all[None], c), km, c["dtype"], fz.k_qmax(c))
        assert np.array_equal(ref.k_codes[b, :, :n], codes[0]), (c["name"], b)
        assert np.array_equal(ref.k_scale[b, :, :(n + 63) // 64].view(np.uint32), scales[0].view(np.uint32)), (c["name"], b)
        assert np.array_equal(ref.v[b, :, :n, :c["D"]], v_all.astype(np.float16).astype(np.float32))
    # the kernel's arithmetic against the oracle's
    o_ref, lse_ref, corr = fz.decode_reference(oracle, c, ref, q)
    q_i8, q_scale = fz.quantised_q(oracle, c, q)
    sm = fz.sm_scale_of(c)
    dead = fz.blind_rows(c)
    assert np.array_equal(np.isinf(lse_ref), dead)
    for ns in c["splits"]:
        what = f"{c['name']} splits={ns}"
        o, lse2 = kr.split_kv_decode(oracle, q_i8, q_scale, ref.k_codes, ref.k_scale, ref.v, ref.seqlens, causal=c["is_causal"],
                                     num_splits=ns or fz.chosen_splits(c), out_dtype=c["dtype"])
        kr.check_o(o[..., :c["D"]], o_ref, c["dtype"], what)
        kr.check_lse(kr.natural_lse(lse2, corr, sm), lse_ref, corr, sm, c["dtype"], what)
        assert np.all(o[dead] == 0) and not np.isnan(o).any(), what


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_numpy_kernel_model_within_the_bounds_on_the_fp8_twin(oracle, case):
    """The same cases read through an fp8 V cache: model and oracle both on V^.  Worst element over the default range: O at 0.712
    of `o_bound` (seed11, bf16; 0.698 on the fp16 V), LSE at 0.001 of `lse_bound`."""
    c = case
    q, kv = fz.make_data(oracle, c)
    ref = fz.replay(oracle, c, kv, new=fz.new_ref_v8)
    plain = fz.replay(oracle, c, kv)
    for name in ("k_codes", "k_scale", "v", "seqlens"):  # everything but V's format is the fp16-V cache's
        assert np.array_equal(getattr(ref, name), getattr(plain, name)), (c["name"], name)
    for b, (_, v_all) in enumerate(fz.concatenated(c, kv)):
        n = v_all.shape[1]
        if n:
            codes, scales = v8.quant_v_rows(oracle, v_all, c["dtype"])
            assert np.array_equal(ref.v_codes[b, :, :n, :c["D"]], codes) and not ref.v_codes[b, :, :n, c["D"]:].any(), (c["name"], b)
            assert np.array_equal(ref.v_scale[b, :, :n].view(np.uint32), scales.view(np.uint32)), (c["name"], b)
    vhat = ref.vhat()
    o_ref, lse_ref, corr = fz.decode_reference(oracle, c, ref, q, v=vhat)
    q_i8, q_scale = fz.quantised_q(oracle, c, q)
    sm = fz.sm_scale_of(c)
    dead = fz.blind_rows(c)
    assert np.array_equal(np.isinf(lse_ref), dead)
    for ns in c["splits"]:
        what = f"{c['name']} fp8 V splits={ns}"
        o, lse2 = kr.split_kv_decode(oracle, q_i8, q_scale, ref.k_codes, ref.k_scale, vhat, ref.seqlens, causal=c["is_causal"],
                                     num_splits=ns or fz.chosen_splits(c), out_dtype=c["dtype"])
        kr.check_o(o[..., :c["D"]], o_ref, c["dtype"], what)
        kr.check_lse(kr.natural_lse(lse2, corr, sm), lse_ref, corr, sm, c["dtype"], what)
        assert np.all(o[dead] == 0) and not np.isnan(o).any(), what
