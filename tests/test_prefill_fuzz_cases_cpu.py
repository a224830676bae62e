"""The prefill fuzz without a GPU: what its cases cover, and that the unchanged operator bounds are attainable on them.

* Census: over the default range (`PINNED` + seeds 0 ... 23) every kernel instance, every edge of head geometry, Q blocks, key
  tiles, slices and pages, and every option occurs.  The conditions are the point - a generator that misses one is changed, not
  the condition.
* The reference alone: for every such case the numpy cache (`CacheRef` / `CacheRefV8`) after the case's append schedule holds the
  dense quantiser's codes and scales bit for bit (and, with an fp8 V cache, `quant_v_rows`' codes and scales), and the numpy
  model of the kernel (`split_kv_prefill`) at the case's three slice counts lies inside `check_o` / `check_lse` of
  `oracle_prefill` on every element, for both masks and at every step at which the case calls the operator.  With an fp8 V cache
  both read V^.  So the GPU test asks nothing of the kernel that plain fp32 arithmetic in the kernel's order does not deliver.
"""
import numpy as np
import pytest

import kvcache_reference as kr
import prefill_fuzz_cases as pz
import prefill_reference as pr
import v8_reference as v8

CASES = pz.default_cases()
PINNED = {c["name"]: c for c in pz.PINNED}


def test_census_of_the_default_range():
    # kernel instances: (dtype, padded head dim, v_bits); each case runs contiguous and paged, causal and not
    assert {(c["dtype"], c["Dp"], c["v_bits"]) for c in CASES} == {(t, d, v) for t in ("fp16", "bf16") for d in (64, 128) for v in (16, 8)}
    # head geometry
    assert {c["B"] for c in CASES} == {1, 2, 3} and {c["Hkv"] for c in CASES} == {1, 2, 3}
    assert {c["G"] for c in CASES} >= {1, 2, 3, 4, 5, 8}
    assert any(c["G"] == 1 and c["Hkv"] == 3 for c in CASES) and any(c["G"] == 8 for c in CASES)
    assert any(c["G"] >= 3 and c["Hkv"] >= 2 and c["B"] >= 2 for c in CASES)
    assert {d for dims in pz.HEAD_DIMS.values() for d in dims} == {c["D"] for c in CASES}
    assert {c["D"] for c in CASES if c["v_bits"] == 8} == {d for dims in pz.HEAD_DIMS.values() for d in dims}
    # Q blocks
    assert {pr.q_blocks(c) for c in CASES} >= {1, 2, 3, 4}
    assert sum(pr.blocks_see_different_tiles(c) >= 3 for c in CASES) >= 3
    assert any(pr.slice_count_between_first_and_last_block(c) for c in CASES)
    assert any(pr.empty_middle_block_next_to_a_full_one(c) for c in CASES)
    assert any(pz.decode_takes_it(c) for c in CASES) and sum(c["Sq"] * c["G"] <= 64 for c in CASES) >= 2
    # q_lens: None, 0, a cut inside a 16-row block, at a wave's 32-row edge, at a Q block's edge, whole trailing blocks
    assert any(c["q_lens_arg"] is None for c in CASES)
    assert set().union(*(pr.q_len_cuts(c) for c in CASES)) == {"zero", "row16", "wave", "block", "trailing"}
    # key tiles and slices: up to 12 tiles, slices of 5 tiles and more (three trips of the look-ahead loop and a ragged end),
    # n - q_len on both sides of a tile edge, blind causal rows, a sequence without keys
    assert max(pr.visible_tiles(c, b, 0, False) for c in CASES if c["name"].startswith("seed") for b in range(c["B"])) >= 11
    assert sum(pr.longest_slice(c) >= 5 for c in CASES) >= 5 and any(pr.longest_slice(c) % 2 for c in CASES)
    assert set().union(*(pr.key_offset_to_tile_edge(c) for c in CASES)) >= {63, 0, 1}
    assert any(pr.fewer_keys_than_queries(c) for c in CASES) and any(pr.no_keys_next_to_a_full_sequence(c) for c in CASES)
    assert any(pr.slice_starts_on_odd_tile_inside_page(c) for c in CASES)
    assert any(pr.combine_second_trip(c) for c in CASES)
    assert sum(max(c["splits"]) > 256 for c in CASES) >= 2 and any(0 in c["splits"] for c in CASES)
    assert {s for c in CASES for s in c["splits"]} >= set(pz.SPLIT_CHOICES)
    # pages
    assert {c["page"] for c in CASES} == set(pz.PAGES)
    assert any(pr.page_192_with_ragged_tiles_and_odd_tps(c) for c in CASES)
    assert any(c["page"] == 256 and max(c["lens"]) > 256 for c in CASES)
    assert any(c["num_slots"] > c["B"] for c in CASES) and any(c["slots"] != sorted(c["slots"]) for c in CASES)
    # data and options
    assert {(c["q_bits"], c["k_bits"]) for c in CASES} == {(8, 8), (4, 4), (8, 4), (4, 8)}
    assert {c["dist"] for c in CASES} == {"normal", "randint"}
    assert any(c["dist"] == "randint" and c["smooth_k"] for c in CASES)
    assert any(not c["smooth_k"] for c in CASES) and any(c["smooth_k"] and c["sm_scale"] is not None for c in CASES)
    assert {c["k_bias"] for c in CASES} >= {0.0, 0.3, -0.5}
    assert sum(c["q_view"] is not None and any(c["q_view"]) for c in CASES) >= 4
    assert {c["q_layout"] for c in CASES} == {"HND", "NHD"} and {c["return_lse"] for c in CASES} == {True, False}
    # the schedules: 1 ... 4 appends, uniform and ragged first appends, both layouts, packed views, chunked use
    assert {len(c["appends"]) for c in CASES} >= {1, 2, 3, 4}
    assert {c["appends"][0]["new_lens"] is None for c in CASES} == {True, False}
    assert {a["layout"] for c in CASES for a in c["appends"]} == {"HND", "NHD"}
    assert any(a["packed"] for c in CASES for a in c["appends"])
    assert sum(len(c["calls"]) > 1 for c in CASES) >= 2
    # the size every drawn case keeps
    for c in CASES:
        if c["name"].startswith("seed"):
            assert c["B"] * c["G"] * c["Hkv"] * c["Sq"] <= pz.MAX_ROWS and max(c["lens"]) <= pz.MAX_KEYS, c["name"]
    assert len({c["name"] for c in CASES}) == len(CASES)


def test_pinned_cases_are_the_edges():
    c = PINNED["four-q-blocks"]
    assert pr.q_blocks(c) == 4 and pr.slice_count_between_first_and_last_block(c)
    assert (pr.visible_tiles(c, 0, 0), pr.visible_tiles(c, 0, 3)) == (7, 12) and 9 in c["splits"]
    assert pr.empty_middle_block_next_to_a_full_one(PINNED["empty-middle-blocks"])
    assert PINNED["G8"]["G"] == 8 and (PINNED["G1-Hkv3"]["G"], PINNED["G1-Hkv3"]["Hkv"]) == (1, 3)
    c = PINNED["combine-second-trip"]
    assert pr.combine_second_trip(c) and c["Sq"] == 129 and c["lens"] == [300 * 64 - 19] and c["splits"] == [300, 257, 1]
    assert c["dist"] == "randint" and c["page"] == 256
    c = PINNED["page192-odd-tps"]
    assert pr.page_192_with_ragged_tiles_and_odd_tps(c) and pr.slice_starts_on_odd_tile_inside_page(c)
    assert pr.no_keys_next_to_a_full_sequence(PINNED["no-keys-next-to-full"])
    assert pr.fewer_keys_than_queries(PINNED["fewer-keys-than-queries"])
    assert PINNED["chunked"]["calls"] == [0, 1, 2] and pz.decode_takes_it(PINNED["decode-sized"])
    assert {c["D"] for c in pz.PINNED if c["v_bits"] == 8} == {d for dims in pz.HEAD_DIMS.values() for d in dims}
    assert any(c["smooth_k"] and c["sm_scale"] is not None for c in pz.PINNED)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_numpy_kernel_model_within_the_bounds_on_every_case(oracle, case):
    """Worst element over the default range (`PINNED` + seeds 0 ... 23, three slice counts, both masks, every call step): O at
    0.759 of `o_bound` (seed15, bf16, integer data; the worst pinned case is fewer-keys-than-queries, bf16, 0.758), LSE at 0.001 of
    `lse_bound`.  No drawn case had to be changed to fit."""
    c = case
    q, kv = pz.make_data(oracle, c)
    ref = pz.new_ref(oracle, c)
    sm, dtype = pz.sm_scale_of(c), c["dtype"]
    worst_o = worst_l = 0.0
    for step, (k, v) in enumerate(kv):
        pz.ref_append(oracle, c, ref, step, k, v)
        if step not in c["calls"]:
            continue
        lens = pz.lens_after(c, step)
        assert list(ref.seqlens) == lens
        # the kernel's arithmetic against the oracle's, both on the V a reader sees
        want, corr = pz.prefill_reference(oracle, c, ref, q)
        _, q_i8, q_scale = pz.quantised_q(oracle, c, q)
        v_read = pr.oracle_state(ref).v
        for causal in (False, True):
            o_ref, lse_ref = want[causal]
            dead = pz.dead_rows(c, lens, causal)
            assert np.array_equal(np.isinf(lse_ref), dead), (c["name"], step, causal)
            for ns in c["splits"]:
                what = f"{c['name']} step={step} causal={causal} splits={ns}"
                o, lse2 = pr.split_kv_prefill(oracle, q_i8, q_scale, ref.k_codes, ref.k_scale, v_read, ref.seqlens, c["q_lens"],
                                              causal=causal, num_splits=pr.effective_splits(c, ns), out_dtype=dtype)
                worst_o = max(worst_o, kr.check_o(o[..., :c["D"]], o_ref, dtype, what))
                worst_l = max(worst_l, kr.check_lse(kr.natural_lse(lse2, corr, sm), lse_ref, corr, sm, dtype, what))
                assert np.all(o[dead] == 0) and np.all(np.isneginf(lse2[dead])) and not np.isnan(o).any(), what
    assert list(ref.seqlens) == c["lens"]
    # the stateful append against the dense quantisers on the concatenated K and V
    for b, (k_all, v_all) in enumerate(pz.concatenated(c, kv)):
        n = k_all.shape[1]
        assert n == c["lens"][b]
        if n == 0:
            continue
        km = None if ref.km is None else ref.km[b:b + 1]
        codes, scales = kr.dense_k_codes(oracle, np.pad(k_all[None], [(0, 0)] * 3 + [(0, c["Dp"] - c["D"])]), km, dtype,
                                         127 if c["k_bits"] == 8 else 7)
        assert np.array_equal(ref.k_codes[b, :, :n], codes[0]), (c["name"], b)
        assert np.array_equal(ref.k_scale[b, :, :(n + 63) // 64].view(np.uint32), scales[0].view(np.uint32)), (c["name"], b)
        assert np.array_equal(ref.v[b, :, :n, :c["D"]], v_all.astype(np.float16).astype(np.float32))
        if c["v_bits"] == 8:
            vc, vs = v8.quant_v_rows(oracle, v_all, dtype)
            assert np.array_equal(ref.v_codes[b, :, :n, :c["D"]], vc) and not ref.v_codes[b, :, :n, c["D"]:].any(), (c["name"], b)
            assert np.array_equal(ref.v_scale[b, :, :n].view(np.uint32), vs.view(np.uint32)), (c["name"], b)
    print(f"{c['name']}: worst O ratio {worst_o:.3f}, worst LSE ratio {worst_l:.3f}")
