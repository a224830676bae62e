"""CPU: the numpy model of the cached-prefill kernel (tests/prefill_reference.py `split_kv_prefill`: tile loop, key slices, combine)
against `oracle_prefill` on EVERY case of tests/test_gpu_prefill.py, at its slice counts - the bounds the GPU is held to
(`o_bound`, `lse_bound`, every element) are attainable at these shapes.  The worst ratios are printed (DESIGN.md section 3.10 records them)."""
import numpy as np
import pytest

import kvcache_reference as kr
import prefill_reference as pr


@pytest.mark.parametrize("case", pr.CASES + pr.SHORT_CASES, ids=pr.case_id)
def test_numpy_model_is_inside_the_bounds_on_every_gpu_case(oracle, case):
    c = pr.build_case(oracle, case)
    ref, dtype = c["ref"], case["dtype"]
    worst_o = worst_l = 0.0
    for causal in (False, True):
        o_ref, lse_ref = c["oracle"][causal]
        for ns in c["splits"]:
            eff = ns or pr.chosen_splits(case["Sq"], max(int(c["lens"].max()), 1))
            o, lse2 = pr.split_kv_prefill(oracle, c["q_i8"], c["q_scale"], ref.k_codes, ref.k_scale, ref.v, c["lens"], c["q_lens"],
                                          causal=causal, num_splits=eff, out_dtype=dtype)
            what = f"{pr.case_id(case)} causal={causal} splits={ns}"
            worst_o = max(worst_o, kr.check_o(o, o_ref, dtype, what))
            worst_l = max(worst_l, kr.check_lse(kr.natural_lse(lse2, c["corr"], c["sm_scale"]), lse_ref, c["corr"], c["sm_scale"],
                                                dtype, what))
            for b in range(pr.shape_of(case)[0]):  # rows past q_lens: exactly zeros and -inf
                assert np.all(o[b, :, c["q_lens"][b]:] == 0) and np.all(np.isneginf(lse2[b, :, c["q_lens"][b]:])), what
    print(f"{pr.case_id(case)}: worst O ratio {worst_o:.3f}, worst LSE ratio {worst_l:.3f}")


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_numpy_model_is_inside_the_bounds_on_the_containment_shapes(oracle, dtype, D):
    """the hostile-memory cases of tests/test_gpu_prefill_containment.py: 5 sequences of 1, 63, 64, 65 and 130 keys (70 rows, then the
    rest), Sq 130 with q_lens [130, 1, 129, 0, 77], 1 and 3 slices, both masks"""
    lens, q_lens, Sq, H, G = np.array(pr.CONTAINMENT_LENS), pr.CONTAINMENT_Q_LENS, pr.CONTAINMENT_SQ, 2, 2
    rng = np.random.default_rng(D)
    mk = lambda h, rows, bias: oracle.to_storage(rng.standard_normal((len(lens), h, rows, D), dtype=np.float32) + np.float32(bias), dtype)
    q, k, v = mk(H * G, Sq, 0.0), mk(H, 130, 0.5), mk(H, 130, 0.0)
    ref = kr.CacheRef(oracle, len(lens), H, D, 192, dtype)
    ref.append(k[:, :, :70], v[:, :, :70], np.minimum(lens, 70))
    ref.append(k[:, :, 70:], v[:, :, 70:], np.maximum(lens - 70, 0))
    sm = D ** -0.5
    q_i8, q_scale = pr.quant_q_blocks(oracle, q, q_lens, sm, 127)
    corr = kr.lse_correction(oracle, q, ref.km, dtype)
    for causal in (False, True):
        o_ref, lse2_ref = pr.oracle_prefill(oracle, q_i8, q_scale, ref, q_lens, causal=causal, out_dtype=dtype)
        for ns in (1, 3):
            o, lse2 = pr.split_kv_prefill(oracle, q_i8, q_scale, ref.k_codes, ref.k_scale, ref.v, lens, q_lens, causal=causal,
                                          num_splits=ns, out_dtype=dtype)
            what = f"containment {dtype} D={D} causal={causal} splits={ns}"
            kr.check_o(o, o_ref, dtype, what)
            kr.check_lse(kr.natural_lse(lse2, corr, sm), kr.natural_lse(lse2_ref, corr, sm), corr, sm, dtype, what)


def test_one_uniform_append_gives_the_dense_operators_codes(oracle):
    """Sq == Sk after one uniform append: the Q codes and scales are `per_block_int8`'s, i.e. the dense operator's"""
    rng = np.random.default_rng(5)
    q = oracle.to_storage(rng.standard_normal((2, 4, 200, 64), dtype=np.float32), "fp16")
    k = oracle.to_storage(rng.standard_normal((2, 2, 200, 64), dtype=np.float32), "fp16")
    codes, scale = pr.quant_q_blocks(oracle, q, [200, 200], 0.125, 127)
    q_i8, q_scale, _, _ = oracle.per_block_int8(q, k, None, 0.125, "fp16", amax_floor=1e-7)
    assert np.array_equal(codes, q_i8) and np.array_equal(scale.view(np.uint32), q_scale.view(np.uint32))


def test_split_rule_model():
    assert pr.chosen_splits(128, 321) == 1 and pr.chosen_splits(1, 4096, batch=1, hq=32) == 16
    assert pr.chosen_splits(8192, 131072, batch=1, hq=32) == 1 and pr.chosen_splits(128, 1 << 20, batch=1, hq=1) == 256
