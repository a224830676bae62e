"""CPU tests of the oracle's chosen-block paths (`q_blocks`): the long-sequence GPU tests check sampled 128-row Q blocks only,
so the oracle run on those blocks has to give exactly the bits of the same rows of a full run - O, LSE and the fp8 flip slack -
for every operator family, causal or not, GQA, fp16 / bf16, a ragged last block, and per-block key-tile order for fp8."""
import numpy as np
import pytest


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max diff {np.abs(a - b).max():.3e}"


def _rows(x, rows, layout):
    return x[:, rows] if layout == "NHD" else x[:, :, rows]


S = 1000  # 7 whole blocks + a ragged one of 104 rows
BLOCK_SETS = [[0], [7], [0, 3, 7], [2, 5], [1, 2, 3, 4, 5, 6, 7]]


@pytest.mark.parametrize("pv,q_qmax,k_qmax", [("fp16", 127.0, 127.0), ("fp16", 7.0, 7.0), ("fp8", 127.0, 127.0)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,layout,H,Hkv,D", [("fp16", "HND", 2, 2, 64), ("bf16", "NHD", 4, 2, 128)])
def test_chosen_blocks_equal_rows_of_a_full_run(oracle, pv, q_qmax, k_qmax, causal, dtype, layout, H, Hkv, D):
    q, k, v = oracle.make_inputs(1, H, S, D, seed=7, layout=layout, dtype=dtype, Hkv=Hkv, k_bias=0.5)
    kw = dict(dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True, q_qmax=q_qmax, k_qmax=k_qmax, pv=pv,
              tail="neg_inf", amax_floor=1e-7)
    if pv == "fp8":
        kw["return_slack"] = True
    full = oracle.lowbit_fa_forward(q, k, v, **kw)
    for blocks in BLOCK_SETS:
        rows = oracle.block_rows(blocks, S)
        part = oracle.lowbit_fa_forward(_rows(q, rows, layout), k, v, q_blocks=blocks, **kw)
        for f, p in zip(full[:-1], part[:-1]):  # o (and the slack): layout-shaped
            _same(_rows(f, rows, layout), p)
        _same(full[-1][:, :, rows], part[-1])   # lse [B, H, S]


@pytest.mark.parametrize("causal", [False, True])
def test_chosen_blocks_of_the_exact_attention(oracle, causal):
    q, k, v = oracle.make_inputs(1, 4, S, 64, seed=8, Hkv=2, k_bias=0.5)
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    o, lse = oracle.sdpa_naive(q, k, v, is_causal=causal, sm_scale=0.125, return_lse=True)
    for blocks in BLOCK_SETS:
        rows = oracle.block_rows(blocks, S)
        po, plse = oracle.sdpa_naive(q[:, :, rows], k, v, is_causal=causal, sm_scale=0.125, return_lse=True, q_blocks=blocks)
        # the same rows of the same row-wise arithmetic: equal up to the summation order of the matrix products
        np.testing.assert_allclose(po, o[:, :, rows], rtol=0, atol=1e-12)
        np.testing.assert_allclose(plse, lse[:, :, rows], rtol=0, atol=1e-12)
    if causal:  # the mask follows the absolute rows: row r of block 7 sees keys 0..r, not 0..(r - 896)
        r = oracle.block_rows([7], S)
        po = oracle.sdpa_naive(q[:, :, r], k, v, is_causal=True, sm_scale=0.125, q_blocks=[7])
        assert not np.allclose(po, oracle.sdpa_naive(q[:, :, r], k[:, :, :len(r)], v[:, :, :len(r)], is_causal=True, sm_scale=0.125))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_fp8_key_tile_order_per_block(oracle, dtype):
    """fp8: the key-tile direction is a property of the Q block (`(qt // 64) & 1` in the kernel).  Mixed per-block flags must give,
    block by block, the rows of the full run that walks that way - with and without `q_blocks`."""
    q, k, v = oracle.make_inputs(1, 2, S, 64, seed=9, dtype=dtype, k_bias=0.5)
    kw = dict(dtype=dtype, return_lse=True, pv="fp8", amax_floor=1e-7, return_slack=True)
    fwd = oracle.lowbit_fa_forward(q, k, v, fp8_key_tiles_reversed=False, **kw)
    rev = oracle.lowbit_fa_forward(q, k, v, fp8_key_tiles_reversed=True, **kw)
    # the two orders must differ somewhere, or this test would not see a swapped flag
    assert not np.array_equal(fwd[1], rev[1])
    flags = [b % 3 == 1 for b in range(8)]
    mixed = oracle.lowbit_fa_forward(q, k, v, fp8_key_tiles_reversed=flags, **kw)
    for blocks in ([1, 2, 7], [0, 4], [4, 7]):
        rows = oracle.block_rows(blocks, S)
        part = oracle.lowbit_fa_forward(q[:, :, rows], k, v, q_blocks=blocks, fp8_key_tiles_reversed=[flags[b] for b in blocks], **kw)
        for b in blocks:
            br = oracle.block_rows([b], S)
            pr = np.searchsorted(rows, br)
            want = rev if flags[b] else fwd
            for w, m, p in zip(want, mixed, part):
                _same(w[:, :, br], m[:, :, br])
                _same(w[:, :, br], p[:, :, pr])
    with pytest.raises(AssertionError):
        oracle.lowbit_fa_forward(q, k, v, fp8_key_tiles_reversed=[True, False], **kw)


def test_block_rows_and_misuse(oracle):
    assert oracle.block_rows([0, 7], S).tolist() == list(range(128)) + list(range(896, 1000))
    q, k, v = oracle.make_inputs(1, 1, S, 64, seed=1)
    with pytest.raises(AssertionError):  # 130 rows are more than the one block they are said to be
        oracle.lowbit_fa_forward(q[:, :, :130], k, v, q_blocks=[0])
    with pytest.raises(AssertionError):  # blocks must be ascending
        oracle.lowbit_fa_forward(q[:, :, :256], k, v, q_blocks=[3, 1])
