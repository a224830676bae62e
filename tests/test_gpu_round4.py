"""GPU parity tests added in round 4 (run with `-m gpu`).

  * SHORT Q blocks on purpose (2, 3, 4 full key tiles; the first Q blocks of a causal sequence): the overflow votes of the lazy
    pass sit on the tiles' own barriers, and a vote that every wave does not see the same way makes the workgroup's waves take
    different paths - a round-3 experiment ("vote on the last tile's barrier") produced run-to-run different outputs for Q blocks
    of exactly two tiles and was caught by accident.  Here: first fp16-P overflow in tile 1 or 2, for all rows / one wave / one
    row, every case run TWICE (bit-equal outputs and LSEs), then against the oracle.  The reference makes one deterministic pass
    (src/triton/attn_qk_int8_per_block.py:45-65).
  * run-to-run bit-stability at the C2 size on the reference's bench distribution (every Q block replays);
  * the replay that is NOT caused by an overflow: softmax references far from zero (|m| > 2^7 binades) leave the rounded-scale
    grid (attn_fwd16.hip, kGridRef) - large common-mode scores that never overflow the lazy pass;
  * the un-quantised bf16 kernel with a 120-binade step: bf16 P does not overflow where fp16 P does, the vote has to come from
    the size of the row sums (attn_fwd16.hip, wave_overflowed).
"""
import numpy as np
import pytest

from test_gpu_round3 import _np, _o_close, _shifted_inputs, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _run_twice(fn):
    a = fn()
    torch.cuda.synchronize()
    b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"two runs of the same launch differ in {(x != y).sum().item()} elements"
    return a


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rows", ["all", "one_wave", "one_row"])
@pytest.mark.parametrize("S,first_high_tile", [(128, 1), (192, 1), (192, 2), (256, 1), (256, 2)])
def test_short_q_blocks_vote_deterministically(oracle, dev, D, rows, S, first_high_tile):
    """Non-causal, n_main = S / 64 = 2, 3, 4 full tiles (no vote inside the loop for 2; one at tile 2 for 3 and 4), the overflow
    in the second or third tile."""
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = _shifted_inputs(oracle, 256, D, first_high_tile, rows, False, seed=31)
    q, k, v = q[:, :, :S], k[:, :, :S], v[:, :, :S]
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, return_lse=True, smooth_k=False))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, return_lse=True, smooth_k=False, amax_floor=1e-7, tail="neg_inf")
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rows", ["all", "one_wave", "one_row"])
@pytest.mark.parametrize("first_high_tile", [1, 2, 3])
def test_first_q_blocks_of_a_causal_sequence(oracle, dev, D, rows, first_high_tile):
    """Causal S = 512: Q blocks with 0, 2, 4, 6 full tiles in front of their two diagonal tiles; the step sits in tile 1, 2 or 3,
    i.e. inside the full tiles of the later blocks and inside the masked diagonal tiles of the earlier ones."""
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = _shifted_inputs(oracle, 512, D, first_high_tile, rows, False, seed=32)
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, is_causal=True, return_lse=True, smooth_k=False))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=True, return_lse=True, smooth_k=False, amax_floor=1e-7, tail="neg_inf")
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("api", ["int8", "int4", "fp8"])
def test_run_to_run_bit_stability_randint_c2_size(dev, api):
    """B4 H32 S4096 D64 on q, k = randint(-100, 100) (utils/benchmark.py:215-230): every one of the 4096 Q blocks leaves the lazy
    pass at its first vote and replays; three launches, identical bits."""
    import lowbit_quant_fa2_paddle_amd as lb
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    q = torch.randint(-100, 100, (4, 32, 4096, 64), generator=g, device=dev).half()
    k = torch.randint(-100, 100, (4, 32, 4096, 64), generator=g, device=dev).half()
    v = torch.randn((4, 32, 4096, 64), generator=g, device=dev).half()
    fn = {"int8": lb.lowbit_fa_qk_int8_pv_fp16_triton, "int4": lb.lowbit_fa_qk_int4_pv_fp16_triton,
          "fp8": lb.lowbit_fa_qk_int8_pv_fp8_cuda}[api]
    kw = {} if api == "fp8" else {"return_lse": True}
    outs = []
    for _ in range(3):
        r = fn(q, k, v, **kw)
        outs.append(r if isinstance(r, tuple) else (r,))
    torch.cuda.synchronize()
    for r in outs[1:]:
        for x, y in zip(outs[0], r):
            assert torch.isfinite(x).all() and torch.equal(x, y)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_large_common_mode_scores_replay_without_overflow(oracle, dev, D, causal, sign):
    """q = a u + N(0,1), k = +-a u + N(0,1), no smoothing: every score carries +-a^2 / sqrt(D) ~ +-290 binades and the rows are
    as flat as N(0,1) rows - nothing overflows the lazy pass, but a scale rounded by 2^-19 would move the exponents by 290 * 2^-19
    ~ 2^-11 *per key block*, differently from tile to tile.  The waves vote for the replay because their references left the
    grid's range, and the replay dequantises exactly."""
    import lowbit_quant_fa2_paddle_amd as lb
    S = 640
    q, k, v = oracle.make_inputs(1, 2, S, D, seed=41)
    rng = np.random.default_rng(9)
    u = rng.standard_normal(D).astype(np.float32)
    u /= np.linalg.norm(u)
    a = 40.0 * (D / 64.0) ** 0.25
    # key blocks of different magnitude: different k_scale per tile
    k = k * np.repeat(rng.uniform(0.5, 2.0, S // 64), 64).astype(np.float32)[None, None, :, None]
    q = oracle.to_storage(q + a * u, "fp16")
    k = oracle.to_storage(k + sign * a * u, "fp16")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, is_causal=causal, return_lse=True, smooth_k=False))
    o_ref, lse_ref, mid = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, smooth_k=False, amax_floor=1e-7,
                                                   tail="neg_inf", return_intermediates=True)
    assert np.abs(lse_ref).max() * 1.44269504 > 150.0, "the case must leave the grid's range"
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("late_tile", [1, 5])
def test_bf16_kernel_120_binade_step(oracle, dev, D, late_tile):
    """Un-quantised bf16 kernel: keys from tile `late_tile` on score ~120 binades above the earlier ones for every query, |v| up to
    ~4.  bf16 P = exp2(120) is finite, so no infinity reaches the row sums - but 2^120 |v| 64 keys would overflow the fp32
    accumulators of O over a long sequence, and P so far above 1 loses nothing only if the reference moves: the waves vote on
    `row sum >= 2^64` and the replay takes the exact path."""
    from lowbit_quant_fa2_paddle_amd import core
    S = 1024
    q, k, v = oracle.make_inputs(1, 2, S, D, seed=51, dtype="bf16")
    # scores in base 2: q0 k0 sm_scale log2(e); channel 0 carries a step of 2 * b * b * sm_scale * log2(e) = 120
    b = (60.0 * D ** 0.5 / 1.44269504) ** 0.5
    q[..., 0] = b
    k[:, :, :64 * late_tile, 0] = -b
    k[:, :, 64 * late_tile:, 0] = b
    q, k = oracle.to_storage(q, "bf16"), oracle.to_storage(k, "bf16")
    tq, tk, tv = (_t(x, "bf16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: core.flash_attn_fp16(tq, tk, tv, return_lse=True))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    ref, rlse = oracle.sdpa_naive(*(x.astype(np.float64) for x in (q, k, v)), sm_scale=D ** -0.5, return_lse=True)
    _o_close(_np(o), ref, atol=4e-3, rtol=2e-3 + 2.0 ** -7)
    assert np.abs(_np(lse) - rlse).max() <= 2.5e-3 + 2.0 ** -20 * np.abs(rlse).max()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("layout", ["HND", "NHD"])
def test_router_statistic_runs_in_the_library(oracle, dev, dt, layout):
    """`select_quantization` (src/core.py:1051-1063): the three max|x| reductions are `lbfa_absmax` launches - bit-equal to the
    framework's reduction on contiguous, strided (packed-qkv view) and odd-sized tensors - and the thresholds pick the same branch
    as the reference's arithmetic on 0-d tensors of the storage dtype."""
    from lowbit_quant_fa2_paddle_amd import core
    from test_gpu_round3 import TDT
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    qkv = torch.randn((2, 3, 3, 333, 72), generator=g, device=dev).to(TDT[dt])
    if layout == "NHD":
        qkv = qkv.permute(0, 1, 3, 2, 4).contiguous()
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]  # strided views: batch stride 3x
    got = core._absmax([q, k, v])
    want = [float(t.float().abs().max()) for t in (q, k, v)]
    assert got == want
    for scale, kind in ((0.5, "INT4"), (3.0, "INT8"), (40.0, "FP16")):
        ts = [(t.float() * scale / t.float().abs().max() * 4.2).to(TDT[dt]) for t in (q, k, v)]
        ref_avg = sum((t.abs().max() / 127 for t in ts[1:]), ts[0].abs().max() / 127) / 3.0   # 0-d tensors of the storage dtype
        ref_kind = "FP16" if float(ref_avg) > 0.2 else ("INT8" if float(ref_avg) > 0.05 else "INT4")
        assert core.select_quantization(*ts) == ref_kind == kind
    assert core.compute_scale(q) == float(q.abs().max() / 127)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_reference_leaves_the_grid_inside_a_replay(oracle, dev, D, causal):
    """Two steps in channel 0: keys of tiles 1..4 score ~23 binades above tile 0 (fp16-P overflow at the first vote -> replay, with
    references of ~±30 binades: still on the rounded-scale grid), keys from tile 5 on ~300 binades above that: the replaying waves'
    references jump past 2^7 in tile 5 and they switch to the un-rounded scale in that tile (attn_fwd16.hip, compute_tile, REPLAY).
    Key blocks of different magnitude give every tile its own k_scale, so a rounded scale would shift ties between tiles."""
    import lowbit_quant_fa2_paddle_amd as lb
    S = 768
    q, k, v = oracle.make_inputs(1, 2, S, D, seed=61)
    a = 8.0 * (D / 64.0) ** 0.5
    q[..., 0] += a
    k[:, :, :64, 0] -= a
    k[:, :, 64:320, 0] += a
    k[:, :, 320:, 0] += 300.0 * D ** 0.5 / (1.44269504 * a)   # q0 k0 sm_scale log2(e) ~ +300
    rng = np.random.default_rng(3)
    k[:, :, 320:, 1:] *= np.repeat(rng.uniform(0.5, 2.0, (S - 320) // 64), 64).astype(np.float32)[None, None, :, None]
    q, k = oracle.to_storage(q, "fp16"), oracle.to_storage(k, "fp16")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, is_causal=causal, return_lse=True, smooth_k=False))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, smooth_k=False, amax_floor=1e-7, tail="neg_inf")
    assert np.abs(lse_ref).max() * 1.44269504 > 200.0
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_one_wave_off_the_grid_the_others_on_it(oracle, dev, D, causal):
    """Only the rows of ONE wave of every Q block (rows 32..63) carry the ±290-binade common mode: that wave votes for the replay and
    replays un-rounded, the three others keep their accumulators and their rounded-scale arithmetic through the partial replay
    (per-wave `wide`, attn_fwd16.hip)."""
    import lowbit_quant_fa2_paddle_amd as lb
    S = 768
    q, k, v = oracle.make_inputs(1, 2, S, D, seed=71)
    rng = np.random.default_rng(13)
    u = rng.standard_normal(D).astype(np.float32)
    u /= np.linalg.norm(u)
    a = 40.0 * (D / 64.0) ** 0.25
    r = np.arange(S) % 128
    sel = (r >= 32) & (r < 64)
    q[:, :, sel] += a * u
    k = k * np.repeat(rng.uniform(0.5, 2.0, S // 64), 64).astype(np.float32)[None, None, :, None] + a * u
    q, k = oracle.to_storage(q, "fp16"), oracle.to_storage(k, "fp16")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, is_causal=causal, return_lse=True, smooth_k=False))
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, smooth_k=False, amax_floor=1e-7, tail="neg_inf")
    big = np.abs(lse_ref[0, :, sel]).min() * 1.44269504
    small = np.abs(lse_ref[0, :, ~sel]).max() * 1.44269504
    assert big > 150.0 and small < 100.0, (big, small)
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("S", [1, 40, 64, 100, 128, 192])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_randint_on_one_to_three_tiles(oracle, dev, S, D, causal):
    """The reference's bench distribution on sequences of one to three key tiles (full, ragged, a single key): no vote inside the
    loop ever fires there - the off-grid references (thousands of binades) are caught by the vote behind the last tile, and the
    replay recomputes everything un-rounded."""
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = oracle.make_inputs(1, 2, S, D, seed=81 + S, dist="randint")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, is_causal=causal, return_lse=True))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, amax_floor=1e-7, tail="neg_inf")
    _o_close(_np(o), o_ref)
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -10 * np.abs(lse_ref).max()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_fp8_pv_on_the_bench_distribution(oracle, dev, D, causal):
    """qk_int8_pv_fp8 on q, k = randint(-100, 100): before round 4 the fp8 kernel kept these scores on its rounded-scale grid -
    tiles drifted against each other by a fraction of a binade, 30 % of the rows missed the per-element bound by 3..4 % (a
    common factor per row: e4m3(P) / P of the dominant key) - it now dequantises them un-rounded (attn_fwd.hip, `wide`).
    fp8-PV parity itself stays unpinned: this is the HIP path against the oracle's restatement."""
    import lowbit_quant_fa2_paddle_amd as lb
    from test_gpu_parity import _fp8_close, _fp8_flip_close
    q, k, v = oracle.make_inputs(1, 2, 512, D, seed=5, dist="randint")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp8_cuda(tq, tk, tv, is_causal=causal, return_lse=True))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_ref, slack, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, pv="fp8", amax_floor=1e-7,
                                                     return_slack=True)
    _fp8_close(_np(o), o_ref)
    _fp8_flip_close(_np(o), o_ref, slack, "fp16")
    assert np.abs(_np(lse) - lse_ref).max() <= 2e-3 + 2.0 ** -10 * np.abs(lse_ref).max()


def test_fp8_pv_largest_p_never_leaves_the_e4m3_range(oracle, dev):
    """B1 H8 S2048 D128 randint (the configuration in which tools/soak.py found it): at D = 128 the bias constant of the one-fma
    form is ~1e6, its fp32 ulp 2^-4 binades, and two roundings of it could lift a row's largest P from 448 past 464 - the last
    value that still rounds to 448; v_cvt_pk_fp8_f32 returns the NaN code beyond it, and the query's whole output row was NaN.
    Every output finite, and the head that failed against the oracle."""
    import lowbit_quant_fa2_paddle_amd as lb
    from test_gpu_parity import _fp8_close, _fp8_flip_close
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B, H, S, D = 1, 8, 2048, 128
    q = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).half()
    k = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).half()
    v = torch.randn((B, H, S, D), generator=g, device=dev).half()
    o, lse = lb.lowbit_fa_qk_int8_pv_fp8_cuda(q, k, v, return_lse=True)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    h = 7
    qn, kn, vn = (x[:, h:h + 1].float().cpu().numpy() for x in (q, k, v))
    o_ref, slack = oracle.lowbit_fa_forward(qn, kn, vn, pv="fp8", amax_floor=1e-7, return_slack=True)
    _fp8_close(_np(o[:, h:h + 1]), o_ref)
    _fp8_flip_close(_np(o[:, h:h + 1]), o_ref, slack, "fp16")


@pytest.mark.parametrize("op", ["int8", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_lse_overflows_exactly_where_the_reference_overflows(oracle, dev, op, D):
    """q, k ~ 1000 N(0,1) in fp16: the reference rounds `lse_correction = q . km` to the storage dtype (src/core.py:294-304), which
    overflows fp16 for most rows - its LSE is inf there and so must this one be, row for row (the fp8 kernel runs its tile loop with the
    mode bit that clamps fp16 overflows set; prologue and epilogue must not); O stays finite and, on these one-hot rows, equal to
    the oracle's for the fp16-P operator."""
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(D)
    q, k, v = (rng.standard_normal((1, 2, 640, D)).astype(np.float32) for _ in range(3))
    q, k, v = oracle.to_storage(q * 1000.0, "fp16"), oracle.to_storage(k * 1000.0, "fp16"), oracle.to_storage(v, "fp16")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    fn = lb.lowbit_fa_qk_int8_pv_fp16_triton if op == "int8" else lb.lowbit_fa_qk_int8_pv_fp8_cuda
    o, lse = fn(tq, tk, tv, return_lse=True)
    with np.errstate(all="ignore"):
        res = oracle.lowbit_fa_forward(q, k, v, return_lse=True, amax_floor=1e-7,
                                       **({"pv": "fp8", "return_slack": True} if op == "fp8" else {"tail": "neg_inf"}))
        o_ref, lse_ref = res[0], res[-1]
    assert torch.isfinite(o).all() and np.isfinite(o_ref).all()
    bad, bad_ref = ~np.isfinite(_np(lse)), ~np.isfinite(lse_ref)
    assert bad_ref.sum() > 100 and np.array_equal(bad, bad_ref)
    assert np.array_equal(np.sign(_np(lse)[bad]), np.sign(lse_ref[bad]))
    if op == "int8":
        _o_close(_np(o), o_ref)
    else:  # (before the fp8 kernel re-referenced such scores - next test - 73 % of these rows missed the bound, by up to 11 x)
        from test_gpu_parity import _fp8_close, _fp8_flip_close
        _fp8_close(_np(o), o_ref)
        _fp8_flip_close(_np(o), o_ref, res[1], "fp16")


@pytest.mark.parametrize("dt,mul", [("fp16", 300.0), ("fp16", 1000.0), ("fp16", 1e4), ("bf16", 1e5), ("bf16", 1e7)])
@pytest.mark.parametrize("D,causal", [(64, False), (128, True)])
def test_fp8_pv_on_scores_millions_of_binades_wide(oracle, dev, dt, mul, D, causal):
    """q, k = mul x N(0,1): softmax references of 1e5 .. 1e15 binades.  One fma `s sc - m` against the reference ROUNDED to fp32 leaves
    the largest P of a row at 448 x 2^(that rounding) - percents of P from |m| ~ 2^19 on, whole binades beyond 2^24 - which the e4m3
    conversion saturates away while the fp32 row sum keeps it: rows came out scaled down by up to 1/3 (x1000), LSE non-finite at
    x1e5.  The fp8 kernel now keeps the reference as an exact product (m_run + m_lo) and takes the scores relative to it
    (attn_fwd.hip, `huge`): these rows are one-hot or nearly so and must match the oracle's restatement element for element."""
    import lowbit_quant_fa2_paddle_amd as lb
    from test_gpu_parity import _fp8_close, _fp8_flip_close
    rng = np.random.default_rng(int(mul) % 1000 + D)
    q, k, v = (rng.standard_normal((1, 2, 640, D)).astype(np.float32) for _ in range(3))
    q, k, v = oracle.to_storage(q * mul, dt), oracle.to_storage(k * mul, dt), oracle.to_storage(v, dt)
    tq, tk, tv = (_t(x, dt, dev) for x in (q, k, v))
    o, lse = _run_twice(lambda: lb.lowbit_fa_qk_int8_pv_fp8_cuda(tq, tk, tv, is_causal=causal, return_lse=True, smooth_k=False))
    with np.errstate(all="ignore"):
        o_ref, slack, lse_ref = oracle.lowbit_fa_forward(q, k, v, dtype=dt, is_causal=causal, return_lse=True, smooth_k=False, pv="fp8",
                                                         amax_floor=1e-7, return_slack=True)
    assert np.isfinite(o_ref).all() and np.isfinite(lse_ref).all()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    _fp8_close(_np(o), o_ref)
    _fp8_flip_close(_np(o), o_ref, slack, dt)
    assert np.abs(_np(lse) - lse_ref).max() <= 2.0 ** -20 * np.abs(lse_ref).max()


@pytest.mark.parametrize("D,Hq,Hkv", [(64, 2, 2), (128, 4, 2)])
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_on_the_bench_distribution(oracle, dev, D, Hq, Hkv, causal):
    """Packed variable-length batches of q, k = randint(-100, 100): sequences of 1 key tile up to 9, ragged tails, a one-token
    sequence - every one of them leaves the scale grid (the packed path shares the tile loop, its votes and its replay)."""
    import lowbit_quant_fa2_paddle_amd as lb
    lens = [300, 1, 64, 577, 130]
    rng = np.random.default_rng(91)
    tot = sum(lens)
    q = oracle.to_storage(rng.integers(-100, 100, (tot, Hq, D)).astype(np.float32), "fp16")
    k = oracle.to_storage(rng.integers(-100, 100, (tot, Hkv, D)).astype(np.float32), "fp16")
    v = oracle.to_storage(rng.standard_normal((tot, Hkv, D)).astype(np.float32), "fp16")
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    tcu = torch.from_numpy(cu).to(dev)
    o = lb.lowbit_fa_varlen(tq, tk, tv, tcu, tcu, max(lens), max(lens), is_causal=causal)
    o2 = lb.lowbit_fa_varlen(tq, tk, tv, tcu, tcu, max(lens), max(lens), is_causal=causal)
    assert torch.isfinite(o).all() and torch.equal(o, o2)
    o_ref = oracle.lowbit_fa_varlen(q, k, v, cu, cu, is_causal=causal, amax_floor=1e-7, tail="neg_inf")
    _o_close(_np(o), o_ref)


@pytest.mark.parametrize("op", ["int8", "int4", "fp8", "sdpa16"])
@pytest.mark.parametrize("D", [64, 96, 128])
def test_strided_operands_give_the_bits_of_contiguous_ones(dev, op, D):
    """q, k, v as views with a batch, head or token stride of their own (a slice of a fused projection output, every second token
    of a cache, every second head): operands go to the C ABI as strides (attn_qk_int8_per_block.py:183-196), no copy is made, and
    O and LSE are bit for bit those of the contiguous call."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import core
    g = torch.Generator(device=dev)
    g.manual_seed(D)
    B, H, S = 2, 4, 333
    fn = {"int8": lambda q, k, v: lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, is_causal=True, return_lse=True),
          "int4": lambda q, k, v: lb.lowbit_fa_qk_int4_pv_fp16_triton(q, k, v, return_lse=True),
          "fp8": lambda q, k, v: lb.lowbit_fa_qk_int8_pv_fp8_cuda(q, k, v, return_lse=True),
          "sdpa16": lambda q, k, v: core.flash_attn_fp16(q, k, v, is_causal=True, return_lse=True)}[op]
    q, k, v = (torch.randn((B, H, S, D), generator=g, device=dev).half() for _ in range(3))

    def batch_strided(x):
        buf = torch.zeros((B, 3, H, S, D), device=dev, dtype=x.dtype)
        buf[:, 1] = x
        return buf[:, 1]

    def token_strided(x):
        buf = torch.zeros((B, H, 2 * S, D), device=dev, dtype=x.dtype)
        buf[:, :, 1::2] = x
        return buf[:, :, 1::2]

    def head_strided(x):
        buf = torch.zeros((B, 2 * H, S, D), device=dev, dtype=x.dtype)
        buf[:, ::2] = x
        return buf[:, ::2]

    o0, lse0 = fn(q, k, v)
    assert torch.isfinite(o0).all()
    for views in ((batch_strided(q), token_strided(k), head_strided(v)), (token_strided(q), head_strided(k), batch_strided(v)),
                  (head_strided(q), batch_strided(k), token_strided(v))):
        assert not any(t.is_contiguous() for t in views)
        o, lse = fn(*views)
        assert torch.equal(o, o0) and torch.equal(lse, lse0)
