"""GPU tests (run with `-m gpu`): the configurations of tools/soak.py as single launches checked against the oracle, one long
randint sequence through the fp8-PV operator, and the stated range of the fp16-P operators (include/lowbit_fa.h, `range`).

tools/soak.py launches each configuration many times and compares the launches with each other; here every configuration runs
ONCE, all of O and LSE must be finite (the check that caught the NaN rows of round 4) and one sampled (batch, head) is compared
with the oracle - one head keeps its quantisation blocks, km and V scales, as test_int8_fp8_c5_shard does."""
import numpy as np
import pytest

from test_gpu_parity import _fp8_flip_close, _np, _o_close, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SOAK_KINDS = ["normal", "randint", "exact", "peaky", "late"]
SOAK_ROWS = [  # B, H, S, D, causal, operator, dtype  (tools/soak.py)
    (2, 16, 4096, 64, False, "int8", "fp16"),
    (2, 16, 2048, 128, True, "int8", "fp16"),
    (2, 8, 1000, 64, True, "int4", "bf16"),
    (1, 8, 2048, 128, False, "fp8", "fp16"),
]


def _soak_inputs(kind, B, H, S, D, dtype, dev):
    """tools/soak.py `inputs`, on the device generator with the same seed."""
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    if kind == "randint":
        q = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).to(dtype)
        k = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).to(dtype)
    else:
        q = torch.randn((B, H, S, D), generator=g, device=dev)
        k = torch.randn((B, H, S, D), generator=g, device=dev)
        if kind == "exact":      # first key tile far below the rest: every Q block replays on the grid
            a = 8.0 * (D / 64.0) ** 0.5
            q[..., 0] += a
            k[:, :, :64, 0] -= a
            k[:, :, 64:, 0] += a
        elif kind == "peaky":    # some rows overflow at some vote, others never
            q *= 6.0
        elif kind == "late":     # a 300-binade step in the middle of the sequence
            a = 8.0 * (D / 64.0) ** 0.5
            q[..., 0] += a
            k[:, :, :64, 0] -= a
            k[:, :, 64:S // 2, 0] += a
            k[:, :, S // 2:, 0] += 300.0 * D ** 0.5 / (1.44269504 * a)
        q, k = q.to(dtype), k.to(dtype)
    v = torch.randn((B, H, S, D), generator=g, device=dev).to(dtype)
    return q, k, v


@pytest.mark.parametrize("row", SOAK_ROWS, ids=lambda r: f"{r[5]}-S{r[2]}-D{r[3]}-c{int(r[4])}")
@pytest.mark.parametrize("kind", SOAK_KINDS)
def test_soak_configuration_once(oracle, dev, kind, row):
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, S, D, causal, op, dt = row
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    q, k, v = _soak_inputs(kind, B, H, S, D, tdt, dev)
    fn = {"int8": lb.lowbit_fa_qk_int8_pv_fp16_triton, "int4": lb.lowbit_fa_qk_int4_pv_fp16_triton,
          "fp8": lb.lowbit_fa_qk_int8_pv_fp8_cuda}[op]
    o, lse = fn(q, k, v, is_causal=causal, return_lse=True)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    rng = np.random.default_rng(10 * SOAK_KINDS.index(kind) + SOAK_ROWS.index(row))
    b, h = int(rng.integers(0, B)), int(rng.integers(0, H))
    rows = S if causal else min(S, 1024)  # non-causal: whole 128-row Q blocks against all keys
    qn = q[b:b + 1, h:h + 1, :rows].float().cpu().numpy()
    kn, vn = (x[b:b + 1, h:h + 1].float().cpu().numpy() for x in (k, v))
    got = _np(o[b:b + 1, h:h + 1, :rows])
    if op == "fp8":
        ref, slack = oracle.lowbit_fa_forward(qn, kn, vn, dtype=dt, is_causal=causal, pv="fp8", amax_floor=1e-7, return_slack=True)
        _fp8_flip_close(got, ref, slack, dt)
    else:
        ref = oracle.lowbit_fa_forward(qn, kn, vn, dtype=dt, is_causal=causal, amax_floor=1e-7, tail="neg_inf", causal_mask="neg_inf",
                                       q_qmax=7 if op == "int4" else 127, k_qmax=7 if op == "int4" else 127)
        _o_close(got, ref, dt)


def test_fp8_pv_long_randint_sequence(oracle, dev):
    """B1 H4 S32768 D128 on the reference's bench distribution q, k = randint(-100, 100), v ~ N(0,1) (test_int8_fp8_c5_shard does
    this for N(0,1) only): all outputs finite, and the first 1024 rows of one head against the oracle over all 32768 keys."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, S, D = 1, 4, 32768, 128
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    q = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).half()
    k = torch.randint(-100, 100, (B, H, S, D), generator=g, device=dev).half()
    v = torch.randn((B, H, S, D), generator=g, device=dev).half()
    o, lse = lb.lowbit_fa_qk_int8_pv_fp8_cuda(q, k, v, return_lse=True)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    h, rows = 2, 1024
    qn = q[:, h:h + 1, :rows].float().cpu().numpy()
    kn, vn = (x[:, h:h + 1].float().cpu().numpy() for x in (k, v))
    ref, slack, lse_ref = oracle.lowbit_fa_forward(qn, kn, vn, pv="fp8", amax_floor=1e-7, return_lse=True, return_slack=True)
    _fp8_flip_close(_np(o[:, h:h + 1, :rows]), ref, slack, "fp16")
    assert np.abs(_np(lse[:, h:h + 1, :rows]) - lse_ref).max() <= 2e-3 + 2.0 ** -9 * np.abs(lse_ref).max()


@pytest.mark.parametrize("mul", [1000.0, 2500.0])
@pytest.mark.parametrize("op", ["int8", "int4"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_fp16_p_operators_at_the_stated_range(oracle, dev, mul, op, D, causal):
    """include/lowbit_fa.h promises finite, correct fp16-P output for |s| < 2^27, "q, k of a few thousand times N(0,1)": pinned at
    1000 and 2500 N(0,1), smooth_k off so that the LSE is finite.  The oracle masks the causal diagonal with -inf as the kernels do
    (the reference's additive -1e6 no longer masks at these scores)."""
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(int(mul) + D + 2 * causal)
    q, k, v = (rng.standard_normal((1, 2, 384, D)).astype(np.float32) for _ in range(3))
    q, k, v = oracle.to_storage(q * np.float32(mul), "fp16"), oracle.to_storage(k * np.float32(mul), "fp16"), oracle.to_storage(v, "fp16")
    tq, tk, tv = (_t(x, "fp16", dev) for x in (q, k, v))
    fn = lb.lowbit_fa_qk_int8_pv_fp16_triton if op == "int8" else lb.lowbit_fa_qk_int4_pv_fp16_triton
    o, lse = fn(tq, tk, tv, is_causal=causal, return_lse=True, smooth_k=False)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    qm = 7 if op == "int4" else 127
    o_ref, lse_ref = oracle.lowbit_fa_forward(q, k, v, is_causal=causal, return_lse=True, smooth_k=False, amax_floor=1e-7,
                                              tail="neg_inf", causal_mask="neg_inf", q_qmax=qm, k_qmax=qm)
    _o_close(_np(o), o_ref, "fp16")
    assert np.abs(_np(lse) - lse_ref).max() <= 1e-3 + 2.0 ** -20 * np.abs(lse_ref).max()
