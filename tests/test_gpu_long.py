"""GPU tests past 64K keys and at the 2 GiB operand window (run with `-m gpu` on an MI355X).

  * the smooth-K mean beyond 64 partial sums: `lbfa_forward` adds the fp64 partials inside the K quantiser only while there are at
    most 64 of them (Sk <= 65536); longer key sequences take a separate finalize launch.  The one-call operator must give the bits
    of the modular composition on both sides of that switch, and km the bits of the oracle's float64 mean;
  * long sequences against the oracle on sampled 128-row Q blocks (`q_blocks`): block 0, the block of row 65536, one block of an
    even and one of an odd round of Q blocks (the non-causal kernels walk the key tiles backwards in odd rounds, `kRound` in
    attn_fwd16.hip / attn_fwd.hip), the last block - ragged at 65537;
  * the 2 GiB operand windows of the C ABI: for every entry the largest length its own check accepts runs and is checked at the far
    end of its window (last rows of the last head), one row more is refused before anything is launched; and one tensor with more
    than 2^31 elements (64-bit base offsets).

Bounds are those of the short-sequence tests (test_gpu_parity.py, test_gpu_fp16.py).  The worst ratio error / bound of every check
is printed as `LONGBOUND <test> <check> worst=<ratio>`.
"""
import os

import numpy as np
import pytest

from test_gpu_parity import TDT, _canon, _fp8_flip_close, _np, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LIM = 0x7FFFFFFF            # largest per-(batch, head) operand window the C ABI accepts, in bytes
BLKQ, BLKK = 128, 64        # LBFA_BLKQ / LBFA_BLKK
KROUND16 = {64: 96, 128: 64}  # attn_fwd16.hip: Q blocks per round of the fp16-P kernels (int8 / int4 with fp16 P, and the fp16 kernel)
KROUND8 = 64                  # attn_fwd.hip: the fp8-PV kernel


def _report(check, worst):
    if os.environ.get("PYTEST_CURRENT_TEST"):
        print(f"LONGBOUND {os.environ['PYTEST_CURRENT_TEST'].split(' ')[0]} {check} worst={worst:.3f}")


def _close(o, ref, atol, rtol, check):
    """|o - ref| <= atol + rtol |ref| on every element (the `_o_close` bound), everything finite."""
    assert np.isfinite(o).all(), f"{check}: non-finite output"
    ratio = np.abs(o - ref) / (atol + rtol * np.abs(ref))
    _report(check, float(ratio.max()))
    assert (ratio <= 1).all(), f"{check}: {(ratio > 1).sum()} elements beyond the bound, worst ratio {ratio.max():.2f}"


def _o_bound(o, ref, dtype, atol=2e-3, rtol=2e-3, check="o"):
    _close(o, ref, atol, rtol + (2.0 ** -7 if dtype == "bf16" else 0.0), check)


def _lse_bound(lse, ref, bound, check="lse"):
    assert np.isfinite(lse).all(), f"{check}: non-finite LSE"
    err = float(np.abs(lse - ref).max())
    _report(check, err / bound)
    assert err <= bound, f"{check}: max |dLSE| {err:.3e} > {bound:.3e}"


def _lse_bound_int8(ref, dtype):  # test_operator_int8_fp16_vs_oracle: 1e-3 + one ulp of the rounded lse correction
    return 1e-3 + (2.0 ** -10 if dtype == "fp16" else 2.0 ** -7) * float(np.abs(ref).max())


def _lse_bound_fp8(ref):          # test_operator_int8_fp8_vs_oracle
    return 2e-3 + 2.0 ** -9 * float(np.abs(ref).max())


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _rows_of(x, rows, layout):
    return x[:, rows] if layout == "NHD" else x[:, :, rows]


def _sample_blocks(S, kround):
    """Block 0, the block of row 65536, one block of round 1 (odd: keys walked backwards) and one of round 2 (even), the last."""
    nq = (S + BLKQ - 1) // BLKQ
    return sorted({b for b in (0, 65536 // BLKQ, kround + 5, 2 * kround + 7, nq - 1) if b < nq})


def _reversed(blocks, S, causal):
    """attn_fwd.hip: a Q block walks the key tiles backwards when (qt / kRound) is odd, for non-causal calls with Sk % 64 == 0."""
    return [(not causal) and S % BLKK == 0 and (b // KROUND8) % 2 == 1 for b in blocks]


# ------------------------------------------------------------------------------------------------------
# a. the unfused smooth-K mean, exactly
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk", [65536, 65537, 131072])   # 64 partial sums (fused) / 65 / 128 (separate finalize launch)
@pytest.mark.parametrize("dtype,layout,pv", [("fp16", "HND", "fp16"), ("bf16", "NHD", "fp8"), ("fp16", "NHD", "fp8"),
                                             ("bf16", "HND", "fp16")])
def test_smooth_k_mean_past_64_partials_is_exact(oracle, dev, Sk, dtype, layout, pv):
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib, attn_qk_int8_per_block as attn, quant, quant_per_block as qpb
    B, H, Hkv, Sq, D = 1, 4, 2, 256, 128
    q, k, v = oracle.make_inputs(B, H, Sq, D, seed=Sk + 7 * len(dtype + layout + pv), layout=layout, dtype=dtype, Hkv=Hkv,
                                 Sk=Sk, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    # leave NaN in the allocator's free block of the workspace's size: a km the operator reads before it was written shows
    ws_bytes = _lib.load().lbfa_forward_workspace_bytes_dt(B, H, Hkv, Sq, Sk, D, _lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16,
                                                           1 if pv == "fp8" else 0, 1, 1)
    poison = torch.full((ws_bytes // 2 + 1,), float("nan"), dtype=torch.float16, device=dev)
    del poison
    fn = lb.lowbit_fa_qk_int8_pv_fp16_triton if pv == "fp16" else lb.lowbit_fa_qk_int8_pv_fp8_cuda
    o, lse = fn(tq, tk, tv, tensor_layout=layout, return_lse=True)
    sm_scale = D ** -0.5
    km = qpb.mean_seq(tk, layout)
    km_ref = oracle.mean_seq(_canon(k, layout), dtype)
    assert np.array_equal(_np(km).reshape(km_ref.shape), km_ref), "km differs from the float64 mean"
    q8, qs, corr = qpb.quantize(tq, sm_scale=sm_scale * 1.44269504, qmax=127, blk=128, tensor_layout=layout, rowdot_vec=km)
    k8, ks = qpb.quantize(tk, sm_scale=1.0, qmax=127, blk=64, tensor_layout=layout, mean=km)
    if pv == "fp8":
        vin, vs, _ = quant.per_channel_fp8(tv, tensor_layout=layout)
    else:
        vin, vs = tv, None
    o2, lse2 = attn.forward(q8, k8, vin, qs, ks, tensor_layout=layout, output_dtype=TDT[dtype], return_lse=True, v_scale=vs)
    assert torch.equal(o, o2), "one-call operator and modular composition differ"
    # the fused epilogue forms q . km in another fp32 order than the quantiser's row dot: the two may round it to neighbouring
    # values of the storage dtype (one ulp of |corr|, scaled by sm_scale)
    ulp = 2.0 ** -10 if dtype == "fp16" else 2.0 ** -7
    assert bool(((lse - (lse2 / 1.44269504 + corr * sm_scale)).abs() <= 1e-5 + ulp * sm_scale * corr.abs()).all())
    ro, rlse = oracle.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, return_lse=True, pv=pv, tail="neg_inf",
                                        amax_floor=1e-7)
    _lse_bound(_np(lse), rlse, _lse_bound_int8(rlse, dtype) if pv == "fp16" else _lse_bound_fp8(rlse))
    if pv == "fp16":
        _o_bound(_np(o), ro, dtype)
    del tq, tk, tv, o, o2, lse, lse2, q8, k8, vin, km
    _free()


# ------------------------------------------------------------------------------------------------------
# b. long sequences against the oracle on sampled Q blocks
# ------------------------------------------------------------------------------------------------------
LONG = [
    # op, S, D, H, Hkv, layout, causal, dtype
    ("int8", 131072, 64, 2, 2, "HND", False, "fp16"),
    ("int8", 65537, 128, 4, 2, "NHD", True, "bf16"),
    ("int8", 131072, 128, 1, 1, "HND", True, "fp16"),
    ("int4", 65537, 64, 1, 1, "HND", False, "fp16"),
    ("int4", 131072, 128, 2, 1, "NHD", False, "bf16"),
    ("fp8", 131072, 64, 1, 1, "HND", False, "fp16"),
    ("fp8", 65537, 128, 1, 1, "NHD", True, "bf16"),
    ("fp8", 131072, 128, 1, 1, "HND", False, "bf16"),
    ("fp16", 131072, 64, 2, 2, "HND", False, "fp16"),
    ("fp16", 65537, 128, 4, 2, "NHD", True, "bf16"),
    ("fp16", 131072, 128, 2, 1, "NHD", False, "fp16"),
]


@pytest.mark.parametrize("op,S,D,H,Hkv,layout,causal,dtype", LONG)
def test_long_sequence_vs_oracle_on_sampled_blocks(oracle, dev, op, S, D, H, Hkv, layout, causal, dtype):
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = oracle.make_inputs(1, H, S, D, seed=S % 1000 + D + H, layout=layout, dtype=dtype, Hkv=Hkv, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    blocks = _sample_blocks(S, KROUND8 if op == "fp8" else KROUND16[D])
    rows = oracle.block_rows(blocks, S)
    qr = _rows_of(q, rows, layout)
    if op == "fp16":
        o, lse = lb.core.flash_attn_fp16(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True)
        o, lse = _canon(_np(o), layout)[:, :, rows], _np(lse)[:, :, rows]
        del tq, tk, tv
        _free()
        kc, vc = (_canon(a, layout).astype(np.float64) for a in (k, v))
        qc = _canon(qr, layout).astype(np.float64)
        for i, b in enumerate(blocks):  # one block at a time: [H, 128, S] scores in float64
            sl = slice(i * BLKQ, min((i + 1) * BLKQ, len(rows)))
            ro, rlse = oracle.sdpa_naive(qc[:, :, sl], kc, vc, is_causal=causal, sm_scale=D ** -0.5, return_lse=True, q_blocks=[b])
            _o_bound(o[:, :, sl], ro, dtype, atol=2e-3 if dtype == "fp16" else 4e-3, check=f"o[block {b}]")
            _lse_bound(lse[:, :, sl], rlse, 1e-3 if dtype == "fp16" else 2.5e-3, check=f"lse[block {b}]")
        return
    kw = dict(dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True, tail="neg_inf", amax_floor=1e-7, q_blocks=blocks)
    if op == "fp8":
        o, lse = lb.lowbit_fa_qk_int8_pv_fp8_cuda(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True)
        ro, slack, rlse = oracle.lowbit_fa_forward(qr, k, v, pv="fp8", return_slack=True,
                                                   fp8_key_tiles_reversed=_reversed(blocks, S, causal), **kw)
    else:
        fn = lb.lowbit_fa_qk_int8_pv_fp16_triton if op == "int8" else lb.lowbit_fa_qk_int4_pv_fp16_triton
        o, lse = fn(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True)
        qmax = 127.0 if op == "int8" else 7.0
        ro, rlse = oracle.lowbit_fa_forward(qr, k, v, q_qmax=qmax, k_qmax=qmax, **kw)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o, lse = _rows_of(_np(o), rows, layout), _np(lse)[:, :, rows]
    del tq, tk, tv
    _free()
    if op == "fp8":
        worst, _ = _fp8_flip_close(o, ro, slack, dtype)
        _report("o", worst)
        _lse_bound(lse, rlse, _lse_bound_fp8(rlse))
    else:
        _o_bound(o, ro, dtype)
        _lse_bound(lse, rlse, _lse_bound_int8(rlse, dtype))


# ------------------------------------------------------------------------------------------------------
# c. the 2 GiB operand windows, both sides
# ------------------------------------------------------------------------------------------------------
# Head counts: with 46 heads (94 for the int8 Q of lbfa_attn_fwd) of 128 channels the largest accepted window ends 255 (127) bytes
# below 2^31 - 1, the closest any head count up to 128 gets - so a limit that moves by one channel stride (D elements) fails here.
def _largest(win, D=128):
    """Largest length n whose window win(n) (bytes, increasing in n) the C ABI accepts (win(n) <= LIM), within 2 D bytes of it."""
    lo, hi = 1, 1 << 40
    while win(hi) <= LIM:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if win(mid) <= LIM else (lo, mid)
    assert win(lo) <= LIM < win(lo + 1)
    assert LIM - win(lo) < 2 * D, f"window ends {LIM - win(lo)} bytes below the limit: choose another head count"
    return lo


def _randn(shape, dtype, seed, bias=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, generator=g, device="cuda", dtype=TDT[dtype])
    return x.add_(bias) if bias else x


def _refused(monkeypatch, call, what):
    """`call()` must raise ValueError naming the 2 GiB window before it launches anything: every buffer the operator allocates
    (its output among them) is pre-filled and must still hold that value afterwards."""
    from lowbit_quant_fa2_paddle_amd import _tensor
    made = []

    def empty(self, shape, dtype, like):
        t = torch.full(shape, 7, dtype=dtype, device=like.device)
        made.append(t)
        return t
    monkeypatch.setattr(_tensor.TorchOps, "empty", empty)
    with pytest.raises(ValueError, match=f"{what}: per-.* operand window exceeds 2 GiB"):
        call()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert made, "the operator allocated no output"
    for t in made:
        assert bool((t == 7).all()), f"a buffer of shape {tuple(t.shape)} was written by a call that was refused"
    del made[:]
    _free()


# fp8 on the K / V side is left out: there the int8 K codes in the workspace ([B, Hkv, Sk, D], stride D) bind, at 16M keys (D = 128),
# too many for the oracle to follow within the time of this file
@pytest.mark.parametrize("side,pv,dtype", [("q", "fp16", "fp16"), ("q", "fp8", "bf16"), ("kv", "fp16", "bf16")])
def test_forward_window_limit(oracle, dev, monkeypatch, side, pv, dtype):
    """lbfa_forward: Q window 2 ((Sq + 128) qs + D), K codes (Sk + 128) D + D, V 2 ((Sk + 128) vs + D) (fp8: (Sk + 128) D)."""
    import lowbit_quant_fa2_paddle_amd as lb
    H, D = 46, 128
    fn = lb.lowbit_fa_qk_int8_pv_fp16_triton if pv == "fp16" else lb.lowbit_fa_qk_int8_pv_fp8_cuda
    if side == "q":
        Hkv = 2
        n = _largest(lambda s: 2 * ((s + BLKQ) * H * D + D))
        Sq, Sk = n, 256
    else:
        Hkv = H
        n = _largest(lambda s: max(2 * ((s + 2 * BLKK) * Hkv * D + D), (s + 2 * BLKK) * D + D))
        Sq, Sk = 200, n
    big_q, big_k = (Sq + 1, Sk) if side == "q" else (Sq, Sk + 1)
    q = _randn((1, big_q, H, D), dtype, 1)
    k = _randn((1, big_k, Hkv, D), dtype, 2, bias=0.5)
    v = _randn((1, big_k, Hkv, D), dtype, 3)
    _refused(monkeypatch, lambda: fn(q, k, v, tensor_layout="NHD", return_lse=True), "lbfa_forward")
    q, k, v = q[:, :Sq], k[:, :Sk], v[:, :Sk]
    o, lse = fn(q, k, v, tensor_layout="NHD", return_lse=True)
    h, hk = H - 1, Hkv - 1
    nq = (Sq + BLKQ - 1) // BLKQ
    blocks = [nq - 1]
    rows = oracle.block_rows(blocks, Sq)
    qr = q[:, rows[0]:, h:h + 1].float().cpu().numpy()
    kh, vh = (t[:, :, hk:hk + 1].float().cpu().numpy() for t in (k, v))
    orow = o[:, rows[0]:, h:h + 1].float().cpu().numpy()
    lrow = lse[:, h:h + 1, rows[0]:].cpu().numpy()
    assert bool(torch.isfinite(o[:, -BLKQ:]).all())
    del q, k, v, o, lse
    _free()
    kw = dict(dtype=dtype, tensor_layout="NHD", return_lse=True, tail="neg_inf", amax_floor=1e-7, q_blocks=blocks)
    if pv == "fp8":
        ro, slack, rlse = oracle.lowbit_fa_forward(qr, kh, vh, pv="fp8", return_slack=True,
                                                   fp8_key_tiles_reversed=_reversed(blocks, Sk, False), **kw)
        _report("o", _fp8_flip_close(orow, ro, slack, dtype)[0])
        _lse_bound(lrow, rlse, _lse_bound_fp8(rlse))
    else:
        ro, rlse = oracle.lowbit_fa_forward(qr, kh, vh, **kw)
        _o_bound(orow, ro, dtype)
        _lse_bound(lrow, rlse, _lse_bound_int8(rlse, dtype))


@pytest.mark.parametrize("side", ["q", "kv"])
def test_sdpa_window_limit(oracle, dev, monkeypatch, side):
    """lbfa_sdpa_fwd: 2 ((Sq + 128) qs + D), 2 ((Sk + 128) ks + D), 2 ((Sk + 128) vs + D), D the caller's head dim."""
    from lowbit_quant_fa2_paddle_amd import core
    H, D, dtype = 46, 128, "fp16"
    if side == "q":
        Hkv = 2
        Sq, Sk = _largest(lambda s: 2 * ((s + BLKQ) * H * D + D)), 256
    else:
        Hkv = H
        Sq, Sk = 200, _largest(lambda s: 2 * ((s + 2 * BLKK) * Hkv * D + D))
    big_q, big_k = (Sq + 1, Sk) if side == "q" else (Sq, Sk + 1)
    q = _randn((1, big_q, H, D), dtype, 4)
    k = _randn((1, big_k, Hkv, D), dtype, 5, bias=0.5)
    v = _randn((1, big_k, Hkv, D), dtype, 6)
    _refused(monkeypatch, lambda: core.flash_attn_fp16(q, k, v, tensor_layout="NHD", return_lse=True), "lbfa_sdpa_fwd")
    q, k, v = q[:, :Sq], k[:, :Sk], v[:, :Sk]
    o, lse = core.flash_attn_fp16(q, k, v, tensor_layout="NHD", return_lse=True)
    h, hk = H - 1, Hkv - 1
    nq = (Sq + BLKQ - 1) // BLKQ
    r0 = (nq - 1) * BLKQ
    qr = q[:, r0:, h].double().cpu().numpy()[:, None]
    kh, vh = (t[:, :, hk].double().cpu().numpy()[:, None] for t in (k, v))
    orow, lrow = o[:, r0:, h].float().cpu().numpy()[:, None], lse[:, h, r0:].cpu().numpy()[:, None]
    del q, k, v, o, lse
    _free()
    ro, rlse = oracle.sdpa_naive(qr, kh, vh, sm_scale=D ** -0.5, return_lse=True, q_blocks=[nq - 1])
    _o_bound(orow, ro, dtype)
    _lse_bound(lrow, rlse, 1e-3)


@pytest.mark.parametrize("side", ["q", "kv"])
def test_attn_fwd_window_limit(oracle, dev, monkeypatch, side):
    """lbfa_attn_fwd (int8 codes): (Sq + 128) qs + D, (Sk + 128) ks + D, fp16 V 2 ((Sk + 128) vs + D)."""
    from lowbit_quant_fa2_paddle_amd import attn_qk_int8_per_block as attn
    D = 128
    if side == "q":
        H, Hkv = 94, 2
        Sq, Sk = _largest(lambda s: (s + BLKQ) * H * D + D), 256
    else:
        H = Hkv = 46
        Sq, Sk = 200, _largest(lambda s: max((s + 2 * BLKK) * Hkv * D + D, 2 * ((s + 2 * BLKK) * Hkv * D + D)))
    big_q, big_k = (Sq + 1, Sk) if side == "q" else (Sq, Sk + 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    q8 = torch.randint(-127, 128, (1, big_q, H, D), generator=g, device="cuda", dtype=torch.int8)
    k8 = torch.randint(-127, 128, (1, big_k, Hkv, D), generator=g, device="cuda", dtype=torch.int8)
    v = _randn((1, big_k, Hkv, D), "fp16", 8)
    # scales that put the scores at about one unit of log2: q_scale k_scale ~ 1 / (sqrt(D) 127^2 / 3)
    s0 = (3.0 / (127.0 ** 2 * D ** 0.5)) ** 0.5

    def scales(n, blk, seed):
        gs = torch.Generator(device="cuda").manual_seed(seed)
        return (torch.rand((1, n[0], (n[1] + blk - 1) // blk), generator=gs, device="cuda") * 0.4 + 0.8) * s0
    qs, ks = scales((H, big_q), BLKQ, 9), scales((Hkv, big_k), BLKK, 10)
    _refused(monkeypatch, lambda: attn.forward(q8, k8, v, qs, ks, tensor_layout="NHD", return_lse=True), "lbfa_attn_fwd")
    q8, k8, v = q8[:, :Sq], k8[:, :Sk], v[:, :Sk]
    qs, ks = qs[:, :, :(Sq + BLKQ - 1) // BLKQ].contiguous(), ks[:, :, :(Sk + BLKK - 1) // BLKK].contiguous()
    o, lse = attn.forward(q8, k8, v, qs, ks, tensor_layout="NHD", return_lse=True)
    h, hk = H - 1, Hkv - 1
    nq = (Sq + BLKQ - 1) // BLKQ
    r0 = (nq - 1) * BLKQ
    qr = q8[:, r0:, h].cpu().numpy()[:, None]
    kh = k8[:, :, hk].cpu().numpy()[:, None]
    vh = v[:, :, hk].float().cpu().numpy()[:, None]
    qsr, ksr = qs[:, h:h + 1, nq - 1:].cpu().numpy(), ks[:, hk:hk + 1].cpu().numpy()
    orow, lrow = o[:, r0:, h].float().cpu().numpy()[:, None], lse[:, h, r0:].cpu().numpy()[:, None]
    del q8, k8, v, qs, ks, o, lse
    _free()
    ro, rlse = oracle.attn_fwd_int8_fp16(qr, kh, vh, qsr, ksr, causal=False, return_lse=True, tail="neg_inf", q_blocks=[nq - 1])
    _o_bound(orow, ro, "fp16")
    _lse_bound(lrow, rlse, 1e-3 + 2.0 ** -21 * float(np.abs(rlse).max()))  # base-2 LSE of lbfa_attn_fwd (test_gpu_parity golden bound)


@pytest.mark.parametrize("side", ["q", "kv"])
def test_varlen_window_limit(oracle, dev, monkeypatch, side):
    """lbfa_forward_varlen, per sequence from max_seqlen: 2 ((max_q + 128) sq + D), (max_k + 128) Hkv D + D, 2 ((max_k + 128) sv + D)."""
    import lowbit_quant_fa2_paddle_amd as lb
    H, D, dtype = 46, 128, "fp16"
    if side == "q":
        Hkv = 2
        n = _largest(lambda s: 2 * ((s + BLKQ) * H * D + D))
        lq, lk = [n, 77], [256, 77]
    else:
        Hkv = H
        n = _largest(lambda s: max((s + 2 * BLKK) * Hkv * D + D, 2 * ((s + 2 * BLKK) * Hkv * D + D)))
        lq, lk = [200, 77], [n, 77]
    # the long sequence first, one token more than accepted: the refused call states that length, the accepted one a prefix of it
    big_q = [lq[0] + (side == "q"), lq[1]]
    big_k = [lk[0] + (side == "kv"), lk[1]]
    q = _randn((sum(big_q), H, D), dtype, 11)
    k = _randn((sum(big_k), Hkv, D), dtype, 12, bias=0.5)
    v = _randn((sum(big_k), Hkv, D), dtype, 13)
    cu = lambda lens: torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    _refused(monkeypatch, lambda: lb.lowbit_fa_varlen(q, k, v, cu(big_q), cu(big_k), max(big_q), max(big_k)), "lbfa_forward_varlen")
    # accepted: the long sequence one token shorter
    q2 = torch.cat([q[:lq[0]], q[big_q[0]:]]) if side == "q" else q
    k2 = torch.cat([k[:lk[0]], k[big_k[0]:]]) if side == "kv" else k
    v2 = torch.cat([v[:lk[0]], v[big_k[0]:]]) if side == "kv" else v
    del q, k, v
    _free()
    o = lb.lowbit_fa_varlen(q2, k2, v2, cu(lq), cu(lk), max(lq), max(lk))
    h, hk = H - 1, Hkv - 1
    nq = (lq[0] + BLKQ - 1) // BLKQ
    r0 = (nq - 1) * BLKQ
    # varlen smooth-K: ONE mean over all packed tokens (src/core.py:452-454), then the dense path per sequence without a mean
    km = oracle.mean_seq(k2[:, hk].float().cpu().numpy()[None, None], dtype)[0, 0]
    qr = q2[r0:lq[0], h].float().cpu().numpy()[None, None]
    kh = oracle.to_storage(k2[:lk[0], hk].float().cpu().numpy() - km, dtype)[None, None]
    vh = v2[:lk[0], hk].float().cpu().numpy()[None, None]
    orow = o[r0:lq[0], h].float().cpu().numpy()[None, None]
    assert bool(torch.isfinite(o).all())
    del q2, k2, v2, o
    _free()
    ro = oracle.lowbit_fa_forward(qr, kh, vh, dtype=dtype, smooth_k=False, tail="neg_inf", amax_floor=1e-7, q_blocks=[nq - 1])
    _o_bound(orow, ro, dtype)


def test_more_than_2_31_elements_hnd(oracle, dev):
    """HND, B H Sq D = 2^31 + 2^20 elements in Q and in O: the last (batch, head) starts past 2^31 elements (64-bit base offsets)."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, Sq, Sk, D, dtype = 2, 64, 131136, 256, 128, "fp16"
    assert B * H * Sq * D >= 2 ** 31 + 2 ** 20
    q = _randn((B, H, Sq, D), dtype, 14)
    k = _randn((B, H, Sk, D), dtype, 15, bias=0.5)
    v = _randn((B, H, Sk, D), dtype, 16)
    o, lse = lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, return_lse=True)
    blocks = [0, (Sq + BLKQ - 1) // BLKQ - 1]
    rows = torch.from_numpy(oracle.block_rows(blocks, Sq)).to(dev)
    qr = q[B - 1:, H - 1:, rows].float().cpu().numpy()
    kh, vh = (t[B - 1:, H - 1:].float().cpu().numpy() for t in (k, v))
    orow, lrow = o[B - 1:, H - 1:, rows].float().cpu().numpy(), lse[B - 1:, H - 1:, rows].cpu().numpy()
    assert bool(torch.isfinite(o[B - 1]).all())
    del q, k, v, o, lse
    _free()
    ro, rlse = oracle.lowbit_fa_forward(qr, kh, vh, dtype=dtype, return_lse=True, tail="neg_inf", amax_floor=1e-7, q_blocks=blocks)
    _o_bound(orow, ro, dtype)
    _lse_bound(lrow, rlse, _lse_bound_int8(rlse, dtype))
