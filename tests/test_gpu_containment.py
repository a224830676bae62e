"""Containment of every kernel's WRITES: outputs and workspaces inside guard bands (tests/guarded.py).

Each case runs a call once as it is and once inside a `GuardArena` - every `torch.empty` of the front end (outputs, workspaces,
gradient buffers) then sits between two 128 KiB bands of a sentinel byte -, asserts that the two results have the same bits (the
kernels are deterministic), that no guard byte changed, and that the guarded result meets the oracle at the bars the project
already has (`_o_close`, the LSE tolerance of test_gpu_fuzz.py, `_fp8_flip_close`, the backward's `grad_bound`,
`kvcache_reference.check_o` / `check_lse`).  The entry points that take output strides are also called through ctypes with an
output inside `guarded_out`: doubled token and head strides, 80 channels in 128-channel rows, and a workspace pointer inside
a guard buffer with exactly `*_workspace_bytes(...)` passed as its size.

Shapes: B 2, Hq 4, Hkv 2; Sq 129 (a second Q block of one row), Sk 65 (a second key tile of one key), causal 129 / 129;
head dims 64, 128, 80 (inside the 128 kernels), 40 (inside the 64 kernels), 36 (padded by the host); HND / NHD; fp16 / bf16 (bf16
adds the V-cast member of the workspace); LSE on.

Entry points of include/lowbit_fa.h that write device memory -> the cases here (reads: tests/test_gpu_hostile_memory.py):

    lbfa_forward                 test_dense_forward_is_contained (int8 / int4 / q8k4 / fp8), test_strided_outputs_by_ctypes
    lbfa_sdpa_fwd                test_dense_forward_is_contained[fp16], test_strided_outputs_by_ctypes
    lbfa_absmax                  test_router_statistic_and_router_are_contained
    lbfa_mean_seq                test_modular_entry_points_are_contained, test_contiguous_cache_is_contained (first append)
    lbfa_quant_per_block         test_modular_entry_points_are_contained
    lbfa_quant_v_fp8             test_modular_entry_points_are_contained
    lbfa_cast_bf16_to_f16        test_modular_entry_points_are_contained[bf16], test_modular_varlen_entry_points_are_contained[bf16]
    lbfa_attn_fwd                test_modular_entry_points_are_contained
    lbfa_quant_per_block_varlen  test_modular_varlen_entry_points_are_contained
    lbfa_attn_fwd_varlen         test_modular_varlen_entry_points_are_contained
    lbfa_forward_varlen          test_varlen_forward_is_contained (sageattn_varlen)
    lbfa_forward_varlen_lse      test_varlen_forward_is_contained (_varlen_attention), test_strided_outputs_by_ctypes
    lbfa_backward                test_dense_backward_is_contained
    lbfa_backward_varlen         test_varlen_backward_is_contained
    lbfa_kvcache_mean            test_contiguous_cache_is_contained / test_paged_cache_is_contained (ragged first append)
    lbfa_kvcache_append          test_contiguous_cache_is_contained
    lbfa_decode                  test_contiguous_cache_is_contained, test_strided_outputs_by_ctypes
    lbfa_kvcache_paged_append    test_paged_cache_is_contained
    lbfa_decode_paged            test_paged_cache_is_contained
    left out: lbfa_profile_next_attn (records two events, writes no device memory of the caller).

Mutants these cases are there for (a store one row, one channel chunk or one block too far):
  * the O store without `if (d0 >= p.d_valid) continue;`: test_strided_outputs_by_ctypes[lbfa_forward / lbfa_sdpa_fwd] - the
    channels 80 .. 127 of the 128-channel output rows no longer hold the sentinel; through the front end
    test_dense_forward_is_contained[D = 80 / 40] only sees it behind the last row (the other rows' padding is inside o).
  * `fwd_layout`'s `ks` member one block short at Sk = 65: test_dense_forward_is_contained at Sk = 65 (the member behind it is
    overwritten, so the result changes, or the last member runs into the guard) and test_strided_outputs_by_ctypes, whose
    workspace ends exactly at `lbfa_forward_workspace_bytes_dt`.
"""
import functools

import numpy as np
import pytest

import kvcache_reference as kr
from bwd_reference import attention_backward
from bwd_varlen_reference import varlen_backward, varlen_lse
from guarded import GuardArena, guarded_out
from oracle import lowbit_fa_oracle as orc
from test_gpu_backward import _assert_close, _grad_close
from test_gpu_parity import TDT, _canon, _fp8_flip_close, _np, _o_close, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B, HQ, HKV = 2, 4, 2
SQ, SK = 129, 65
LOG2E = 1.44269504
# layout, dtype, causal: both layouts, both dtypes and both masks meet every operator and head dim
COMBOS = [("HND", "fp16", False), ("NHD", "bf16", True), ("NHD", "fp16", True), ("HND", "bf16", False)]
HEAD_DIMS = [64, 128, 80, 40, 36]
# kind -> (operator, its extra arguments, the oracle's arguments)
KINDS = {
    "int8": ("lowbit_fa_qk_int8_pv_fp16_triton", {}, dict(tail="neg_inf")),
    "int4": ("lowbit_fa_qk_int4_pv_fp16_triton", dict(q_bits=4), dict(q_qmax=7, k_qmax=7, tail="neg_inf")),
    "q8k4": ("lowbit_fa_qk_int4_pv_fp16_triton", dict(q_bits=8), dict(k_qmax=7, tail="neg_inf")),
    "fp8": ("lowbit_fa_qk_int8_pv_fp8_cuda", {}, dict(pv="fp8", return_slack=True)),
    "fp16": ("flash_attn_fp16", {}, None),
}
VARLEN_LENS = {False: ([1, 129, 0, 64], [65, 1, 0, 130]), True: ([129, 1, 64], [129, 1, 64])}


def lens(causal):
    return (SQ, SQ) if causal else (SQ, SK)


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def same_bits(a, b, what):
    """two results (tensors, None or tuples of them) bit for bit"""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what} [{i}]")
        return
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} bytes differ"


def twice(monkeypatch, dev, call, what, min_allocations=1):
    """`call()` as it is and inside a GuardArena: the same bits, no guard byte touched -> the guarded result"""
    plain = call()
    with GuardArena(monkeypatch, dev) as arena:
        guarded = call()
    torch.cuda.synchronize()
    assert len(arena) >= min_allocations, f"{what}: only {len(arena)} allocations went through the arena"
    arena.check()
    same_bits(plain, guarded, what)
    return guarded


def operator(kind):
    import lowbit_quant_fa2_paddle_amd as lb
    name, extra, _ = KINDS[kind]
    fn = getattr(lb, name, None) or getattr(lb.core, name)
    return lambda *a, **kw: fn(*a, **extra, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# references, computed once per configuration and shared with tests/test_gpu_hostile_memory.py
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_reference(kind, D, layout, dtype, causal):
    """-> dict: q, k, v (numpy, in `layout`), o, lse, slack (fp8 only) of the oracle"""
    sq, sk = lens(causal)
    q, k, v = orc.make_inputs(B, HQ, sq, D, seed=100 + D, layout=layout, dtype=dtype, Hkv=HKV, Sk=sk, k_bias=0.5)
    okw = KINDS[kind][2]
    slack = None
    if okw is None:  # un-quantised: float64 softmax attention
        o, lse = orc.sdpa_naive(*(_canon(a, layout).astype(np.float64) for a in (q, k, v)), is_causal=causal, sm_scale=D ** -0.5,
                                return_lse=True)
        o = _canon(o, layout)  # (the transpose is its own inverse)
    else:
        with np.errstate(all="ignore"):
            res = orc.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True,
                                        amax_floor=1e-7, **okw)
        (o, slack, lse) = res if len(res) == 3 else (res[0], None, res[1])
    return dict(q=q, k=k, v=v, o=o, lse=lse, slack=slack)


def check_forward(kind, dtype, ref, o, lse, what):
    """the bars of tests/test_gpu_parity.py, test_gpu_fuzz.py and test_gpu_fp16.py"""
    on, ln = _np(o), _np(lse)
    assert on.shape == ref["o"].shape and np.isfinite(on).all() and np.isfinite(ln).all(), what
    if kind == "fp16":
        _o_close(on, ref["o"], dtype, atol=2e-3 if dtype == "fp16" else 4e-3)
        assert np.abs(ln - ref["lse"]).max() <= (1e-3 if dtype == "fp16" else 2.5e-3), what
        return
    if kind == "fp8":
        _fp8_flip_close(on, ref["o"], ref["slack"], dtype)
    else:
        _o_close(on, ref["o"], dtype)
    assert np.abs(ln - ref["lse"]).max() <= 2e-3 + 2.0 ** -9 * float(np.abs(ref["lse"]).max()), what


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the dense forward operators
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype,causal", COMBOS)
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_forward_is_contained(monkeypatch, dev, kind, D, layout, dtype, causal):
    ref = forward_reference(kind, D, layout, dtype, causal)
    tq, tk, tv = (_t(ref[x], dtype, dev) for x in "qkv")
    fn = operator(kind)
    what = f"{kind} D={D} {layout} {dtype} causal={causal}"
    # o, lse and - the quantised operators - the workspace
    o, lse = twice(monkeypatch, dev, lambda: fn(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True), what,
                   min_allocations=2 if kind == "fp16" else 3)
    check_forward(kind, dtype, ref, o, lse, what)


def test_router_statistic_and_router_are_contained(monkeypatch, dev):
    """`_absmax` writes three floats next to one another through `ptr + 4 i`; then the router itself on its three branches"""
    import lowbit_quant_fa2_paddle_amd as lb
    ref = forward_reference("int8", 64, "HND", "fp16", False)
    base = [_t(ref[x], "fp16", dev) for x in "qkv"]
    for mul, kind in ((1, "INT4"), (3, "INT8"), (8, "FP16")):
        t = [x * mul for x in base]
        plain = lb.core._absmax(t)
        with GuardArena(monkeypatch, dev) as arena:
            got = lb.core._absmax(t)
        arena.check()
        assert len(arena) == 1 and arena.allocations[0]["shape"] == (3,)
        assert got == plain == [float(x.abs().max()) for x in t], (got, plain)
        assert lb.core.select_quantization(*t) == kind
        o, lse = twice(monkeypatch, dev, lambda: lb.sageattn_multi_precision(*t, return_lse=True), f"router {kind}", min_allocations=3)
        direct = {"INT4": operator("int4"), "INT8": operator("int8"), "FP16": operator("fp16")}[kind](*t, return_lse=True)
        same_bits((o, lse), direct, f"router {kind} against its operator")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the modular entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype,D,causal", [("HND", "fp16", 64, False), ("NHD", "bf16", 128, True), ("NHD", "fp16", 128, False)])
def test_modular_entry_points_are_contained(monkeypatch, dev, layout, dtype, D, causal):
    """mean_seq, quantize (S = 129 at blk 128 without a mean and with a rowdot_vec, S = 65 at blk 64 with and without a mean),
    the fp8 V quantiser and attn_qk_int8_per_block.forward with an fp16 / bf16 and an fp8 V: km, codes and scales are the
    oracle's bits, O and the composed LSE within its bars"""
    from fp8_layout import decode_v_fp8
    from lowbit_quant_fa2_paddle_amd import attn_qk_int8_per_block as attn, quant, quant_per_block as qpb
    sq, sk = lens(causal)
    q, k, v = orc.make_inputs(B, HQ, sq, D, seed=7 + D, layout=layout, dtype=dtype, Hkv=HKV, Sk=sk, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    sm = D ** -0.5
    o_ref, lse_ref, mid = orc.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True,
                                                tail="neg_inf", amax_floor=1e-7, return_intermediates=True)
    run = lambda call, what, n=1: twice(monkeypatch, dev, call, f"{what} {layout} {dtype} D={D}", min_allocations=n)
    km = run(lambda: qpb.mean_seq(tk, layout), "mean_seq", 2)  # the mean and the fp64 partial sums
    assert np.array_equal(_np(km).reshape(mid["km"].shape), mid["km"])
    q8, qs, corr = run(lambda: qpb.quantize(tq, sm_scale=sm * LOG2E, qmax=127, blk=128, tensor_layout=layout, rowdot_vec=km),
                       "quantize q with a rowdot_vec", 3)
    q8b, qsb = run(lambda: qpb.quantize(tq, sm_scale=sm * LOG2E, qmax=127, blk=128, tensor_layout=layout), "quantize q", 2)
    same_bits((q8, qs), (q8b, qsb), "the rowdot_vec changes codes or scales")
    k8, ks = run(lambda: qpb.quantize(tk, sm_scale=1.0, qmax=127, blk=64, tensor_layout=layout, mean=km), "quantize k with a mean", 2)
    k8n, ksn = run(lambda: qpb.quantize(tk, sm_scale=1.0, qmax=127, blk=64, tensor_layout=layout), "quantize k without a mean", 2)
    for got, want in ((q8, "q_i8"), (k8, "k_i8")):
        assert np.array_equal(_canon(got.cpu().numpy(), layout), mid[want]), want
    for got, want in ((qs, "q_scale"), (ks, "k_scale")):
        assert tuple(got.shape) == mid[want].shape and np.array_equal(got.cpu().numpy().view(np.uint32), mid[want].view(np.uint32)), want
    _, _, k8_ref, ks_ref = orc.per_block_int8(_canon(q, layout), _canon(k, layout), None, sm, dtype, amax_floor=1e-7)
    assert np.array_equal(_canon(k8n.cpu().numpy(), layout), k8_ref) and np.array_equal(ksn.cpu().numpy().view(np.uint32), ks_ref.view(np.uint32))
    # attention on an fp16 / bf16 V (bf16: lbfa_cast_bf16_to_f16 into a guarded copy first)
    o, lse2 = run(lambda: attn.forward(q8, k8, tv, qs, ks, tensor_layout=layout, output_dtype=TDT[dtype], return_lse=True,
                                       is_causal=causal), "attn forward", 3 if dtype == "bf16" else 2)
    _o_close(_np(o), o_ref, dtype)
    lse = _np(lse2) / np.float32(LOG2E) + _np(corr) * np.float32(sm)
    assert np.abs(lse - lse_ref).max() <= 2e-3 + 2.0 ** -9 * float(np.abs(lse_ref).max())
    # the fp8 V quantiser (its padded keys 65 .. 127 are written as zeros, inside its buffer) and the fp8-PV kernel
    v8, vs, _ = run(lambda: (lambda r: (r[0].buf, r[1], None))(quant.per_channel_fp8(tv, tensor_layout=layout)), "per_channel_fp8", 2)
    ref8, ref_s = orc.per_channel_fp8(_canon(v, layout))
    assert np.array_equal(vs.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))
    got8 = decode_v_fp8(v8.cpu().numpy(), B, HKV, sk, D)
    assert np.array_equal(got8[:, :, :sk], orc.e4m3fn_encode(ref8)) and np.all(got8[:, :, sk:] == 0)
    o8, _ = run(lambda: attn.forward(q8, k8, quant.Fp8V(v8, B, HKV, sk, D), qs, ks, tensor_layout=layout, output_dtype=TDT[dtype],
                                     return_lse=True, is_causal=causal, v_scale=vs), "attn forward fp8", 2)
    with np.errstate(all="ignore"):
        o8_ref, slack, _ = orc.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True,
                                                 amax_floor=1e-7, pv="fp8", return_slack=True)
    _fp8_flip_close(_np(o8), o8_ref, slack, dtype)


def varlen_inputs(D, dtype, causal, Hq=HQ, Hkv=HKV):
    lq, lk = VARLEN_LENS[causal]
    return orc.make_varlen_inputs(lq, lk, Hq, Hkv, D, seed=50 + D, dtype=dtype, k_bias=0.5) + (max(lq), max(lk))


@pytest.mark.parametrize("dtype,D,causal", [("fp16", 64, False), ("bf16", 128, True), ("bf16", 64, False)])
def test_modular_varlen_entry_points_are_contained(monkeypatch, dev, dtype, D, causal):
    """quant_per_block_varlen.per_block_int8 and attn_qk_int8_block_varlen.forward on the packed lengths (a sequence of one row,
    one of 129, an empty one, one of 64): the oracle's packed codes and scales bit for bit, O within its bar"""
    from lowbit_quant_fa2_paddle_amd import attn_qk_int8_block_varlen as attn, quant_per_block_varlen as qpbv
    q, k, v, cu_q, cu_k, max_q, max_k = varlen_inputs(D, dtype, causal)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    tcq, tck = (torch.from_numpy(c).to(dev) for c in (cu_q, cu_k))
    o_ref, mid = orc.lowbit_fa_varlen(q, k, v, cu_q, cu_k, dtype=dtype, is_causal=causal, tail="neg_inf", amax_floor=1e-7,
                                      return_intermediates=True)
    km = _t(mid["km"], dtype, dev)
    q8, qs, k8, ks, cqs, cks = twice(monkeypatch, dev, lambda: qpbv.per_block_int8(tq, tk, tcq, tck, max_q, max_k, km=km),
                                     f"varlen per_block_int8 {dtype} D={D}", min_allocations=4)
    assert np.array_equal(q8.cpu().numpy(), mid["q_i8"]) and np.array_equal(k8.cpu().numpy(), mid["k_i8"])
    assert np.array_equal(qs.cpu().numpy().view(np.uint32), mid["q_scale"].view(np.uint32))
    assert np.array_equal(ks.cpu().numpy().view(np.uint32), mid["k_scale"].view(np.uint32))
    o = twice(monkeypatch, dev, lambda: attn.forward(q8, k8, tv, tcq, tck, max_q, qs, ks, cqs, cks, output_dtype=TDT[dtype],
                                                     is_causal=causal, max_seqlen_k=max_k),
              f"varlen attn forward {dtype} D={D}", min_allocations=2 if dtype == "bf16" else 1)
    _o_close(_np(o), o_ref, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. packed batches
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def varlen_reference(D, dtype, causal):
    q, k, v, cu_q, cu_k, max_q, max_k = varlen_inputs(D, dtype, causal)
    o = orc.lowbit_fa_varlen(q, k, v, cu_q, cu_k, dtype=dtype, is_causal=causal, tail="neg_inf", amax_floor=1e-7)
    lse, corr = varlen_lse(q, k, v, cu_q, cu_k, return_corr=True, dtype=dtype, is_causal=causal, smooth_k=True)
    return dict(q=q, k=k, v=v, cu_q=cu_q, cu_k=cu_k, max_q=max_q, max_k=max_k, o=o, lse=lse, corr=corr)


def check_varlen(dtype, ref, o, lse, what):
    """`_o_close`, and the LSE bound of test_gpu_varlen_backward.test_varlen_lse_vs_reference"""
    on = _np(o)
    assert np.isfinite(on).all(), what
    _o_close(on, ref["o"], dtype)
    if lse is None:
        return
    got, want = _np(lse).astype(np.float64), ref["lse"]
    fin = np.isfinite(want)
    assert np.all(got[~fin & ~np.isnan(want)] == -np.inf), what
    ulp = (2.0 ** -10 if dtype == "fp16" else 2.0 ** -7) * np.abs(ref["corr"][fin])
    assert np.all(np.abs(got[fin] - want[fin]) <= 2.0 ** -21 * np.abs(want[fin]) + 1e-3 + ulp), what


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128), ("fp16", 80), ("bf16", 40), ("fp16", 36)])
def test_varlen_forward_is_contained(monkeypatch, dev, dtype, D, causal):
    import lowbit_quant_fa2_paddle_amd as lb
    ref = varlen_reference(D, dtype, causal)
    tq, tk, tv = (_t(ref[x], dtype, dev) for x in "qkv")
    tcq, tck = (torch.from_numpy(ref[c]).to(dev) for c in ("cu_q", "cu_k"))
    what = f"varlen {dtype} D={D} causal={causal}"
    o = twice(monkeypatch, dev, lambda: lb.sageattn_varlen(tq, tk, tv, tcq, tck, ref["max_q"], ref["max_k"], is_causal=causal), what, 2)
    o2, lse = twice(monkeypatch, dev, lambda: lb.core._varlen_attention(tq, tk, tv, tcq, tck, ref["max_q"], ref["max_k"], is_causal=causal,
                                                                        sm_scale=None, smooth_k=True, q_qmax=127, k_qmax=127,
                                                                        return_lse=True), what + " with an LSE", 3)
    same_bits(o, o2, what + ": the LSE changes O")
    check_varlen(dtype, ref, o2, lse, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the backward, through autograd
# ---------------------------------------------------------------------------------------------------------------------------
def upstream(shape, dtype, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


@pytest.mark.parametrize("layout,dtype,causal", COMBOS)
@pytest.mark.parametrize("D", [64, 128, 80])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_dense_backward_is_contained(monkeypatch, dev, kind, D, layout, dtype, causal):
    """dq, dk, dv (and the backward's workspace) with a gradient into the LSE: bit-equal with and without the arena, inside
    their allocations, within `grad_bound`"""
    ref = forward_reference(kind, D, layout, dtype, causal)
    tq, tk, tv = (_t(ref[x], dtype, dev).requires_grad_() for x in "qkv")
    o, lse = operator(kind)(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True)
    do, dlse = upstream(o.shape, TDT[dtype], dev, 1), upstream(lse.shape, torch.float32, dev, 2)
    what = f"backward {kind} D={D} {layout} {dtype} causal={causal}"
    grads = twice(monkeypatch, dev, lambda: torch.autograd.grad((o, lse), (tq, tk, tv), (do, dlse), retain_graph=True), what, 4)
    qq, kq = (127, 127) if kind == "int8" else (7, 7)
    c = lambda a: _canon(a, layout)
    want = attention_backward(c(ref["q"]), c(ref["k"]), c(ref["v"]), c(_np(o)), _np(lse), c(_np(do)), sm_scale=D ** -0.5,
                              is_causal=causal, dtype=dtype, q_qmax=qq, k_qmax=kq, smooth_k=True, dlse=_np(dlse), return_bound=True)
    for name, got, rf, bnd in zip(("dq", "dk", "dv"), grads, want[:3], want[3:]):
        assert got.shape == {"dq": tq, "dk": tk, "dv": tv}[name].shape
        _assert_close(c(_np(got)), rf, dtype, f"{what} {name}")
        _grad_close(c(_np(got)), rf, bnd, f"{what} {name}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,D,qmax", [("fp16", 64, 127), ("bf16", 128, 7), ("fp16", 80, 127)])
def test_varlen_backward_is_contained(monkeypatch, dev, dtype, D, qmax, causal):
    from lowbit_quant_fa2_paddle_amd import core
    q, k, v, cu_q, cu_k, max_q, max_k = varlen_inputs(D, dtype, causal)
    tq, tk, tv = (_t(a, dtype, dev).requires_grad_() for a in (q, k, v))
    tcq, tck = (torch.from_numpy(c).to(dev) for c in (cu_q, cu_k))
    o, lse = core._varlen_attention(tq, tk, tv, tcq, tck, max_q, max_k, is_causal=causal, sm_scale=None, smooth_k=True, q_qmax=qmax,
                                    k_qmax=qmax, return_lse=True)
    do, dlse = upstream(o.shape, TDT[dtype], dev, 3), upstream(lse.shape, torch.float32, dev, 4)
    what = f"varlen backward {dtype} D={D} qmax={qmax} causal={causal}"
    grads = twice(monkeypatch, dev, lambda: torch.autograd.grad((o, lse), (tq, tk, tv), (do, dlse), retain_graph=True), what, 4)
    want = varlen_backward(q, k, v, _np(o), _np(lse).astype(np.float64), _np(do), cu_q, cu_k, dtype=dtype, is_causal=causal,
                           smooth_k=True, q_qmax=qmax, k_qmax=qmax, dlse=_np(dlse).astype(np.float64), return_bound=True)
    for name, got, rf, bnd in zip(("dq", "dk", "dv"), grads, want[:3], want[3:]):
        _assert_close(_np(got), rf, dtype, f"{what} {name}")
        _grad_close(_np(got), rf, bnd, f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the caches
# ---------------------------------------------------------------------------------------------------------------------------
CACHE_STATE = ("k_codes", "k_scale", "v", "k_tail", "km")
APPENDS = [(1, None), (63, None), (2, None), (200, [200, 7, 131])]  # T = 1; 63 then 2 (crossing a block); 200 with ragged new_lens
RAGGED_FIRST = [(5, [5, 0, 3])] + APPENDS                        # a ragged first append: lbfa_kvcache_mean


def arena_backed(cache, arena, names=CACHE_STATE, fill=None):
    """replace the state tensors of a cache by arena-backed ones with the same contents (or `fill`: name -> value)"""
    for name in names:
        t = getattr(cache, name)
        if t is not None:
            setattr(cache, name, arena.like(t, None if fill is None else fill[name]))
    return cache


def cache_data(D, dtype, schedule, Bc=3, seed=0):
    """k, v [Bc, HKV, T, D] of every append of `schedule` (numpy, storage dtype)"""
    rng = np.random.default_rng(seed)
    mk = lambda T, bias: orc.to_storage(rng.standard_normal((Bc, HKV, T, D), dtype=np.float32) + np.float32(bias), dtype)
    return [(mk(T, 0.5), mk(T, 0.0)) for T, _ in schedule]


def run_schedule(cache, data, schedule, dtype, dev, ref=None, **kw):
    for (T, nl), (k, v) in zip(schedule, data):
        tl = None if nl is None else torch.tensor(nl, dtype=torch.int32, device=dev)
        cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=tl, **kw)
        if ref is not None:
            ref.append(k, v, nl)
    return cache


def state_equals_ref(cache, ref, what):
    """the valid part of a contiguous cache against the numpy cache (as tests/test_gpu_decode_fuzz.py)"""
    assert np.array_equal(cache.seqlens.cpu().numpy(), ref.seqlens), what
    codes, scales, v = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy(), _np(cache.v)
    for b, n in enumerate(int(x) for x in ref.seqlens):
        nb = (n + 63) // 64
        assert np.array_equal(codes[b, :, :n], ref.k_codes[b, :, :n]), (what, b, "codes")
        assert np.array_equal(scales[b, :, :nb].view(np.uint32), ref.k_scale[b, :, :nb].view(np.uint32)), (what, b, "scales")
        assert np.array_equal(v[b, :, :n], ref.v[b, :, :n]), (what, b, "v")
    assert np.array_equal(_np(cache.km), ref.km), (what, "km")


def decode_reference(q, ref, seqlens, dtype, causal):
    """the oracle's kernel on the numpy cache (tests/kvcache_reference.py): q [B, Hq, Sq, D] canonical -> o, lse, corr, sm_scale"""
    sm = q.shape[-1] ** -0.5
    q_i8, q_scale = kr.quant_q(orc, q, sm, 127)
    corr = kr.lse_correction(orc, q, ref.km, dtype)
    o, lse2 = kr.oracle_decode(orc, q_i8, q_scale, ref.k_codes, ref.k_scale, ref.v, np.asarray(seqlens), causal=causal, out_dtype=dtype)
    return o, kr.natural_lse(lse2, corr, sm), corr, sm


def decode_cases(D, dtype, dev, Bc=3, G=2):
    """(Sq, causal, layout, q numpy canonical, q tensor in layout)"""
    out = []
    for Sq, causal, layout in ((1, False, "HND"), (3, True, "NHD")):
        q = orc.to_storage(np.random.default_rng(Sq).standard_normal((Bc, G * HKV, Sq, D), dtype=np.float32), dtype)
        tq = _t(q if layout == "HND" else np.transpose(q, (0, 2, 1, 3)), dtype, dev)
        out.append((Sq, causal, layout, q, tq))
    return out


def check_decode(monkeypatch, dev, cache, ref, D, dtype, what, twin=None, **kw):
    """decode with one slice (writes o directly) and three (the partials workspace and the combine kernel), Sq 1 and 3 causal"""
    import lowbit_quant_fa2_paddle_amd as lb
    for Sq, causal, layout, q, tq in decode_cases(D, dtype, dev):
        o_ref, lse_ref, corr, sm = decode_reference(q, ref, ref.seqlens, dtype, causal)
        for ns in (1, 3):
            w = f"{what} Sq={Sq} splits={ns}"
            call = lambda c=cache: lb.lowbit_fa_decode(tq, c, tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns, **kw)
            o, lse = twice(monkeypatch, dev, call, w, min_allocations=3)
            on = _np(o if layout == "HND" else o.transpose(1, 2))
            assert not np.isnan(on).any(), w
            kr.check_o(on, o_ref, dtype, w)
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, w)
            if twin is not None:
                same_bits((o, lse), call(twin), w + ": against the cache in plain memory")


@pytest.mark.parametrize("dtype,D,schedule", [("fp16", 64, APPENDS), ("bf16", 128, APPENDS), ("fp16", 128, RAGGED_FIRST)])
def test_contiguous_cache_is_contained(monkeypatch, dev, dtype, D, schedule):
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap = 3, 320
    data = cache_data(D, dtype, schedule)
    ref = kr.CacheRef(orc, Bc, HKV, D, cap, dtype)
    plain = run_schedule(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), data, schedule, dtype, dev, ref=ref)
    arena = GuardArena(monkeypatch, dev)
    cache = arena_backed(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), arena)
    with arena:  # the mean's workspace of the first append
        run_schedule(cache, data, schedule, dtype, dev)
    torch.cuda.synchronize()
    arena.check()
    what = f"contiguous cache {dtype} D={D}"
    for name in CACHE_STATE + ("seqlens",):
        same_bits(getattr(plain, name), getattr(cache, name), f"{what}: {name}")
    state_equals_ref(cache, ref, what)
    check_decode(monkeypatch, dev, cache, ref, D, dtype, what, twin=plain)
    arena.check()  # decode wrote nothing around the cache either


@pytest.mark.parametrize("dtype,D,page,schedule", [("fp16", 64, 64, APPENDS), ("bf16", 128, 128, APPENDS), ("fp16", 128, 64, RAGGED_FIRST)])
def test_paged_cache_is_contained(monkeypatch, dev, dtype, D, page, schedule):
    """the same schedules through a pool of pages handed out in a scrambled order: the pool, the tails and the means are
    arena-backed, the state and the decode equal the contiguous cache's bit for bit (which the test above ties to the oracle)"""
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap = 3, 320
    max_pages = -(-cap // page)
    data = cache_data(D, dtype, schedule)
    ref = kr.CacheRef(orc, Bc, HKV, D, cap, dtype)
    dense = run_schedule(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), data, schedule, dtype, dev, ref=ref)
    order = np.random.default_rng(page).permutation(Bc * max_pages + 2).tolist()
    arena = GuardArena(monkeypatch, dev)
    paged = arena_backed(lb.LowbitPagedKVCache(Bc * max_pages + 2, page, HKV, D, Bc, max_pages, TDT[dtype], dev, page_order=order), arena)
    with arena:  # km_new and the mean's workspace of the first append
        run_schedule(paged, data, schedule, dtype, dev)
    torch.cuda.synchronize()
    arena.check()
    what = f"paged cache {dtype} D={D} page={page}"
    assert torch.equal(paged.seqlens, dense.seqlens), what
    for b, n in enumerate(dense.seqlens.tolist()):
        codes, scales, v = paged.gather(b)
        nb = (n + 63) // 64
        same_bits(codes[:, :n], dense.k_codes[b, :, :n], f"{what}: codes of {b}")
        same_bits(scales[:, :nb], dense.k_scale[b, :, :nb], f"{what}: scales of {b}")
        same_bits(v[:, :n], dense.v[b, :, :n], f"{what}: v of {b}")
    same_bits(paged.km, dense.km, what + ": km")
    same_bits(paged.k_tail, dense.k_tail, what + ": k_tail")
    # the two spare pages were handed to nobody: still zero
    spare = torch.tensor(paged.allocator.free_pages, device=dev)
    assert not paged.k_codes[spare].any() and not paged.v[spare].any() and not paged.k_scale[spare].any(), what
    check_decode(monkeypatch, dev, paged, ref, D, dtype, what, twin=dense)
    arena.check()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. outputs with strides, by ctypes: gaps between rows and heads, 80 channels in 128-channel rows, an exact workspace
# ---------------------------------------------------------------------------------------------------------------------------
def exact_workspace(arena, nbytes):
    """a workspace of exactly `nbytes` bytes whose last byte is the last one before the guard"""
    return arena.allocate((max(nbytes, 16),), torch.uint8) if nbytes else None


@pytest.mark.parametrize("layout,dtype,causal", COMBOS)
@pytest.mark.parametrize("entry", ["lbfa_forward", "lbfa_forward_fp8", "lbfa_sdpa_fwd"])
def test_strided_outputs_by_ctypes(monkeypatch, dev, entry, layout, dtype, causal):
    """D = 80 in 128-channel output rows with doubled token and head strides: the channels 80 .. 127 of every row, the rows and
    the heads in between keep the sentinel, O and LSE are the front end's bits"""
    from cabi_calls import call_gpu
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    D, Dbuf = 80, 128
    kind = {"lbfa_forward": "int8", "lbfa_forward_fp8": "fp8", "lbfa_sdpa_fwd": "fp16"}[entry]
    ref = forward_reference(kind, D, layout, dtype, causal)
    tq, tk, tv = (_t(ref[x], dtype, dev) for x in "qkv")
    sq, sk = lens(causal)
    o_want, lse_want = operator(kind)(tq, tk, tv, tensor_layout=layout, is_causal=causal, return_lse=True)
    # [B, H, S] order of the strides whatever the layout; token rows of 2 * Dbuf, heads twice as far apart as they need be
    if layout == "HND":
        so = (HQ * 2 * sq * 2 * Dbuf, 2 * sq * 2 * Dbuf, 2 * Dbuf)
    else:
        so = (sq * HQ * 2 * 2 * Dbuf, 2 * Dbuf, HQ * 2 * 2 * Dbuf)
    o, check = guarded_out((B, HQ, sq, D), TDT[dtype], so + (1,), dev)
    arena = GuardArena(monkeypatch, dev)
    lse = arena.allocate((B, HQ, sq), torch.float32)
    st = lambda t: tuple(t.stride()[i] for i in ((0, 1, 2) if layout == "HND" else (0, 2, 1)))
    code = _lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16
    common = dict(q=tq.data_ptr(), k=tk.data_ptr(), v=tv.data_ptr(), dtype=code, o=o.data_ptr(), lse=lse.data_ptr(), B=B, Hq=HQ,
                  Hkv=HKV, Sq=sq, Sk=sk, D=D, sq=st(tq), sk=st(tk), sv=st(tv), so=so, sm_scale=D ** -0.5, causal=int(causal),
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    if entry == "lbfa_sdpa_fwd":
        call_gpu(lib, "lbfa_sdpa_fwd", **common)
    else:
        fp8 = int(kind == "fp8")
        nbytes = lib.lbfa_forward_workspace_bytes_dt(B, HQ, HKV, sq, sk, D, code, fp8, 1, 1)
        ws = exact_workspace(arena, nbytes)
        call_gpu(lib, "lbfa_forward", workspace=ws.data_ptr(), workspace_bytes=nbytes, q_qmax=127, k_qmax=127, pv_fp8=fp8, smooth_k=1,
                 **common)
    torch.cuda.synchronize()
    what = f"{entry} {layout} {dtype} causal={causal}"
    check(what)
    arena.check()
    got = o if layout == "HND" else o.transpose(1, 2)
    same_bits(got, o_want, what + ": O")
    same_bits(lse, lse_want, what + ": LSE")


@pytest.mark.parametrize("dtype,D,causal", [("fp16", 64, False), ("bf16", 128, True), ("fp16", 80, False)])
def test_strided_varlen_output_by_ctypes(monkeypatch, dev, dtype, D, causal):
    """lbfa_forward_varlen_lse into a packed output with doubled token and head strides (D = 80: 80-channel rows, the kernels work
    on 128 channels and must leave the gap behind every row alone) and an exact workspace"""
    from cabi_calls import call_gpu
    from lowbit_quant_fa2_paddle_amd import _lib, core
    lib = _lib.load()
    ref = varlen_reference(D, dtype, causal)
    tq, tk, tv = (_t(ref[x], dtype, dev) for x in "qkv")
    tcq, tck = (torch.from_numpy(ref[c]).to(dev) for c in ("cu_q", "cu_k"))
    o_want, lse_want = core._varlen_attention(tq, tk, tv, tcq, tck, ref["max_q"], ref["max_k"], is_causal=causal, sm_scale=None,
                                              smooth_k=True, q_qmax=127, k_qmax=127, return_lse=True)
    total_q, total_k = tq.shape[0], tk.shape[0]
    so = (2 * D, HQ * 2 * 2 * D)  # {head, token}
    o, check = guarded_out((total_q, HQ, D), TDT[dtype], (so[1], so[0], 1), dev)
    arena = GuardArena(monkeypatch, dev)
    lse = arena.allocate((HQ, total_q), torch.float32)
    code = _lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16
    nbytes = lib.lbfa_forward_varlen_workspace_bytes_dt(len(ref["cu_q"]) - 1, HQ, HKV, total_q, total_k, ref["max_q"], ref["max_k"], D, code)
    ws = exact_workspace(arena, nbytes)
    hs = lambda t: (t.stride(1), t.stride(0))
    call_gpu(lib, "lbfa_forward_varlen_lse", q=tq.data_ptr(), k=tk.data_ptr(), v=tv.data_ptr(), dtype=code, o=o.data_ptr(),
             lse=lse.data_ptr(), cu_q=tcq.data_ptr(), cu_k=tck.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes,
             B=len(ref["cu_q"]) - 1, Hq=HQ, Hkv=HKV, total_q=total_q, total_k=total_k, max_q=ref["max_q"], max_k=ref["max_k"], D=D,
             sq=hs(tq), sk=hs(tk), sv=hs(tv), so=so, sm_scale=D ** -0.5, q_qmax=127, k_qmax=127, causal=int(causal), smooth_k=1,
             stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    what = f"lbfa_forward_varlen_lse {dtype} D={D} causal={causal}"
    check(what)
    arena.check()
    same_bits(o, o_want, what + ": O")
    same_bits(lse, lse_want, what + ": LSE")


@pytest.mark.parametrize("dtype,D,Sq,causal,ns", [("fp16", 64, 1, False, 1), ("bf16", 128, 3, True, 3), ("fp16", 128, 3, True, 1),
                                                  ("bf16", 64, 1, False, 3)])
def test_strided_decode_output_by_ctypes(monkeypatch, dev, dtype, D, Sq, causal, ns):
    """lbfa_decode into an output with doubled token and head strides; with three slices the partials live in a workspace of
    exactly lbfa_decode_workspace_bytes"""
    import lowbit_quant_fa2_paddle_amd as lb
    from cabi_calls import call_gpu
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    Bc, cap, G = 3, 320, 2
    Hq = G * HKV
    data = cache_data(D, dtype, APPENDS)
    cache = run_schedule(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), data, APPENDS, dtype, dev)
    q = upstream((Bc, Hq, Sq, D), TDT[dtype], dev, 9)
    o_want, lse_want = lb.lowbit_fa_decode(q, cache, is_causal=causal, return_lse=True, num_splits=ns)
    so = (Hq * 2 * Sq * 2 * D, 2 * Sq * 2 * D, 2 * D)
    o, check = guarded_out((Bc, Hq, Sq, D), TDT[dtype], so + (1,), dev)
    arena = GuardArena(monkeypatch, dev)
    lse = arena.allocate((Bc, Hq, Sq), torch.float32)
    max_k = min(cache.max_seqlen, cache.capacity)
    nbytes = lib.lbfa_decode_workspace_bytes(Bc, Hq, HKV, Sq, D, max_k, ns)
    assert (nbytes > 0) == (ns > 1)
    ws = exact_workspace(arena, nbytes)
    call_gpu(lib, "lbfa_decode", q=q.data_ptr(), dtype=_lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16,
             k_codes=cache.k_codes.data_ptr(), k_scale=cache.k_scale.data_ptr(), v_cache=cache.v.data_ptr(), km=cache.km.data_ptr(),
             seqlens=cache.seqlens.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), workspace=ws.data_ptr() if ws is not None else None,
             workspace_bytes=nbytes, B=Bc, Hq=Hq, Hkv=HKV, Sq=Sq, D=D, capacity=cap, max_seqlen_k=max_k, num_splits=ns,
             sq=tuple(q.stride()[:3]), so=so, sm_scale=D ** -0.5, q_qmax=127, causal=int(causal),
             stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    what = f"lbfa_decode {dtype} D={D} Sq={Sq} splits={ns}"
    check(what)
    arena.check()
    same_bits(o, o_want, what + ": O")
    same_bits(lse, lse_want, what + ": LSE")
