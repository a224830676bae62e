"""Containment of every kernel's READS, and the device-side defences of include/lowbit_fa.h, in hostile memory.

Part 1 - reads.  The shapes of tests/test_gpu_containment.py; q, k, v (and dO, the codes and scales of the modular entry points,
the new tokens of a cache append) are `hostile_view`s (tests/guarded.py): NaN (codes -128, scales +inf) before row 0 and behind
the last row of every (batch, head), between heads and batches, and in the channels 80 .. 127 / 40 .. 63 of every row when the
head dim is 80 / 40.  A masked key whose V row was fetched from there gives 0 x NaN = NaN.  Every result must be finite where
the oracle's is, bit-equal to the same call on contiguous copies (strides alone change no bits:
test_strided_operands_give_the_bits_of_contiguous_ones), and within the oracle's bar.  The unwritten part of a cache is codes
-128, scales +inf, V NaN; decode runs at the lengths 1, 63, 64, 65 and 130.

Part 2 - the defences.  The front end refuses a length past the capacity, a slot or a page out of range before it launches, so
these tests put the bad value on the device behind its back, or call the C ABI directly.

    THE RULE: every out-of-range value is chosen so that the address an undefended kernel would form from it still lies inside
    a buffer this test allocated.  A missing defence then shows as a touched guard, a changed neighbour or a NaN - never as a
    fault.  The reachable address is derived next to each constant below.

Entry points of include/lowbit_fa.h that write device memory -> the cases here (writes: tests/test_gpu_containment.py):

    lbfa_forward, lbfa_sdpa_fwd                       test_dense_forward_reads_only_its_operands
    lbfa_absmax                                       test_router_statistic_reads_only_its_operands
    lbfa_mean_seq, lbfa_quant_per_block, lbfa_quant_v_fp8, lbfa_cast_bf16_to_f16, lbfa_attn_fwd
                                                      test_modular_entry_points_read_only_their_operands
    lbfa_quant_per_block_varlen, lbfa_attn_fwd_varlen test_modular_varlen_entry_points_read_only_their_operands
    lbfa_forward_varlen, lbfa_forward_varlen_lse      test_varlen_forward_reads_only_its_operands
    lbfa_backward                                     test_dense_backward_reads_only_its_operands
    lbfa_backward_varlen                              test_varlen_backward_reads_only_its_operands
    lbfa_kvcache_mean, lbfa_kvcache_append, lbfa_decode
                                                      test_contiguous_cache_in_hostile_memory, test_append_at_the_capacity_drops_rows,
                                                      test_append_clamps_negative_lengths, test_decode_clamps_the_lengths
    lbfa_kvcache_paged_append, lbfa_decode_paged      test_paged_cache_in_hostile_memory, test_paged_append_skips_corrupt_ids,
                                                      test_paged_decode_clamps_corrupt_ids
    left out: lbfa_profile_next_attn (writes no device memory of the caller).

Mutants these cases are there for:
  * `append_range` without `tb = min(tb, p.cap - s0)`: test_append_at_the_capacity_drops_rows - batch 1 (full) changes, rows
    0 .. 4 of the head or batch behind batch 0 change.
  * the V fetch of the decode kernel's last tile unguarded (`store_v` without its `t * 64 + r < n`): test_contiguous_cache_in_hostile_memory
    and test_paged_cache_in_hostile_memory at the lengths 1, 63, 65 and 130 - the rows behind the end hold NaN, 0 x NaN = NaN in O.
"""
import numpy as np
import pytest

import kvcache_reference as kr
from bwd_reference import attention_backward
from bwd_varlen_reference import varlen_backward
from guarded import GuardArena, hostile_fill, hostile_view
from oracle import lowbit_fa_oracle as orc
from test_gpu_backward import _assert_close, _grad_close
from test_gpu_containment import (B, COMBOS, HEAD_DIMS, HKV, HQ, KINDS, LOG2E, arena_backed, bits, cache_data, check_forward,  # noqa: F401
                                  check_varlen, decode_cases, decode_reference, forward_reference, lens, operator, same_bits,
                                  state_equals_ref, upstream, varlen_inputs, varlen_reference)
from test_gpu_parity import TDT, _canon, _fp8_flip_close, _np, _o_close, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def hostile(t, scale=False):
    """`t` inside hostile memory: one hostile row / head / batch (token / head for a packed tensor) before and behind it in every
    dimension but the last, and hostile channels up to 64 / 128 behind every row"""
    D = t.shape[-1]
    Dbuf = D if D in (64, 128) else (64 if D < 64 else 128)
    n = t.dim() - 1
    return hostile_view(t, before=(1,) * n + (0,), after=(1,) * n + (Dbuf - D,), fill=hostile_fill(t.dtype, scale))


def hostile_rows(t, scale=False):
    """a tensor the ABI wants contiguous (scales, means, the fp8 V buffer): hostile memory before and behind it"""
    pad = 1 if t.dim() > 1 else 256
    return hostile_view(t, before=(pad,) + (0,) * (t.dim() - 1), after=(pad,) + (0,) * (t.dim() - 1),
                        fill=0x7F if t.dtype == torch.uint8 else hostile_fill(t.dtype, scale), check_abi=False)  # 0x7f: e4m3 NaN


def clean(t):
    return t.clone(memory_format=torch.contiguous_format)


def finite(x, what):
    for t in (x if isinstance(x, (tuple, list)) else (x,)):
        if t is not None and t.is_floating_point():
            assert torch.isfinite(t).all(), f"{what}: a non-finite value - hostile memory was read"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. reads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype,causal", COMBOS)
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_forward_reads_only_its_operands(dev, kind, D, layout, dtype, causal):
    ref = forward_reference(kind, D, layout, dtype, causal)
    hq, hk, hv = (hostile(_t(ref[x], dtype, dev)) for x in "qkv")
    assert hq.stride(-2) in (64, 128) and not hq.is_contiguous()
    fn = operator(kind)
    what = f"{kind} D={D} {layout} {dtype} causal={causal}"
    got = fn(hq, hk, hv, tensor_layout=layout, is_causal=causal, return_lse=True)
    finite(got, what)
    same_bits(got, fn(clean(hq), clean(hk), clean(hv), tensor_layout=layout, is_causal=causal, return_lse=True), what)
    check_forward(kind, dtype, ref, *got, what)


def test_router_statistic_reads_only_its_operands(dev):
    import lowbit_quant_fa2_paddle_amd as lb
    ref = forward_reference("int8", 80, "NHD", "bf16", True)
    t = [hostile(_t(ref[x], "bf16", dev)) for x in "qkv"]
    got = lb.core._absmax(t)
    assert got == [float(x.abs().max()) for x in t] and all(np.isfinite(got)), got


@pytest.mark.parametrize("layout,dtype,D,causal", [("HND", "fp16", 64, False), ("NHD", "bf16", 128, True), ("NHD", "fp16", 128, False)])
def test_modular_entry_points_read_only_their_operands(dev, layout, dtype, D, causal):
    """x and the mean of the quantisers, the codes, the scales, V (16-bit and fp8) and the V scale of the attention kernel"""
    from lowbit_quant_fa2_paddle_amd import attn_qk_int8_per_block as attn, quant, quant_per_block as qpb
    sq, sk = lens(causal)
    q, k, v = orc.make_inputs(B, HQ, sq, D, seed=7 + D, layout=layout, dtype=dtype, Hkv=HKV, Sk=sk, k_bias=0.5)
    cq, ck, cv = (_t(a, dtype, dev) for a in (q, k, v))
    hq, hk, hv = hostile(cq), hostile(ck), hostile(cv)
    sm = D ** -0.5
    what = f"{layout} {dtype} D={D}"
    km = qpb.mean_seq(hk, layout)
    same_bits(km, qpb.mean_seq(ck, layout), what + ": mean_seq")
    hkm = hostile_rows(km)
    q8, qs, corr = qpb.quantize(hq, sm_scale=sm * LOG2E, qmax=127, blk=128, tensor_layout=layout, rowdot_vec=hkm)
    same_bits((q8, qs, corr), qpb.quantize(cq, sm_scale=sm * LOG2E, qmax=127, blk=128, tensor_layout=layout, rowdot_vec=km), what + ": q")
    k8, ks = qpb.quantize(hk, sm_scale=1.0, qmax=127, blk=64, tensor_layout=layout, mean=hkm)
    same_bits((k8, ks), qpb.quantize(ck, sm_scale=1.0, qmax=127, blk=64, tensor_layout=layout, mean=km), what + ": k")
    same_bits(qpb.quantize(hk, sm_scale=1.0, qmax=7, blk=64, tensor_layout=layout),
              qpb.quantize(ck, sm_scale=1.0, qmax=7, blk=64, tensor_layout=layout), what + ": k without a mean")
    finite((km, qs, ks, corr), what)
    kw = dict(tensor_layout=layout, output_dtype=TDT[dtype], return_lse=True, is_causal=causal)
    got = attn.forward(hostile(q8), hostile(k8), hv, hostile_rows(qs, scale=True), hostile_rows(ks, scale=True), **kw)
    finite(got, what + ": attn forward")
    same_bits(got, attn.forward(q8, k8, cv, qs, ks, **kw), what + ": attn forward")
    o_ref, lse_ref = orc.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True,
                                           tail="neg_inf", amax_floor=1e-7)
    _o_close(_np(got[0]), o_ref, dtype)
    lse = _np(got[1]) / np.float32(LOG2E) + _np(corr) * np.float32(sm)
    assert np.abs(lse - lse_ref).max() <= 2e-3 + 2.0 ** -9 * float(np.abs(lse_ref).max())
    # fp8 V: the quantiser reads a hostile V, the kernel a hostile fp8 buffer and V scale
    v8, vs, _ = quant.per_channel_fp8(hv, tensor_layout=layout)
    v8c, vsc, _ = quant.per_channel_fp8(cv, tensor_layout=layout)
    same_bits((v8.buf, vs), (v8c.buf, vsc), what + ": per_channel_fp8")
    finite(vs, what)
    got8 = attn.forward(hostile(q8), hostile(k8), quant.Fp8V(hostile_rows(v8.buf), B, HKV, sk, D), hostile_rows(qs, scale=True),
                        hostile_rows(ks, scale=True), v_scale=hostile_rows(vs, scale=True), **kw)
    finite(got8, what + ": attn forward fp8")
    same_bits(got8, attn.forward(q8, k8, v8c, qs, ks, v_scale=vsc, **kw), what + ": attn forward fp8")
    with np.errstate(all="ignore"):
        o8_ref, slack, _ = orc.lowbit_fa_forward(q, k, v, dtype=dtype, tensor_layout=layout, is_causal=causal, return_lse=True,
                                                 amax_floor=1e-7, pv="fp8", return_slack=True)
    _fp8_flip_close(_np(got8[0]), o8_ref, slack, dtype)


@pytest.mark.parametrize("dtype,D,causal", [("fp16", 64, False), ("bf16", 128, True), ("bf16", 64, False)])
def test_modular_varlen_entry_points_read_only_their_operands(dev, dtype, D, causal):
    from lowbit_quant_fa2_paddle_amd import attn_qk_int8_block_varlen as attn, quant_per_block_varlen as qpbv
    q, k, v, cu_q, cu_k, max_q, max_k = varlen_inputs(D, dtype, causal)
    cq, ck, cv = (_t(a, dtype, dev) for a in (q, k, v))
    tcq, tck = (torch.from_numpy(c).to(dev) for c in (cu_q, cu_k))
    o_ref, mid = orc.lowbit_fa_varlen(q, k, v, cu_q, cu_k, dtype=dtype, is_causal=causal, tail="neg_inf", amax_floor=1e-7,
                                      return_intermediates=True)
    km = _t(mid["km"], dtype, dev)
    what = f"varlen {dtype} D={D} causal={causal}"
    got = qpbv.per_block_int8(hostile(cq), hostile(ck), tcq, tck, max_q, max_k, km=hostile_rows(km))
    want = qpbv.per_block_int8(cq, ck, tcq, tck, max_q, max_k, km=km)
    same_bits(got, want, what + ": per_block_int8")
    q8, qs, k8, ks, cqs, cks = want
    finite((qs, ks), what)
    kw = dict(output_dtype=TDT[dtype], is_causal=causal, max_seqlen_k=max_k)
    o = attn.forward(hostile(q8), hostile(k8), hostile(cv), tcq, tck, max_q, hostile_rows(qs, scale=True), hostile_rows(ks, scale=True),
                     cqs, cks, **kw)
    finite(o, what)
    same_bits(o, attn.forward(q8, k8, cv, tcq, tck, max_q, qs, ks, cqs, cks, **kw), what + ": attn forward")
    _o_close(_np(o), o_ref, dtype)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128), ("fp16", 80), ("bf16", 40)])
def test_varlen_forward_reads_only_its_operands(dev, dtype, D, causal):
    import lowbit_quant_fa2_paddle_amd as lb
    ref = varlen_reference(D, dtype, causal)
    hq, hk, hv = (hostile(_t(ref[x], dtype, dev)) for x in "qkv")
    tcq, tck = (torch.from_numpy(ref[c]).to(dev) for c in ("cu_q", "cu_k"))
    what = f"varlen {dtype} D={D} causal={causal}"
    kw = dict(is_causal=causal, sm_scale=None, smooth_k=True, q_qmax=127, k_qmax=127, return_lse=True)
    got = lb.core._varlen_attention(hq, hk, hv, tcq, tck, ref["max_q"], ref["max_k"], **kw)
    assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
    same_bits(got, lb.core._varlen_attention(clean(hq), clean(hk), clean(hv), tcq, tck, ref["max_q"], ref["max_k"], **kw), what)
    same_bits(got[0], lb.sageattn_varlen(hq, hk, hv, tcq, tck, ref["max_q"], ref["max_k"], is_causal=causal), what + ": without an LSE")
    check_varlen(dtype, ref, *got, what)


def _grads(fn, tensors, do, dlse):
    """forward with grad on detached leaves with the strides of `tensors`, one backward -> (o, lse, dq, dk, dv)"""
    leaves = [t.detach().requires_grad_() for t in tensors]
    o, lse = fn(*leaves)
    return (o.detach(), lse.detach()) + tuple(torch.autograd.grad((o, lse), leaves, (do, dlse)))


@pytest.mark.parametrize("layout,dtype,causal", COMBOS)
@pytest.mark.parametrize("D", [64, 128, 80])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_dense_backward_reads_only_its_operands(dev, kind, D, layout, dtype, causal):
    """q, k, v and dO hostile: the backward addresses them with plain loads and per-lane guards, no descriptor windows"""
    ref = forward_reference(kind, D, layout, dtype, causal)
    h = [hostile(_t(ref[x], dtype, dev)) for x in "qkv"]
    fn = lambda a, b, c: operator(kind)(a, b, c, tensor_layout=layout, is_causal=causal, return_lse=True)
    do = upstream(h[0].shape, TDT[dtype], dev, 1)
    dlse = upstream((B, HQ, lens(causal)[0]), torch.float32, dev, 2)
    what = f"backward {kind} D={D} {layout} {dtype} causal={causal}"
    got = _grads(fn, h, hostile(do), dlse)
    finite(got, what)
    same_bits(got, _grads(fn, [clean(t) for t in h], do, dlse), what)
    qq, kq = (127, 127) if kind == "int8" else (7, 7)
    c = lambda a: _canon(a, layout)
    want = attention_backward(c(ref["q"]), c(ref["k"]), c(ref["v"]), c(_np(got[0])), _np(got[1]), c(_np(do)), sm_scale=D ** -0.5,
                              is_causal=causal, dtype=dtype, q_qmax=qq, k_qmax=kq, smooth_k=True, dlse=_np(dlse), return_bound=True)
    for name, g, rf, bnd in zip(("dq", "dk", "dv"), got[2:], want[:3], want[3:]):
        _assert_close(c(_np(g)), rf, dtype, f"{what} {name}")
        _grad_close(c(_np(g)), rf, bnd, f"{what} {name}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,D,qmax", [("fp16", 64, 127), ("bf16", 128, 7), ("fp16", 80, 127)])
def test_varlen_backward_reads_only_its_operands(dev, dtype, D, qmax, causal):
    from lowbit_quant_fa2_paddle_amd import core
    q, k, v, cu_q, cu_k, max_q, max_k = varlen_inputs(D, dtype, causal)
    h = [hostile(_t(a, dtype, dev)) for a in (q, k, v)]
    tcq, tck = (torch.from_numpy(c).to(dev) for c in (cu_q, cu_k))
    fn = lambda a, b, c: core._varlen_attention(a, b, c, tcq, tck, max_q, max_k, is_causal=causal, sm_scale=None, smooth_k=True,
                                                q_qmax=qmax, k_qmax=qmax, return_lse=True)
    do = upstream(h[0].shape, TDT[dtype], dev, 3)
    dlse = upstream((HQ, h[0].shape[0]), torch.float32, dev, 4)
    what = f"varlen backward {dtype} D={D} qmax={qmax} causal={causal}"
    got = _grads(fn, h, hostile(do), dlse)
    assert all(torch.isfinite(t).all() for t in (got[0],) + got[2:]), what
    same_bits(got, _grads(fn, [clean(t) for t in h], do, dlse), what)
    want = varlen_backward(q, k, v, _np(got[0]), _np(got[1]).astype(np.float64), _np(do), cu_q, cu_k, dtype=dtype, is_causal=causal,
                           smooth_k=True, q_qmax=qmax, k_qmax=qmax, dlse=_np(dlse).astype(np.float64), return_bound=True)
    for name, g, rf, bnd in zip(("dq", "dk", "dv"), got[2:], want[:3], want[3:]):
        _assert_close(_np(g), rf, dtype, f"{what} {name}")
        _grad_close(_np(g), rf, bnd, f"{what} {name}")


# ---- the caches -----------------------------------------------------------------------------------------------------------
DECODE_LENS = [1, 63, 64, 65, 130]
GARBAGE = dict(k_codes=-128, k_scale=float("inf"), v=float("nan"), k_tail=float("nan"))


def _garbage(cache):
    """codes -128, scales +inf, V and tail NaN everywhere (the mean is an input of the append: written before it is read)"""
    for name, val in GARBAGE.items():
        getattr(cache, name).fill_(val)
    return cache


def _fill_to_lens(cache, k, v, dtype, dev, wrap, **kw):
    """two ragged appends (70 rows, then the rest) that leave the lengths DECODE_LENS"""
    lt = torch.tensor(DECODE_LENS, dtype=torch.int32, device=dev)
    tk, tv = _t(k, dtype, dev), _t(v, dtype, dev)
    cache.append(wrap(tk[:, :, :70]), wrap(tv[:, :, :70]), new_lens=torch.clamp(lt, max=70), **kw)
    cache.append(wrap(tk[:, :, 70:]), wrap(tv[:, :, 70:]), new_lens=torch.clamp(lt - 70, min=0), **kw)
    return cache


def _ref_to_lens(k, v, D, dtype, cap):
    ref = kr.CacheRef(orc, len(DECODE_LENS), HKV, D, cap, dtype)
    ln = np.array(DECODE_LENS)
    ref.append(k[:, :, :70], v[:, :, :70], np.minimum(ln, 70))
    ref.append(k[:, :, 70:], v[:, :, 70:], np.maximum(ln - 70, 0))
    return ref


def _decode_everywhere(lb, dev, cache, twin, ref, D, dtype, what):
    for Sq, causal, layout, q, tq in decode_cases(D, dtype, dev, Bc=len(DECODE_LENS)):
        o_ref, lse_ref, corr, sm = decode_reference(q, ref, ref.seqlens, dtype, causal)
        for ns in (1, 3):
            w = f"{what} Sq={Sq} splits={ns}"
            kw = dict(tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns)
            o, lse = lb.lowbit_fa_decode(hostile(tq), cache, **kw)
            assert torch.isfinite(o).all() and not torch.isnan(lse).any(), w + ": a row behind the end of a sequence was read"
            same_bits((o, lse), lb.lowbit_fa_decode(tq, twin, **kw), w + ": against a clean cache and a contiguous q")
            kr.check_o(_np(o if layout == "HND" else o.transpose(1, 2)), o_ref, dtype, w)
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, w)


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_contiguous_cache_in_hostile_memory(dev, dtype, D):
    import lowbit_quant_fa2_paddle_amd as lb
    n, cap = len(DECODE_LENS), 192
    (k, v), = cache_data(D, dtype, [(130, None)], Bc=n, seed=3)
    twin = _fill_to_lens(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev), k, v, dtype, dev, lambda t: t)
    cache = _fill_to_lens(_garbage(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev)), k, v, dtype, dev, hostile)
    ref = _ref_to_lens(k, v, D, dtype, cap)
    what = f"hostile contiguous cache {dtype} D={D}"
    state_equals_ref(cache, ref, what)
    for b, m in enumerate(DECODE_LENS):  # nothing behind the end of a sequence was written: the garbage is still there
        assert torch.all(cache.k_codes[b, :, m:] == -128) and torch.isnan(cache.v[b, :, m:]).all(), (what, b)
        assert torch.isinf(cache.k_scale[b, :, (m + 63) // 64:]).all(), (what, b)
    _decode_everywhere(lb, dev, cache, twin, ref, D, dtype, what)


@pytest.mark.parametrize("dtype,D,page", [("fp16", 64, 64), ("bf16", 128, 128)])
def test_paged_cache_in_hostile_memory(dev, dtype, D, page):
    import lowbit_quant_fa2_paddle_amd as lb
    n, cap = len(DECODE_LENS), 256
    max_pages = cap // page
    (k, v), = cache_data(D, dtype, [(130, None)], Bc=n, seed=3)
    twin = _fill_to_lens(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev), k, v, dtype, dev, lambda t: t)
    order = np.random.default_rng(page).permutation(n * max_pages + 3).tolist()
    paged = _garbage(lb.LowbitPagedKVCache(n * max_pages + 3, page, HKV, D, n, max_pages, TDT[dtype], dev, page_order=order))
    _fill_to_lens(paged, k, v, dtype, dev, hostile)
    ref = _ref_to_lens(k, v, D, dtype, cap)
    what = f"hostile paged cache {dtype} D={D} page={page}"
    for b, m in enumerate(DECODE_LENS):
        codes, scales, vv = paged.gather(b)
        same_bits(codes[:, :m], twin.k_codes[b, :, :m], f"{what}: codes of {b}")
        same_bits(scales[:, :(m + 63) // 64], twin.k_scale[b, :, :(m + 63) // 64], f"{what}: scales of {b}")
        same_bits(vv[:, :m], twin.v[b, :, :m], f"{what}: v of {b}")
        assert torch.all(codes[:, m:] == -128) and torch.isnan(vv[:, m:]).all(), (what, b)
    spare = torch.tensor(paged.allocator.free_pages, device=dev)
    assert torch.all(paged.k_codes[spare] == -128) and torch.isnan(paged.v[spare]).all() and torch.isinf(paged.k_scale[spare]).all()
    _decode_everywhere(lb, dev, paged, twin, ref, D, dtype, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the device-side defences, exercised inside the test's own memory (THE RULE of the module docstring)
# ---------------------------------------------------------------------------------------------------------------------------
def _whole_state_equals_ref(cache, ref, what):
    """EVERY row of a cache that started as zeros against the numpy cache that started as zeros"""
    assert np.array_equal(cache.k_codes.cpu().numpy(), ref.k_codes), (what, "codes")
    assert np.array_equal(cache.k_scale.cpu().numpy().view(np.uint32), ref.k_scale.view(np.uint32)), (what, "scales")
    assert np.array_equal(_np(cache.v), ref.v), (what, "v")
    assert np.array_equal(_np(cache.k_tail), ref.k_tail), (what, "k_tail")
    assert np.array_equal(_np(cache.km), ref.km), (what, "km")


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_append_at_the_capacity_drops_rows(monkeypatch, dev, dtype, D):
    """capacity 128, device lengths [125, 128, 60] behind the host's back (its bound stays at 60), T = 8: sequence 0 takes rows
    125 .. 127 and drops five, sequence 1 takes none, sequence 2 all eight.

    Reachable without the clipping: sequence b would write rows 128 .. 135 of its [capacity, D] slab, i.e. rows 0 .. 7 of the
    next (batch, head) slab of k_codes / v, and scale 2 of its two, i.e. scale 0 of the next (batch, head).  The farthest is
    (batch 1, last head) -> (batch 2, head 0): inside the tensors, because batch 2 follows - and behind batch 2, which stays in
    range (60 + 8), lies the arena's guard."""
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap, T = 3, 128, 8
    (k0, v0), (k1, v1) = cache_data(D, dtype, [(60, None), (T, None)], Bc=Bc, seed=5)
    arena = GuardArena(monkeypatch, dev)
    cache = arena_backed(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), arena)
    ref = kr.CacheRef(orc, Bc, HKV, D, cap, dtype)
    cache.append(_t(k0, dtype, dev), _t(v0, dtype, dev))
    ref.append(k0, v0)
    what = f"append at the capacity {dtype} D={D}"
    _whole_state_equals_ref(cache, ref, what + " (before)")
    lens_dev = [125, 128, 60]
    cache.seqlens.copy_(torch.tensor(lens_dev, dtype=torch.int32, device=dev))
    ref.seqlens[:] = lens_dev
    assert cache.max_seqlen == 60  # the host's bound: it lets T = 8 through
    before = {name: getattr(cache, name)[1].clone() for name in ("k_codes", "k_scale", "v", "k_tail")}
    v_rows = cache.v[0, :, :125].clone()
    cache.append(_t(k1, dtype, dev), _t(v1, dtype, dev))
    torch.cuda.synchronize()
    arena.check()
    for name, t in before.items():
        same_bits(getattr(cache, name)[1], t, f"{what}: {name} of the full sequence")
    same_bits(cache.v[0, :, :125], v_rows, what + ": V rows of sequence 0 below its length")
    same_bits(cache.v[0, :, 125:], _t(v1, dtype, dev)[0, :, :3].to(torch.float16), what + ": sequence 0 holds rows 125 .. 127")
    same_bits(cache.v[2, :, 60:68], _t(v1, dtype, dev)[2].to(torch.float16), what + ": sequence 2 is appended normally")
    ref.append(k1, v1)
    assert list(ref.seqlens) == [128, 128, 68]
    _whole_state_equals_ref(cache, ref, what)


def test_append_clamps_negative_lengths(monkeypatch, dev):
    """device lengths [-5, 0, 0] and new_lens [-1, 9, 3] at T = 8 are clamped to lengths 0, 0, 0 and 0, 8, 3 new rows.

    Reachable without the clamps: a length of -5 starts the append five rows (5 x 64 bytes of codes, 5 x 128 of V) before slab
    (0, 0), which is the arena's guard in front of k_codes / v; new_lens = 9 > T reads row 8 of k_new / v_new of sequence 1,
    which is row 0 of the next head (or of sequence 2 behind the last head): inside the tensor."""
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap, T, D, dtype = 3, 128, 8, 64, "fp16"
    (k, v), = cache_data(D, dtype, [(T, None)], Bc=Bc, seed=6)
    arena = GuardArena(monkeypatch, dev)
    cache = arena_backed(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev), arena)
    ref = kr.CacheRef(orc, Bc, HKV, D, cap, dtype)
    cache.seqlens.copy_(torch.tensor([-5, 0, 0], dtype=torch.int32, device=dev))
    ref.seqlens[:] = [-5, 0, 0]
    new_lens = [-1, 9, 3]
    with arena:
        cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=torch.tensor(new_lens, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    arena.check()
    ref.append(k, v, new_lens)
    _whole_state_equals_ref(cache, ref, "negative lengths")
    assert not cache.k_codes[0].any() and not cache.v[0].any() and cache.v[1, :, :8].any() and not cache.v[1, :, 8:].any()
    same_bits(cache.v[2, :, :3], _t(v, dtype, dev)[2, :, :3], "sequence 2 takes three rows")


@pytest.mark.parametrize("dtype,D,ns", [("fp16", 64, 1), ("bf16", 128, 3), ("fp16", 128, 0)])
def test_decode_clamps_the_lengths(dev, dtype, D, ns):
    """seqlens = [-3, 0, max_seqlen_k + 70] on the device, the cache's real contents 130 keys per sequence: O and LSE are those of
    [0, 0, max_seqlen_k] - zeros and -inf for the first two.

    Reachable without the clamp: max_seqlen_k = 130 (the host's bound), so 200 keys would be read: rows 130 .. 199 of the same
    [capacity = 320, D] slab and scales 3 of its 5 - inside the cache.  They hold codes -128, scale +inf and NaN, so a kernel
    that reads them returns NaN.  A negative length gives no tile at all."""
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap, n = 3, 320, 130
    (k, v), = cache_data(D, dtype, [(n, None)], Bc=Bc, seed=8)
    cache = _garbage(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev)).append(_t(k, dtype, dev), _t(v, dtype, dev))
    assert cache.max_seqlen == n and n + 70 <= cap
    for Sq, causal, layout, q, tq in decode_cases(D, dtype, dev, Bc=Bc):
        kw = dict(tensor_layout=layout, is_causal=causal, return_lse=True, num_splits=ns)
        cache.seqlens.copy_(torch.tensor([0, 0, n], dtype=torch.int32, device=dev))
        want = lb.lowbit_fa_decode(tq, cache, **kw)
        cache.seqlens.copy_(torch.tensor([-3, 0, n + 70], dtype=torch.int32, device=dev))
        got = lb.lowbit_fa_decode(tq, cache, **kw)
        what = f"decode clamps {dtype} D={D} Sq={Sq} splits={ns}"
        assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
        same_bits(got, want, what)
        ob = got[0] if layout == "HND" else got[0].transpose(1, 2)
        assert not ob[:2].any() and torch.all(torch.isneginf(got[1][:2])), what + ": a sequence without keys gives zeros and -inf"
        assert ob[2].any() and torch.isfinite(got[1][2]).all(), what


PAGED_STATE = ("k_codes", "k_scale", "v", "k_tail", "km", "seqlens", "block_table")


def _paged_in_arena(lb, arena, dev, dtype, D, page, num_pages, num_slots, max_pages):
    """a paged cache whose pool, tails, means, lengths and tables are arena-backed.  The arena's guard (128 KiB) holds more than
    two pages on either side of every pool tensor at these sizes (a V page is HKV x page x D x 2 <= 64 KiB, a codes page half of
    it, a page of scales 8 .. 16 bytes) and more than a slot's worth on either side of the per-slot tensors (a tail slot is
    HKV x 64 x D x 2 <= 32 KiB)."""
    cache = lb.LowbitPagedKVCache(num_pages, page, HKV, D, num_slots, max_pages, TDT[dtype], dev)
    assert 2 * HKV * page * D * 2 <= arena.guard_bytes and HKV * 64 * D * 2 <= arena.guard_bytes
    return arena_backed(cache, arena, names=PAGED_STATE)


def _paged_args(cache, lib, dev, dtype):
    from lowbit_quant_fa2_paddle_amd import _lib
    return dict(dtype=_lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16, km=cache.km.data_ptr(), k_codes=cache.k_codes.data_ptr(),
                k_scale=cache.k_scale.data_ptr(), v_cache=cache.v.data_ptr(), seqlens=cache.seqlens.data_ptr(), Hkv=HKV,
                D=cache.padded_head_dim, num_slots=cache.max_seqs, num_pages=cache.num_pages, page_size=cache.page_size,
                max_pages_per_seq=cache.max_pages_per_seq, stream=torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("dtype,D,page", [("fp16", 64, 64), ("bf16", 128, 128)])
def test_paged_append_skips_corrupt_ids(monkeypatch, dev, dtype, D, page):
    """lbfa_kvcache_paged_append (C ABI) with slots [-1, 1, num_slots] and, in the middle of slot 1's table, the pages -1 and
    num_pages + 1 under the blocks the append touches: rows 0 and 2 are skipped, so are both blocks of row 1 - pool, tails, means
    and guards stay as they were.

    Reachable without the tests: slot -1 / num_slots is one slot before / behind seqlens, k_tail, km and block_table (the arena's
    guard); page -1 is one page before the pool, page num_pages + 1 ends two pages behind it (the guard, see _paged_in_arena)."""
    import lowbit_quant_fa2_paddle_amd as lb
    from cabi_calls import call_gpu
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    num_slots, max_pages, num_pages, T = 3, 4, 14, 3 * page // 2
    arena = GuardArena(monkeypatch, dev)
    cache = _paged_in_arena(lb, arena, dev, dtype, D, page, num_pages, num_slots, max_pages)
    n0 = page + 6  # every slot holds a page and six keys: the open block is block 0 of its second page
    (k0, v0), (k1, v1) = cache_data(D, dtype, [(n0, None), (T, None)], Bc=num_slots, seed=9)
    with arena:
        cache.append(_t(k0, dtype, dev), _t(v0, dtype, dev))
    # the append below covers rows n0 .. n0 + T - 1 of slot 1: table entries 1 and 2 (n0 + T - 1 < 3 * page)
    assert n0 // page == 1 and (n0 + T - 1) // page == 2
    table = cache.block_table.clone()
    table[1, 1], table[1, 2] = -1, num_pages + 1
    bad_table = arena.like(table)
    slots = arena.like(torch.tensor([-1, 1, num_slots], dtype=torch.int32, device=dev))
    state = {name: getattr(cache, name).clone() for name in PAGED_STATE}
    tk, tv = _t(k1, dtype, dev), _t(v1, dtype, dev)
    args = _paged_args(cache, lib, dev, dtype)
    call_gpu(lib, "lbfa_kvcache_paged_append", k_new=tk.data_ptr(), v_new=tv.data_ptr(), new_lens=None, k_tail=cache.k_tail.data_ptr(),
             block_table=bad_table.data_ptr(), slots=slots.data_ptr(), B=num_slots, T=T, sk=tuple(tk.stride()[:3]),
             sv=tuple(tv.stride()[:3]), k_qmax=127, **args)
    torch.cuda.synchronize()
    arena.check()
    for name, t in state.items():
        same_bits(getattr(cache, name), t, f"corrupt ids {dtype} D={D}: {name} changed")
    # the same call with a sound table and slots [0, 1, 2] does append (the case above was not vacuous)
    good = arena.like(torch.tensor([0, 1, 2], dtype=torch.int32, device=dev))
    table = cache.block_table.clone()  # entries 0 and 1 of every slot are sound; a free page each for entry 2
    table[:, 2] = torch.tensor(cache.allocator.free_pages[:num_slots], dtype=torch.int32, device=dev)
    sound = arena.like(table)
    assert len(set(table[:, :3].flatten().tolist())) == 3 * num_slots and int(table.max()) < num_pages
    call_gpu(lib, "lbfa_kvcache_paged_append", k_new=tk.data_ptr(), v_new=tv.data_ptr(), new_lens=None, k_tail=cache.k_tail.data_ptr(),
             block_table=sound.data_ptr(), slots=good.data_ptr(), B=num_slots, T=T, sk=tuple(tk.stride()[:3]),
             sv=tuple(tv.stride()[:3]), k_qmax=127, **args)
    torch.cuda.synchronize()
    arena.check()
    assert not torch.equal(bits(cache.v), bits(state["v"])) and not torch.equal(bits(cache.k_codes), bits(state["k_codes"]))


@pytest.mark.parametrize("dtype,D,page,ns", [("fp16", 64, 64, 1), ("bf16", 128, 128, 3)])
def test_paged_decode_clamps_corrupt_ids(monkeypatch, dev, dtype, D, page, ns):
    """lbfa_decode_paged (C ABI) with slots [-1, 1, num_slots] and the pages -1 and num_pages + 1 in the middle of slot 1's
    table.  attn_decode.hip's PagedKV clamps a slot into [0, num_slots - 1] and a page into [0, num_pages - 1]
    (`min(max(id, 0), n - 1)`): the expected result is the same call with slots [0, 1, num_slots - 1] and the pages 0 and
    num_pages - 1 in those entries, bit for bit, and it is finite - every page of the pool holds finite data here.

    Reachable without the clamps: as in test_paged_append_skips_corrupt_ids - one slot before / behind the per-slot tensors,
    one page before and two behind the pool, all inside the arena's guards, which hold the finite sentinel."""
    import lowbit_quant_fa2_paddle_amd as lb
    from cabi_calls import call_gpu
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    num_slots, max_pages, num_pages, G, Sq = 3, 4, 14, 2, 3
    Hq = G * HKV
    arena = GuardArena(monkeypatch, dev)
    cache = _paged_in_arena(lb, arena, dev, dtype, D, page, num_pages, num_slots, max_pages)
    n = 3 * page + 5  # four table entries per slot, the corrupt ones in the middle
    (k, v), = cache_data(D, dtype, [(n, None)], Bc=num_slots, seed=10)
    with arena:
        cache.append(_t(k, dtype, dev), _t(v, dtype, dev))
    # the pages nobody holds get finite, non-zero keys too: a clamped id reads them
    free = torch.tensor(cache.allocator.free_pages, device=dev)
    cache.k_codes[free] = 3
    cache.k_scale[free] = 0.01
    cache.v[free] = 0.5
    q = upstream((num_slots, Hq, Sq, D), TDT[dtype], dev, 11)

    def run(slot_ids, p1, p2):
        table = cache.block_table.clone()
        table[1, 1], table[1, 2] = p1, p2
        tbl, sl = arena.like(table), arena.like(torch.tensor(slot_ids, dtype=torch.int32, device=dev))
        o, lse = arena.allocate((num_slots, Hq, Sq, D), TDT[dtype]), arena.allocate((num_slots, Hq, Sq), torch.float32)
        nbytes = lib.lbfa_decode_workspace_bytes(num_slots, Hq, HKV, Sq, D, n, ns)
        ws = arena.allocate((max(nbytes, 16),), torch.uint8)
        args = _paged_args(cache, lib, dev, dtype)
        call_gpu(lib, "lbfa_decode_paged", q=q.data_ptr(), block_table=tbl.data_ptr(), slots=sl.data_ptr(), o=o.data_ptr(),
                 lse=lse.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes, B=num_slots, Hq=Hq, Sq=Sq, max_seqlen_k=n, num_splits=ns,
                 sq=tuple(q.stride()[:3]), so=tuple(o.stride()[:3]), sm_scale=D ** -0.5, q_qmax=127, causal=1, **args)
        torch.cuda.synchronize()
        return o, lse

    got = run([-1, 1, num_slots], -1, num_pages + 1)
    want = run([0, 1, num_slots - 1], 0, num_pages - 1)
    arena.check()
    what = f"corrupt ids {dtype} D={D} page={page} splits={ns}"
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), what
    same_bits(got, want, what)
    sound = lb.lowbit_fa_decode(q, cache, is_causal=True, return_lse=True, num_splits=ns)
    same_bits((got[0][[0, 2]], got[1][[0, 2]]), (sound[0][[0, 2]], sound[1][[0, 2]]), what + ": rows 0 and 2 decode slots 0 and 2")
    assert not torch.equal(bits(got[0][1]), bits(sound[0][1])), what + ": the corrupt entries were not used at all"
