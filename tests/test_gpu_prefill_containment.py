"""Cached prefill (`lowbit_fa_prefill`, lbfa_prefill / lbfa_prefill_paged) under the guard bands and hostile memory of
tests/guarded.py, in the manner of tests/test_gpu_containment.py and tests/test_gpu_hostile_memory.py:

* the call inside a `GuardArena`: the same bits as outside, no guard byte touched, the workspace exactly
  `lbfa_prefill_workspace_bytes`;
* a strided output of 80 channels in 128-channel rows through the C ABI (`guarded_out`);
* every operand as a `hostile_view`, a cache full of NaN / -128 / +inf beyond each length and in pages no table names: bit-equal
  to the clean run, no NaN; lengths 1, 63, 64, 65 and 130;
* the device-side defences: `seqlens` outside [0, max_seqlen_k], `q_lens` outside [0, Sq], slot and page ids out of range.

THE RULE of those files holds here: every defence case is chosen so that an UNDEFENDED kernel would still stay inside memory the
test owns (the docstrings say what it would reach).  Nothing here can fault.
"""
import numpy as np
import pytest

import kvcache_reference as kr
import prefill_reference as pr
from guarded import GuardArena, guarded_out
from oracle import lowbit_fa_oracle as orc
from test_gpu_containment import HKV, cache_data, exact_workspace, same_bits, twice, upstream
from test_gpu_hostile_memory import (DECODE_LENS, _fill_to_lens, _garbage, _paged_args, _paged_in_arena, _ref_to_lens, hostile)
from test_gpu_parity import TDT, _np, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 2
HQ = G * HKV
SQ = pr.CONTAINMENT_SQ  # 130: two Q blocks, the second with two rows


def _reference(q, ref, q_lens, dtype, causal):
    """`oracle_prefill` on the numpy cache: q [B, Hq, Sq, D] canonical -> o, lse, corr, sm_scale"""
    sm = q.shape[-1] ** -0.5
    q_i8, q_scale = pr.quant_q_blocks(orc, q, q_lens, sm, 127)
    corr = kr.lse_correction(orc, q, ref.km, dtype)
    o, lse2 = pr.oracle_prefill(orc, q_i8, q_scale, ref, q_lens, causal=causal, out_dtype=dtype)
    return o, kr.natural_lse(lse2, corr, sm), corr, sm


def _queries(D, dtype, dev, n):
    q = orc.to_storage(np.random.default_rng(D).standard_normal((n, HQ, SQ, D), dtype=np.float32), dtype)
    return q, _t(q, dtype, dev)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. hostile memory around every operand and behind every length, both layouts of the cache; the guarded call
# ---------------------------------------------------------------------------------------------------------------------------
def _prefill_everywhere(monkeypatch, lb, dev, cache, twin, ref, D, dtype, what):
    n = len(DECODE_LENS)
    q, tq = _queries(D, dtype, dev, n)
    q_lens = pr.CONTAINMENT_Q_LENS
    assert DECODE_LENS == pr.CONTAINMENT_LENS  # tests/test_prefill_reference_cpu.py holds the numpy model to the bounds here too
    tl = torch.tensor(q_lens, dtype=torch.int32, device=dev)
    for causal in (False, True):
        o_ref, lse_ref, corr, sm = _reference(q, ref, q_lens, dtype, causal)
        for ns in (1, 3):
            w = f"{what} causal={causal} splits={ns}"
            kw = dict(is_causal=causal, return_lse=True, num_splits=ns, q_lens=tl)
            o, lse = twice(monkeypatch, dev, lambda: lb.lowbit_fa_prefill(hostile(tq), cache, **kw), w, min_allocations=3)
            assert torch.isfinite(o).all() and not torch.isnan(lse).any(), w + ": a row behind the end of a sequence was read"
            same_bits((o, lse), lb.lowbit_fa_prefill(tq, twin, **kw), w + ": against a clean cache and a contiguous q")
            kr.check_o(_np(o), o_ref, dtype, w)
            kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, w)


@pytest.mark.parametrize("dtype,D", [("fp16", 64), ("bf16", 128)])
def test_contiguous_cache_in_hostile_memory(monkeypatch, dev, dtype, D):
    import lowbit_quant_fa2_paddle_amd as lb
    n, cap = len(DECODE_LENS), 192
    (k, v), = cache_data(D, dtype, [(130, None)], Bc=n, seed=3)
    twin = _fill_to_lens(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev), k, v, dtype, dev, lambda t: t)
    cache = _fill_to_lens(_garbage(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev)), k, v, dtype, dev, hostile)
    ref = _ref_to_lens(k, v, D, dtype, cap)
    _prefill_everywhere(monkeypatch, lb, dev, cache, twin, ref, D, dtype, f"hostile contiguous cache {dtype} D={D}")


@pytest.mark.parametrize("dtype,D,page", [("fp16", 64, 64), ("bf16", 128, 128)])
def test_paged_cache_in_hostile_memory(monkeypatch, dev, dtype, D, page):
    import lowbit_quant_fa2_paddle_amd as lb
    n, cap = len(DECODE_LENS), 256
    max_pages = cap // page
    (k, v), = cache_data(D, dtype, [(130, None)], Bc=n, seed=3)
    twin = _fill_to_lens(lb.LowbitKVCache(n, HKV, D, cap, TDT[dtype], dev), k, v, dtype, dev, lambda t: t)
    order = np.random.default_rng(page).permutation(n * max_pages + 3).tolist()
    paged = _garbage(lb.LowbitPagedKVCache(n * max_pages + 3, page, HKV, D, n, max_pages, TDT[dtype], dev, page_order=order))
    _fill_to_lens(paged, k, v, dtype, dev, hostile)
    ref = _ref_to_lens(k, v, D, dtype, cap)
    _prefill_everywhere(monkeypatch, lb, dev, paged, twin, ref, D, dtype, f"hostile paged cache {dtype} D={D} page={page}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a strided output through the C ABI, an exact workspace
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,causal,ns", [("fp16", False, 1), ("bf16", True, 3), ("fp16", True, 0)])
def test_strided_output_of_80_channels_by_ctypes(monkeypatch, dev, dtype, causal, ns):
    """lbfa_prefill of an 80-channel head dim into 128-channel rows with doubled token and head strides.  The C ABI knows D = 128
    only (the caller pads q, the cache pads K and V), so a row of the output is 128 channels of which the last 48 come out as
    zeros (the padded V); the gaps between rows and heads must stay untouched.  With three slices the partials live in a workspace
    of exactly lbfa_prefill_workspace_bytes."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    Bc, cap, D, Dp = 3, 320, 80, 128
    schedule = [(63, None), (2, None), (200, [200, 7, 131])]
    data = cache_data(D, dtype, schedule)
    cache = lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev)
    for (T, nl), (k, v) in zip(schedule, data):
        cache.append(_t(k, dtype, dev), _t(v, dtype, dev), new_lens=None if nl is None else torch.tensor(nl, dtype=torch.int32, device=dev))
    q = upstream((Bc, HQ, SQ, D), TDT[dtype], dev, 9)
    q_lens = torch.tensor([SQ, 5, 129], dtype=torch.int32, device=dev)
    o_want, lse_want = lb.lowbit_fa_prefill(q, cache, is_causal=causal, return_lse=True, num_splits=ns, q_lens=q_lens)
    qp = torch.nn.functional.pad(q, (0, Dp - D))
    so = (HQ * 2 * SQ * 2 * Dp, 2 * SQ * 2 * Dp, 2 * Dp)
    o, check = guarded_out((Bc, HQ, SQ, Dp), TDT[dtype], so + (1,), dev)
    arena = GuardArena(monkeypatch, dev)
    lse = arena.allocate((Bc, HQ, SQ), torch.float32)
    max_k = min(cache.max_seqlen, cache.capacity)
    nbytes = lib.lbfa_prefill_workspace_bytes(Bc, HQ, HKV, SQ, Dp, max_k, ns)
    eff = ns or lib.lbfa_prefill_num_splits(Bc, HQ, SQ, max_k)
    assert (nbytes > 0) == (eff > 1)
    ws = exact_workspace(arena, nbytes)
    st = lib.lbfa_prefill(qp.data_ptr(), _lib.LBFA_F16 if dtype == "fp16" else _lib.LBFA_BF16, cache.k_codes.data_ptr(),
                          cache.k_scale.data_ptr(), cache.v.data_ptr(), cache.km.data_ptr(), cache.seqlens.data_ptr(), q_lens.data_ptr(),
                          o.data_ptr(), lse.data_ptr(), ws.data_ptr() if ws is not None else None, nbytes, Bc, HQ, HKV, SQ, Dp, cap,
                          max_k, ns, _lib.strides3(qp.stride()[:3]), _lib.strides3(so), D ** -0.5, 127, int(causal),
                          torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, lib)
    torch.cuda.synchronize()
    what = f"lbfa_prefill {dtype} causal={causal} splits={ns}"
    check(what)
    arena.check()
    same_bits(o[..., :D], o_want, what + ": O")
    assert not o[..., D:].any(), what + ": the padded channels are zeros"
    same_bits(lse, lse_want, what + ": LSE")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the device-side defences
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,ns", [("fp16", 64, 1), ("bf16", 128, 3), ("fp16", 128, 0)])
def test_prefill_clamps_the_lengths(dev, dtype, D, ns):
    """seqlens = [-3, 0, max_seqlen_k + 70] and q_lens = [Sq + 70, -3, Sq + 70] on the device, the cache's real contents 130 keys per
    sequence: O and the LSE are those of seqlens [0, 0, max_seqlen_k] and q_lens [Sq, 0, Sq].

    Reachable without the clamps.  Keys: max_seqlen_k = 130, so 200 keys would be read - rows 130 .. 199 of the same [capacity =
    320, D] slab and scale 3 of its 5, inside the cache; they hold codes -128, scale +inf and NaN, so a kernel that reads them
    returns NaN.  A negative length gives no tile.  Queries: 70 rows behind row Sq - 1 of a (batch, head) of q, which is a view
    inside a larger NaN buffer with a whole head and a whole batch entry (Sq + 2 >= 72 rows each) behind the last one; they
    would enter the block's amax as NaN.  o, lse and the partials are indexed by rows < Sq whatever q_lens says."""
    import lowbit_quant_fa2_paddle_amd as lb
    Bc, cap, n = 3, 320, 130
    (k, v), = cache_data(D, dtype, [(n, None)], Bc=Bc, seed=8)
    cache = _garbage(lb.LowbitKVCache(Bc, HKV, D, cap, TDT[dtype], dev)).append(_t(k, dtype, dev), _t(v, dtype, dev))
    assert cache.max_seqlen == n and n + 70 <= cap and SQ + 2 >= 72
    _, tq = _queries(D, dtype, dev, Bc)
    tq = hostile(tq)
    for causal in (False, True):
        kw = dict(is_causal=causal, return_lse=True, num_splits=ns)
        cache.seqlens.copy_(torch.tensor([0, 0, n], dtype=torch.int32, device=dev))
        want = lb.lowbit_fa_prefill(tq, cache, q_lens=torch.tensor([SQ, 0, SQ], dtype=torch.int32), **kw)
        cache.seqlens.copy_(torch.tensor([-3, 0, n + 70], dtype=torch.int32, device=dev))
        got = lb.lowbit_fa_prefill(tq, cache, q_lens=torch.tensor([SQ + 70, -3, SQ + 70], dtype=torch.int32), **kw)
        what = f"prefill clamps {dtype} D={D} causal={causal} splits={ns}"
        assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
        same_bits(got, want, what)
        assert not got[0][:2].any() and torch.all(torch.isneginf(got[1][:2])), what + ": no keys / no queries give zeros and -inf"
        assert got[0][2].any() and torch.isfinite(got[1][2]).all(), what


@pytest.mark.parametrize("dtype,D,page,ns", [("fp16", 64, 64, 1), ("bf16", 128, 128, 3)])
def test_paged_prefill_clamps_corrupt_ids(monkeypatch, dev, dtype, D, page, ns):
    """lbfa_prefill_paged (C ABI) with slots [-1, 1, num_slots] and the pages -1 and num_pages + 1 in the middle of slot 1's table:
    the result is that of slots [0, 1, num_slots - 1] and the pages 0 and num_pages - 1 in those entries, bit for bit, and finite -
    every page of the pool holds finite data here.

    Reachable without the clamps: as in tests/test_gpu_hostile_memory.py::test_paged_decode_clamps_corrupt_ids - one slot before /
    behind the per-slot tensors, one page before and two behind the pool, all inside the arena's guards (`_paged_in_arena` asserts
    the sizes), which hold the finite sentinel."""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    lib = _lib.load()
    num_slots, max_pages, num_pages = 3, 4, 14
    arena = GuardArena(monkeypatch, dev)
    cache = _paged_in_arena(lb, arena, dev, dtype, D, page, num_pages, num_slots, max_pages)
    n = 3 * page + 5  # four table entries per slot, the corrupt ones in the middle
    (k, v), = cache_data(D, dtype, [(n, None)], Bc=num_slots, seed=10)
    with arena:
        cache.append(_t(k, dtype, dev), _t(v, dtype, dev))
    free = torch.tensor(cache.allocator.free_pages, device=dev)  # the pages nobody holds get finite keys too: a clamped id reads them
    cache.k_codes[free] = 3
    cache.k_scale[free] = 0.01
    cache.v[free] = 0.5
    q = upstream((num_slots, HQ, SQ, D), TDT[dtype], dev, 11)

    def run(slot_ids, p1, p2):
        table = cache.block_table.clone()
        table[1, 1], table[1, 2] = p1, p2
        tbl, sl = arena.like(table), arena.like(torch.tensor(slot_ids, dtype=torch.int32, device=dev))
        o, lse = arena.allocate((num_slots, HQ, SQ, D), TDT[dtype]), arena.allocate((num_slots, HQ, SQ), torch.float32)
        nbytes = lib.lbfa_prefill_workspace_bytes(num_slots, HQ, HKV, SQ, D, n, ns)
        ws = arena.allocate((max(nbytes, 16),), torch.uint8)
        a = _paged_args(cache, lib, dev, dtype)
        st = lib.lbfa_prefill_paged(q.data_ptr(), a["dtype"], a["k_codes"], a["k_scale"], a["v_cache"], a["km"], a["seqlens"], None,
                                    tbl.data_ptr(), sl.data_ptr(), o.data_ptr(), lse.data_ptr(), ws.data_ptr(), nbytes, num_slots, HQ,
                                    HKV, SQ, D, a["num_slots"], a["num_pages"], a["page_size"], a["max_pages_per_seq"], n, ns,
                                    _lib.strides3(q.stride()[:3]), _lib.strides3(o.stride()[:3]), D ** -0.5, 127, 1, a["stream"])
        _lib.check(st, lib)
        torch.cuda.synchronize()
        return o, lse

    got = run([-1, 1, num_slots], -1, num_pages + 1)
    want = run([0, 1, num_slots - 1], 0, num_pages - 1)
    arena.check()
    what = f"corrupt ids {dtype} D={D} page={page} splits={ns}"
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), what
    same_bits(got, want, what)
    sound = lb.lowbit_fa_prefill(q, cache, is_causal=True, return_lse=True, num_splits=ns)
    same_bits((got[0][[0, 2]], got[1][[0, 2]]), (sound[0][[0, 2]], sound[1][[0, 2]]), what + ": rows 0 and 2 read slots 0 and 2")
    assert not torch.equal(got[0][1], sound[0][1]), what + ": the corrupt entries were not used at all"
