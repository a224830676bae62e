"""Seeded fuzz of cached prefill (`lowbit_fa_prefill`) and of the fp8 V cache over head geometries, Q blocks, ragged q_lens, key
lengths, append schedules, slice counts and page layouts (the cases of tests/prefill_fuzz_cases.py;
tests/test_prefill_fuzz_cases_cpu.py shows what they cover and that the numpy model of the kernel meets the same bounds).

Per case the same schedule goes into a `LowbitKVCache`, a `LowbitPagedKVCache` (a pool full of garbage, pages in a scrambled
order, the sequences in permuted slots next to empty ones) and the numpy cache (`CacheRef` / `CacheRefV8`).  With `v_bits = 8`
there is a third cache, `v_bits = 16`, whose `v` is overwritten with V^ computed in numpy from the fp8 cache's codes and scales.
* state: the GPU state equals the numpy cache bit for bit, the paged cache agrees through `gather`;
* values: O and LSE against `oracle_prefill` on the numpy state - so the reference never passes through the code under test -
  within the unchanged `check_o` / `check_lse` on every element, both masks, all three slice counts, at every step at which the
  case calls the operator; rows at or past q_lens and blind rows are exactly 0 and -inf, no NaN anywhere;
* bit for bit: paged == contiguous, a second run, O with and without the LSE, a strided q == its contiguous copy, the fp8 cache ==
  the fp16 cache holding V^, and the call on one sequence's own rows == its rows of the batched call;
* where decode takes the same call (M <= 64, no q_lens) it meets the same oracle output.
"""
import os

import numpy as np
import pytest

import kvcache_reference as kr
import prefill_fuzz_cases as pz
import v8_reference as v8
from test_gpu_decode_fuzz import _bits, _dev, _kv_tensors
from test_gpu_kvcache_decode import TDT, _np, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = int(os.environ.get("LBFA_FUZZ_N", "24"))  # more seeds for a one-off hunt: LBFA_FUZZ_N=400 pytest tests/test_gpu_prefill_fuzz.py -m gpu
SEED0 = int(os.environ.get("LBFA_FUZZ_SEED0", "0"))  # shifts the whole seed range for another hunt
PINNED_NAMES = {c["name"] for c in pz.PINNED}
WORST = {"o": 0.0, "lse": 0.0}  # over the module's run; printed by the last test


def _cases():
    return pz.PINNED + [pz.make_case(SEED0 + s) for s in range(N)]


def _garbage(cache):
    """every page holds what no reader may touch: K codes -128, scales +inf, V NaN; fp8 V the e4m3 NaN code and NaN scales"""
    cache.k_codes.fill_(-128)
    cache.k_scale.fill_(float("inf"))
    if cache.v_bits == 8:
        cache.v.fill_(0xFF)
        cache.v_scale.fill_(float("nan"))
    else:
        cache.v.fill_(float("nan"))
    return cache


def _state_vs_ref(cache, ref, c, what):
    """every valid key of the contiguous cache against the numpy cache: codes, scale bits, V or (v codes, v_scale bits), km, seqlens"""
    assert np.array_equal(cache.seqlens.cpu().numpy(), ref.seqlens), (what, "seqlens")
    codes, scales = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy()
    v = cache.v.cpu().numpy() if c["v_bits"] == 8 else _np(cache.v)
    vs = cache.v_scale.cpu().numpy() if c["v_bits"] == 8 else None
    for b, n in enumerate(int(x) for x in ref.seqlens):
        nb = (n + 63) // 64
        assert np.array_equal(codes[b, :, :n], ref.k_codes[b, :, :n]), (what, b, "codes")
        assert np.array_equal(scales[b, :, :nb].view(np.uint32), ref.k_scale[b, :, :nb].view(np.uint32)), (what, b, "scales")
        if c["v_bits"] == 8:
            assert np.array_equal(v[b, :, :n], ref.v_codes[b, :, :n]), (what, b, "v codes")
            assert np.array_equal(vs[b, :, :n].view(np.uint32), ref.v_scale[b, :, :n].view(np.uint32)), (what, b, "v scales")
        else:
            assert np.array_equal(v[b, :, :n], ref.v[b, :, :n]), (what, b, "v")
    if c["smooth_k"]:
        assert np.array_equal(_np(cache.km), ref.km), (what, "km")
    else:
        assert cache.km is None and ref.km is None


def _paged_vs_dense(paged, dense, c, what):
    """the paged cache through its tables against the contiguous one, bit for bit; the slots no sequence lives in stay empty"""
    slots = torch.tensor(c["slots"], dtype=torch.int64, device=dense.seqlens.device)
    assert torch.equal(paged.seqlens[slots], dense.seqlens), (what, "seqlens")
    assert int(paged.seqlens.sum()) == int(dense.seqlens.sum()), (what, "a slot of no sequence has a length")
    for b, n in enumerate(dense.seqlens.tolist()):
        got = paged.gather(c["slots"][b])
        nb = (n + 63) // 64
        assert got[0].shape[1] >= n, what
        assert torch.equal(got[0][:, :n], dense.k_codes[b, :, :n]), (what, b, "codes")
        assert torch.equal(_bits(got[1][:, :nb]), _bits(dense.k_scale[b, :, :nb])), (what, b, "scales")
        assert torch.equal(_bits(got[2][:, :n]), _bits(dense.v[b, :, :n])), (what, b, "v")
        if c["v_bits"] == 8:
            assert torch.equal(_bits(got[3][:, :n]), _bits(dense.v_scale[b, :, :n])), (what, b, "v scales")
    if c["smooth_k"]:
        assert torch.equal(_bits(paged.km[slots]), _bits(dense.km)), (what, "km")


def _same(a, b, what):
    for name, x, y in zip(("O", "LSE"), a, b):
        if x is not None and y is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, what
            assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs in {int((_bits(x) != _bits(y)).sum())} bytes"


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_fuzz_cache_and_prefill(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    c = case
    B, Hkv, Hq, Sq, D, dtype = c["B"], c["Hkv"], c["G"] * c["Hkv"], c["Sq"], c["D"], c["dtype"]
    fp8 = c["v_bits"] == 8
    q, kv = pz.make_data(oracle, c)
    kw = dict(k_bits=c["k_bits"], smooth_k=c["smooth_k"])
    dense = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, v_bits=c["v_bits"], **kw)
    order = np.random.default_rng(c["page_seed"]).permutation(c["num_pages"]).tolist()
    paged = _garbage(lb.LowbitPagedKVCache(c["num_pages"], c["page"], Hkv, D, c["num_slots"], c["max_pages"], TDT[dtype], dev,
                                           page_order=order, v_bits=c["v_bits"], **kw))
    dense16 = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, **kw) if fp8 else None
    ref = pz.new_ref(oracle, c)
    sm = pz.sm_scale_of(c)

    buf, idx = pz.carry_q(q, c)
    tq = _dev(buf, c, dev)
    if idx is not None:
        tq = tq[idx]
    tq_copy = tq.contiguous()
    layout = c["q_layout"]
    canon = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2))
    q_lens = None if c["q_lens_arg"] is None else torch.tensor(c["q_lens_arg"], dtype=torch.int32, device=dev)

    for step, (a, (k, v)) in enumerate(zip(c["appends"], kv)):
        # ---- the append into all of them; the state after every append of a pinned case and before every call ------------
        tk, tv = _kv_tensors(k, v, a, c, dev)
        tl = None if a["new_lens"] is None else torch.tensor(a["new_lens"], dtype=torch.int32, device=dev)
        dense.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        paged.append(tk, tv, slots=c["slots"], tensor_layout=a["layout"], new_lens=tl)
        if fp8:
            dense16.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        pz.ref_append(oracle, c, ref, step, k, v)
        called = step in c["calls"]
        if called or c["name"] in PINNED_NAMES:
            what = f"{c['name']} after append {step}"
            _state_vs_ref(dense, ref, c, what)
            _paged_vs_dense(paged, dense, c, what)
        if not called:
            continue
        lens = pz.lens_after(c, step)
        assert list(ref.seqlens) == lens
        if fp8:  # V^ in numpy from the fp8 cache's codes and scales, into the public `v` of the fp16 cache
            vhat = v8.dequant_v(oracle, dense.v.cpu().numpy(), dense.v_scale.cpu().numpy())
            assert vhat.dtype == np.float16 and tuple(dense16.v.shape) == vhat.shape
            dense16.v.copy_(torch.from_numpy(vhat).to(dev))

        # ---- prefill against the oracle's kernel on the numpy cache ------------------------------------------------------
        want, corr = pz.prefill_reference(oracle, c, ref, q)
        for causal in (False, True):
            o_ref, lse_ref = want[causal]
            dead = pz.dead_rows(c, lens, causal)
            assert np.array_equal(np.isinf(lse_ref), dead)
            for ns in c["splits"]:
                what = f"{c['name']} step={step} causal={causal} splits={ns}"
                opts = dict(tensor_layout=layout, is_causal=causal, sm_scale=c["sm_scale"], num_splits=ns, q_bits=c["q_bits"])

                def run(cache, tq=tq, lse=c["return_lse"], fn=lb.lowbit_fa_prefill, **more):
                    if fn is lb.lowbit_fa_prefill:
                        more.setdefault("q_lens", q_lens)
                    out = fn(tq, cache, return_lse=lse, **opts, **more)
                    return out if lse else (out, None)

                o, lse = run(dense)
                o_other, lse_other = run(dense, lse=not c["return_lse"])
                assert torch.equal(_bits(o), _bits(o_other)), what + ": O depends on return_lse"
                lse = lse if lse is not None else lse_other
                assert o.shape == tq.shape and o.dtype == tq.dtype and tuple(lse.shape) == (B, Hq, Sq), what
                on, ln = _np(canon(o)), lse.cpu().numpy()
                assert not np.isnan(on).any() and not np.isnan(ln).any(), what + ": NaN"
                WORST["o"] = max(WORST["o"], kr.check_o(on, o_ref, dtype, what))
                WORST["lse"] = max(WORST["lse"], kr.check_lse(ln, lse_ref, corr, sm, dtype, what))
                assert np.all(on[dead] == 0) and np.all(np.isneginf(ln[dead])), what + ": rows past q_lens or without a key"
                # the paged twin, a second run, the contiguous copy of a strided q, the fp16 cache holding V^: the same bits
                got_paged = run(paged, lse=True, slots=c["slots"])
                twins = [("paged cache", got_paged), ("second run", run(dense)), ("contiguous q", run(dense, tq=tq_copy))]
                if fp8:
                    twins.append(("fp16 cache holding V^", run(dense16, lse=True)))
                for label, got in twins:
                    _same(got, (o, lse), f"{what}: the {label}")
                # the sub-batch property: sequence b alone, on its own rows, through its slot
                if ns:
                    for b, ql in enumerate(c["q_lens"]):
                        if ql == 0:
                            continue
                        rows = (slice(b, b + 1), slice(None), slice(0, ql)) if layout == "HND" else (slice(b, b + 1), slice(0, ql))
                        alone = run(paged, tq=tq[rows], lse=True, slots=[c["slots"][b]], q_lens=None)
                        _same(alone, (got_paged[0][rows], got_paged[1][b:b + 1, :, :ql]), f"{what}: sequence {b} alone")
                # decode takes the same call: the same oracle output
                if pz.decode_takes_it(c):
                    od, ld = run(dense, lse=True, fn=lb.lowbit_fa_decode)
                    kr.check_o(_np(canon(od)), o_ref, dtype, what + " decode")
                    kr.check_lse(ld.cpu().numpy(), lse_ref, corr, sm, dtype, what + " decode")
    assert list(ref.seqlens) == c["lens"]


def test_worst_ratios_of_this_run():
    """prints the worst O and LSE ratios the cases above reached (read it with -s; DESIGN.md 3.12 records the default range)"""
    print(f"prefill fuzz, {len(_cases())} cases: worst O at {WORST['o']:.3f} of o_bound, worst LSE at {WORST['lse']:.3f} of lse_bound")
    assert WORST["o"] <= 1.0 and WORST["lse"] <= 1.0
