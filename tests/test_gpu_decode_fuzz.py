"""Seeded fuzz of the int8 KV cache, its paged twin and split-KV decode over row geometries, append schedules and slice counts
(the cases of tests/decode_fuzz_cases.py; tests/test_decode_fuzz_cases_cpu.py shows what they cover).

Per case the same schedule goes into a `LowbitKVCache`, a `LowbitPagedKVCache` (a pool full of garbage, pages in a scrambled
order) and the numpy `CacheRef`.  The GPU state is compared with `CacheRef` bit for bit, and the decode with the oracle's kernel
on `CacheRef`'s state - so the reference never passes through the code under test.  Bounds: `kvcache_reference.o_bound` /
`lse_bound`, on every element.

Every case has an fp8 twin: the same schedule into a `v_bits = 8` contiguous and paged cache.  Their state equals `CacheRefV8` bit
for bit, their decode equals - bit for bit - that of the fp16 cache once its `v` holds V^ (computed in numpy from the fp8 cache's
codes and scales), and lies inside the same bounds of the oracle on V^.
"""
import os

import numpy as np
import pytest

import decode_fuzz_cases as fz
import kvcache_reference as kr
import v8_reference as v8
from test_gpu_kvcache_decode import TDT, _np, dev  # noqa: F401
from test_gpu_paged_kvcache import _paged

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = int(os.environ.get("LBFA_FUZZ_N", "32"))  # more seeds for a one-off hunt: LBFA_FUZZ_N=400 pytest tests/test_gpu_decode_fuzz.py -m gpu
SEED0 = int(os.environ.get("LBFA_FUZZ_SEED0", "0"))  # shifts the whole seed range for another hunt
PINNED_NAMES = {c["name"] for c in fz.PINNED}


def _dev(a, c, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(TDT[c["dtype"]]).to(dev)


def _kv_tensors(k, v, a, c, dev):
    """k and v of one append on the device, as the case carries them: two tensors, or two views of one packed buffer"""
    x, y, idx_v = fz.carry_kv(k, v, a)
    if idx_v is None:
        return _dev(x, c, dev), _dev(y, c, dev)
    buf = _dev(x, c, dev)
    return buf[y], buf[idx_v]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _state_vs_ref(cache, ref, c, what):
    """every valid key of the contiguous cache against the numpy cache: codes, scale bits, V, km, seqlens"""
    lens = cache.seqlens.cpu().numpy()
    assert np.array_equal(lens, ref.seqlens), (what, "seqlens")
    codes, scales, v = cache.k_codes.cpu().numpy(), cache.k_scale.cpu().numpy(), _np(cache.v)
    for b, n in enumerate(int(x) for x in ref.seqlens):
        nb = (n + 63) // 64
        assert np.array_equal(codes[b, :, :n], ref.k_codes[b, :, :n]), (what, b, "codes")
        assert np.array_equal(scales[b, :, :nb].view(np.uint32), ref.k_scale[b, :, :nb].view(np.uint32)), (what, b, "scales")
        assert np.array_equal(v[b, :, :n], ref.v[b, :, :n]), (what, b, "v")
    if c["smooth_k"]:
        assert np.array_equal(_np(cache.km), ref.km), (what, "km")
    else:
        assert cache.km is None and ref.km is None


def _paged_vs_dense(paged, dense, c, what):
    """the paged cache through its tables against the contiguous one, bit for bit"""
    assert torch.equal(paged.seqlens, dense.seqlens), (what, "seqlens")
    for b, n in enumerate(dense.seqlens.tolist()):
        codes, scales, v = paged.gather(b)
        nb = (n + 63) // 64
        assert codes.shape[1] >= n, what
        assert torch.equal(codes[:, :n], dense.k_codes[b, :, :n]), (what, b, "codes")
        assert torch.equal(_bits(scales[:, :nb]), _bits(dense.k_scale[b, :, :nb])), (what, b, "scales")
        assert torch.equal(_bits(v[:, :n]), _bits(dense.v[b, :, :n])), (what, b, "v")
    if c["smooth_k"]:
        assert torch.equal(_bits(paged.km), _bits(dense.km)), (what, "km")


def _paged_v8(lb, c, dev, order, **kw):
    """the fp8 twin of the paged cache: every page holds the e4m3 NaN code and NaN scales next to the K garbage"""
    cache = lb.LowbitPagedKVCache(c["num_pages"], c["page"], c["Hkv"], c["D"], c["B"], c["max_pages"], TDT[c["dtype"]], dev,
                                  page_order=order, v_bits=8, **kw)
    cache.k_codes.fill_(127), cache.k_scale.fill_(float("inf")), cache.v.fill_(0xFF), cache.v_scale.fill_(float("nan"))
    return cache


def _v8_state_vs_ref(dense8, paged8, dense, ref8, what):
    """the fp8 twins: v codes and v_scale bits of every valid key are `CacheRefV8`'s, the K state is the fp16-V cache's, and the
    paged twin agrees through `gather`"""
    codes, scales = dense8.v.cpu().numpy(), dense8.v_scale.cpu().numpy()
    assert np.array_equal(dense8.seqlens.cpu().numpy(), ref8.seqlens) and torch.equal(paged8.seqlens, dense8.seqlens), (what, "seqlens")
    for name in ("k_codes", "k_scale", "k_tail", "seqlens") + (("km",) if dense.km is not None else ()):
        assert torch.equal(_bits(getattr(dense8, name)), _bits(getattr(dense, name))), (what, name, "K state of the fp8 twin")
    for b, n in enumerate(int(x) for x in ref8.seqlens):
        nb = (n + 63) // 64
        assert np.array_equal(codes[b, :, :n], ref8.v_codes[b, :, :n]), (what, b, "v codes")
        assert np.array_equal(scales[b, :, :n].view(np.uint32), ref8.v_scale[b, :, :n].view(np.uint32)), (what, b, "v scales")
        kc, ks, vc, vs = paged8.gather(b)
        assert torch.equal(kc[:, :n], dense8.k_codes[b, :, :n]) and torch.equal(_bits(ks[:, :nb]), _bits(dense8.k_scale[b, :, :nb])), (what, b)
        assert torch.equal(vc[:, :n], dense8.v[b, :, :n]) and torch.equal(_bits(vs[:, :n]), _bits(dense8.v_scale[b, :, :n])), (what, b)
    if dense.km is not None:
        assert torch.equal(_bits(paged8.km), _bits(dense8.km)), (what, "km")


def _cases():
    return fz.PINNED + [fz.make_case(SEED0 + s) for s in range(N)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_fuzz_cache_and_decode(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    c = case
    B, Hkv, Hq, Sq, D, dtype = c["B"], c["Hkv"], c["G"] * c["Hkv"], c["Sq"], c["D"], c["dtype"]
    q, kv = fz.make_data(oracle, c)
    kw = dict(k_bits=c["k_bits"], smooth_k=c["smooth_k"])
    dense = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, **kw)
    order = np.random.default_rng(c["page_seed"]).permutation(c["num_pages"]).tolist()
    paged = _paged(dev, num_pages=c["num_pages"], page=c["page"], Hkv=Hkv, D=D, max_seqs=B, max_pages=c["max_pages"], dtype=dtype,
                   order=order, **kw)
    copies = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, **kw) if any(a["packed"] for a in c["appends"]) else None
    ref = fz.new_ref(oracle, c)
    dense8 = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, v_bits=8, **kw)
    paged8 = _paged_v8(lb, c, dev, order, **kw)
    ref8 = fz.new_ref_v8(oracle, c)

    # ---- the schedule into all of them; the state after the last append (after every append for the pinned cases) -------
    last = len(c["appends"]) - 1
    for step, (a, (k, v)) in enumerate(zip(c["appends"], kv)):
        tk, tv = _kv_tensors(k, v, a, c, dev)
        tl = None if a["new_lens"] is None else torch.tensor(a["new_lens"], dtype=torch.int32, device=dev)
        dense.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        paged.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        if copies is not None:
            copies.append(tk.contiguous(), tv.contiguous(), tensor_layout=a["layout"], new_lens=tl)
        fz.ref_append(oracle, c, ref, step, k, v)
        dense8.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        paged8.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        fz.ref_append(oracle, c, ref8, step, k, v)
        if step == last or c["name"] in PINNED_NAMES:
            what = f"{c['name']} after append {step}"
            _state_vs_ref(dense, ref, c, what)
            _paged_vs_dense(paged, dense, c, what)
            _v8_state_vs_ref(dense8, paged8, dense, ref8, what)
            if copies is not None:  # whole tensors: a packed view leaves the bits of its contiguous copy everywhere
                for name in ("k_codes", "k_scale", "v", "k_tail", "seqlens") + (("km",) if c["smooth_k"] else ()):
                    assert torch.equal(_bits(getattr(dense, name)), _bits(getattr(copies, name))), (what, name, "packed view")
    assert list(ref.seqlens) == c["lens"]

    # ---- decode against the oracle's kernel on the numpy cache -----------------------------------------------------------
    o_ref, lse_ref, corr = fz.decode_reference(oracle, c, ref, q)
    sm = fz.sm_scale_of(c)
    dead = fz.blind_rows(c)
    assert np.array_equal(np.isinf(lse_ref), dead)
    buf, idx = fz.carry_q(q, c)
    tq = _dev(buf, c, dev)
    if idx is not None:
        tq = tq[idx]
    tq_copy = tq.contiguous()
    layout = c["q_layout"]
    canon = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2))
    for ns in c["splits"]:
        what = f"{c['name']} splits={ns}"
        opts = dict(tensor_layout=layout, is_causal=c["is_causal"], sm_scale=c["sm_scale"], num_splits=ns, q_bits=c["q_bits"])

        def run(cache, tq=tq, lse=c["return_lse"]):
            out = lb.lowbit_fa_decode(tq, cache, return_lse=lse, **opts)
            return out if lse else (out, None)

        o, lse = run(dense)
        o_other, lse_other = run(dense, lse=not c["return_lse"])
        assert torch.equal(_bits(o), _bits(o_other)), what + ": O depends on return_lse"
        lse = lse if lse is not None else lse_other
        assert o.shape == tq.shape and o.dtype == tq.dtype and tuple(lse.shape) == (B, Hq, Sq), what
        on = _np(canon(o))
        assert not np.isnan(on).any(), what + ": NaN in O"
        kr.check_o(on, o_ref, dtype, what)
        kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, what)
        assert np.all(on[dead] == 0) and np.all(np.isneginf(lse.cpu().numpy()[dead])), what + ": rows that see no key"
        # the paged twin, a second run, the contiguous copy of a strided q: the same bits
        twins = (("paged cache", run(paged, lse=True)), ("second run", run(dense)), ("contiguous q", run(dense, tq=tq_copy)))
        for label, (o2, lse2) in twins:
            assert torch.equal(_bits(o2), _bits(o)), f"{what}: O of the {label} differs"
            if lse2 is not None:
                assert torch.equal(_bits(lse2), _bits(lse)), f"{what}: LSE of the {label} differs"

    # ---- the fp8 twin: V^ in numpy from its codes and scales into the public `v` of the fp16 cache (whose own reads are done) ---
    vhat = v8.dequant_v(oracle, dense8.v.cpu().numpy(), dense8.v_scale.cpu().numpy())
    assert vhat.dtype == np.float16 and dense.v.dtype == torch.float16 and tuple(dense.v.shape) == vhat.shape
    dense.v.copy_(torch.from_numpy(vhat).to(dev))
    o_ref, lse_ref, corr = fz.decode_reference(oracle, c, ref8, q, v=ref8.vhat())
    for ns in c["splits"]:
        what = f"{c['name']} fp8 V splits={ns}"
        opts = dict(tensor_layout=layout, is_causal=c["is_causal"], sm_scale=c["sm_scale"], num_splits=ns, q_bits=c["q_bits"],
                    return_lse=True)
        o, lse = lb.lowbit_fa_decode(tq, dense8, **opts)
        for label, cache in (("fp16 cache holding V^", dense), ("paged fp8 cache", paged8)):
            o2, lse2 = lb.lowbit_fa_decode(tq, cache, **opts)
            assert torch.equal(_bits(o2), _bits(o)), f"{what}: O of the {label} differs"
            assert torch.equal(_bits(lse2), _bits(lse)), f"{what}: LSE of the {label} differs"
        on = _np(canon(o))
        assert not np.isnan(on).any(), what + ": NaN in O"
        kr.check_o(on, o_ref, dtype, what)
        kr.check_lse(lse.cpu().numpy(), lse_ref, corr, sm, dtype, what)
        assert np.all(on[dead] == 0) and np.all(np.isneginf(lse.cpu().numpy()[dead])), what + ": rows that see no key"
