"""A nibble-packed twin of every case of tests/decode_fuzz_cases.py and tests/prefill_fuzz_cases.py with `k_bits` forced to 4: the
same append schedule goes into a byte-per-code `k_bits=4` cache, a packed contiguous cache and a packed paged cache (a pool full
of garbage, pages in a scrambled order), and everything is compared bit for bit - the state after every append (after the last for
the seeded decode cases), O and LSE of every call the case makes.  The byte cache is checked against the numpy model and the oracle
in tests/test_gpu_decode_fuzz.py and tests/test_gpu_prefill_fuzz.py; no case is skipped here.  The V format alternates over the
decode cases and is the case's own for the prefill cases.
"""
import os

import numpy as np
import pytest

import decode_fuzz_cases as fz
import k4_reference as k4
import prefill_fuzz_cases as pz
from test_gpu_decode_fuzz import _bits, _dev, _kv_tensors
from test_gpu_kvcache_decode import TDT, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_DECODE = int(os.environ.get("LBFA_FUZZ_N", "32"))
N_PREFILL = int(os.environ.get("LBFA_FUZZ_N", "24"))
SEED0 = int(os.environ.get("LBFA_FUZZ_SEED0", "0"))


def _decode_cases():
    return [dict(c, k_bits=4) for c in fz.PINNED + [fz.make_case(SEED0 + s) for s in range(N_DECODE)]]


def _prefill_cases():
    return [dict(c, k_bits=4) for c in pz.PINNED + [pz.make_case(SEED0 + s) for s in range(N_PREFILL)]]


def _garbage(cache):
    """every page holds what no reader may touch: the code pair no quantiser writes, scales +inf, V NaN"""
    cache.k_codes.fill_(0x88), cache.k_scale.fill_(float("inf"))
    if cache.v_bits == 8:
        cache.v.fill_(0xFF), cache.v_scale.fill_(float("nan"))
    else:
        cache.v.fill_(float("nan"))
    return cache


def _caches(lb, c, dev, v_bits, num_slots):
    B, Hkv, D, dtype = c["B"], c["Hkv"], c["D"], c["dtype"]
    kw = dict(k_bits=4, smooth_k=c["smooth_k"], v_bits=v_bits)
    byte = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, **kw)
    dense = lb.LowbitKVCache(B, Hkv, D, c["capacity"], TDT[dtype], dev, k_packed=True, **kw)
    order = np.random.default_rng(c["page_seed"]).permutation(c["num_pages"]).tolist()
    paged = _garbage(lb.LowbitPagedKVCache(c["num_pages"], c["page"], Hkv, D, num_slots, c["max_pages"], TDT[dtype], dev,
                                           page_order=order, k_packed=True, **kw))
    assert byte.k_qmax == dense.k_qmax == paged.k_qmax == 7
    return byte, dense, paged


def _state(byte, dense, paged, slots, c, what):
    """the packed contiguous cache against the byte cache, whole tensors (both began as zeros); the paged one through its tables"""
    assert torch.equal(dense.unpacked_k_codes(), byte.k_codes), (what, "codes")
    assert np.array_equal(dense.k_codes.cpu().numpy(), k4.pack(byte.k_codes.cpu().numpy())), (what, "packed bytes")
    names = ("k_scale", "k_tail", "v", "seqlens") + (("km",) if c["smooth_k"] else ()) + (("v_scale",) if byte.v_bits == 8 else ())
    for name in names:
        assert torch.equal(_bits(getattr(dense, name)), _bits(getattr(byte, name))), (what, name)
    idx = torch.tensor(slots, dtype=torch.int64, device=dense.seqlens.device)
    assert torch.equal(paged.seqlens[idx], dense.seqlens), (what, "paged seqlens")
    for b, n in enumerate(dense.seqlens.tolist()):
        got = paged.gather(slots[b])
        nb = (n + 63) // 64
        assert torch.equal(got[0][:, :n], dense.k_codes[b, :, :n]), (what, b, "paged codes")
        assert torch.equal(_bits(got[1][:, :nb]), _bits(dense.k_scale[b, :, :nb])), (what, b, "paged scales")
        assert torch.equal(_bits(got[2][:, :n]), _bits(dense.v[b, :, :n])), (what, b, "paged v")
        if byte.v_bits == 8:
            assert torch.equal(_bits(got[3][:, :n]), _bits(dense.v_scale[b, :, :n])), (what, b, "paged v scales")
    if c["smooth_k"]:
        assert torch.equal(_bits(paged.km[idx]), _bits(dense.km)), (what, "paged km")


def _same(a, b, what):
    for name, x, y in zip(("O", "LSE"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs"
        assert not torch.isnan(x).any(), f"{what}: NaN in {name}"


def _query(mod, q, c, dev):
    buf, idx = mod.carry_q(q, c)
    tq = _dev(buf, c, dev)
    return tq if idx is None else tq[idx]


@pytest.mark.parametrize("case", list(enumerate(_decode_cases())), ids=lambda ic: ic[1]["name"])
def test_packed_twin_of_the_decode_fuzz(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    i, c = case
    q, kv = fz.make_data(oracle, c)
    slots = list(range(c["B"]))
    byte, dense, paged = _caches(lb, c, dev, 8 if i % 2 else 16, c["B"])
    pinned = c["name"] in {p["name"] for p in fz.PINNED}
    last = len(c["appends"]) - 1
    for step, (a, (k, v)) in enumerate(zip(c["appends"], kv)):
        tk, tv = _kv_tensors(k, v, a, c, dev)
        tl = None if a["new_lens"] is None else torch.tensor(a["new_lens"], dtype=torch.int32, device=dev)
        for cache in (byte, dense, paged):
            cache.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        if step == last or pinned:
            _state(byte, dense, paged, slots, c, f"{c['name']} after append {step}")
    assert byte.seqlens.tolist() == c["lens"]
    tq = _query(fz, q, c, dev)
    for ns in c["splits"]:
        what = f"{c['name']} splits={ns}"
        opts = dict(tensor_layout=c["q_layout"], is_causal=c["is_causal"], sm_scale=c["sm_scale"], num_splits=ns, q_bits=c["q_bits"],
                    return_lse=True)
        want = lb.lowbit_fa_decode(tq, byte, **opts)
        _same(lb.lowbit_fa_decode(tq, dense, **opts), want, what + ": packed")
        _same(lb.lowbit_fa_decode(tq, paged, **opts), want, what + ": packed and paged")
        o_only = lb.lowbit_fa_decode(tq, dense, **dict(opts, return_lse=False))
        assert torch.equal(_bits(o_only), _bits(want[0])), what + ": O depends on return_lse"


@pytest.mark.parametrize("case", _prefill_cases(), ids=lambda c: c["name"])
def test_packed_twin_of_the_prefill_fuzz(oracle, dev, case):
    import lowbit_quant_fa2_paddle_amd as lb
    c = case
    q, kv = pz.make_data(oracle, c)
    byte, dense, paged = _caches(lb, c, dev, c["v_bits"], c["num_slots"])
    tq = _query(pz, q, c, dev)
    q_lens = None if c["q_lens_arg"] is None else torch.tensor(c["q_lens_arg"], dtype=torch.int32, device=dev)
    calls = 0
    for step, (a, (k, v)) in enumerate(zip(c["appends"], kv)):
        tk, tv = _kv_tensors(k, v, a, c, dev)
        tl = None if a["new_lens"] is None else torch.tensor(a["new_lens"], dtype=torch.int32, device=dev)
        byte.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        dense.append(tk, tv, tensor_layout=a["layout"], new_lens=tl)
        paged.append(tk, tv, slots=c["slots"], tensor_layout=a["layout"], new_lens=tl)
        _state(byte, dense, paged, c["slots"], c, f"{c['name']} after append {step}")
        if step not in c["calls"]:
            continue
        calls += 1
        for causal in (False, True):
            for ns in c["splits"]:
                what = f"{c['name']} step={step} causal={causal} splits={ns}"
                opts = dict(tensor_layout=c["q_layout"], is_causal=causal, sm_scale=c["sm_scale"], num_splits=ns, q_bits=c["q_bits"],
                            return_lse=True, q_lens=q_lens)
                want = lb.lowbit_fa_prefill(tq, byte, **opts)
                _same(lb.lowbit_fa_prefill(tq, dense, **opts), want, what + ": packed")
                _same(lb.lowbit_fa_prefill(tq, paged, slots=c["slots"], **opts), want, what + ": packed and paged")
                if pz.decode_takes_it(c):
                    del opts["q_lens"]
                    _same(lb.lowbit_fa_decode(tq, dense, **opts), lb.lowbit_fa_decode(tq, byte, **opts), what + ": decode, packed")
    assert calls and byte.seqlens.tolist() == c["lens"]
