"""C ABI of the fp8 V cache (`lbfa_kvcache_append_v8`, `lbfa_kvcache_paged_append_v8`, `lbfa_decode_v8`, `lbfa_decode_paged_v8`,
`lbfa_prefill_v8`, `lbfa_prefill_paged_v8`): exported, declared, and refused BEFORE the first launch with LBFA_EINVAL and an exact
message, so none of this needs a GPU.  Each entry point is its sibling with `v_scale` behind `v_cache`; the tables hold the two
refusals that are new and a sample of the siblings' (head dim, null cache pointer).  In the style of tests/test_decode_abi_cpu.py."""
import os

import pytest

import cabi_calls
from cabi_calls import A, P, S3

NEW = ["lbfa_kvcache_append_v8", "lbfa_kvcache_paged_append_v8", "lbfa_decode_v8", "lbfa_decode_paged_v8", "lbfa_prefill_v8",
       "lbfa_prefill_paged_v8"]
WS = 1 << 15
_POOL = dict(num_slots=1, num_pages=2, page_size=64, max_pages=2)
_Q = dict(sq=(2048, 512, 64), so=(2048, 512, 64), sm_scale=0.125, q_qmax=127, causal=0, stream=None)
# name -> arguments in ABI order with the values of a small valid problem: B 1, Hkv 2, D 64, T / Sq 8, 128 keys of room
DEFAULTS = {
    "lbfa_kvcache_append_v8": dict(k_new=P, v_new=P, dtype=0, new_lens=None, km=P, k_codes=P, k_scale=P, v_cache=P, v_scale=P,
                                   k_tail=P, seqlens=P, B=1, Hkv=2, T=8, D=64, capacity=128, sk=S3, sv=S3, k_qmax=127, stream=None),
    "lbfa_kvcache_paged_append_v8": dict(k_new=P, v_new=P, dtype=0, new_lens=None, km=P, k_codes=P, k_scale=P, v_cache=P, v_scale=P,
                                         k_tail=P, seqlens=P, block_table=P, slots=None, B=1, Hkv=2, T=8, D=64, **_POOL, sk=S3,
                                         sv=S3, k_qmax=127, stream=None),
    "lbfa_decode_v8": dict(q=P, dtype=0, k_codes=P, k_scale=P, v_cache=P, v_scale=P, km=P, seqlens=P, o=P, lse=None, workspace=P,
                           workspace_bytes=WS, B=1, Hq=4, Hkv=2, Sq=8, D=64, capacity=128, max_seqlen_k=128, num_splits=2, **_Q),
    "lbfa_decode_paged_v8": dict(q=P, dtype=0, k_codes=P, k_scale=P, v_cache=P, v_scale=P, km=P, seqlens=P, block_table=P,
                                 slots=None, o=P, lse=None, workspace=P, workspace_bytes=WS, B=1, Hq=4, Hkv=2, Sq=8, D=64, **_POOL,
                                 max_seqlen_k=128, num_splits=2, **_Q),
    "lbfa_prefill_v8": dict(q=P, dtype=0, k_codes=P, k_scale=P, v_cache=P, v_scale=P, km=P, seqlens=P, q_lens=None, o=P, lse=None,
                            workspace=P, workspace_bytes=WS, B=1, Hq=4, Hkv=2, Sq=8, D=64, capacity=128, max_seqlen_k=128,
                            num_splits=2, **_Q),
    "lbfa_prefill_paged_v8": dict(q=P, dtype=0, k_codes=P, k_scale=P, v_cache=P, v_scale=P, km=P, seqlens=P, q_lens=None,
                                  block_table=P, slots=None, o=P, lse=None, workspace=P, workspace_bytes=WS, B=1, Hq=4, Hkv=2, Sq=8,
                                  D=64, **_POOL, max_seqlen_k=128, num_splits=2, **_Q),
}


@pytest.fixture(scope="module")
def lib():
    from lowbit_quant_fa2_paddle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def call(lib, name, **overrides):
    args = dict(DEFAULTS[name])
    assert overrides and set(overrides) <= set(args), (name, overrides)
    args.update(overrides)
    st = getattr(lib, name)(*[cabi_calls._arg(v) for v in args.values()])
    return st, lib.lbfa_last_error().decode()


def test_new_symbols_are_exported_and_declared(lib):
    import ctypes
    from lowbit_quant_fa2_paddle_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lowbit_fa.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert name in integration, name
        sibling = _lib.SIGNATURES[name[:-3]][1]
        assert len(_lib.SIGNATURES[name][1]) == len(sibling) + 1 == len(DEFAULTS[name]), name
    assert lib.lbfa_version() == 200  # additive: the version does not move


def test_refusals(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    table = []
    for name in NEW:
        table += [(name, dict(v_scale=None), f"{name}: null pointer"),
                  (name, dict(v_scale=A(4)), f"{name}: v_scale must be 16-byte aligned"),
                  (name, dict(v_scale=A(8)), f"{name}: v_scale must be 16-byte aligned"),
                  (name, dict(v_cache=None), f"{name}: null pointer"),
                  (name, dict(k_codes=None), f"{name}: null pointer"),
                  (name, dict(D=80), "Unsupported head_dim: 80"),
                  (name, dict(D=96), "Unsupported head_dim: 96"),
                  (name, dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16")]
        paged = "paged" in name
        bad = " / block_table / slots" if paged else ""
        if "append" in name:
            table.append((name, dict(v_cache=A(8)), f"{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens{bad} "
                                                    "4-byte aligned"))
            table.append((name, dict(T=0), f"{name}: empty tensor"))
        else:
            ql = " / q_lens" if "prefill" in name else ""
            table.append((name, dict(v_cache=A(8)), f"{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens{ql}{bad} / lse "
                                                    "4-byte aligned"))
            table.append((name, dict(workspace_bytes=16), f"{name}: workspace too small (16 < 17408)"))
            table.append((name, dict(Hq=3), "num_qo_heads (3) must be divisible by num_kv_heads (2)"))
        if paged:
            table.append((name, dict(page_size=100), f"{name}: page_size must be a positive multiple of 64, got 100"))
        else:
            table.append((name, dict(capacity=100), f"{name}: capacity must be a positive multiple of 64, got 100"))
    for name, overrides, message in table:
        st, msg = call(lib, name, **overrides)
        assert st == _lib.LBFA_EINVAL, (name, overrides, st, msg)
        assert msg == message, (name, overrides, msg)
    st, msg = call(lib, "lbfa_decode_v8", Sq=33)
    assert st == _lib.LBFA_EINVAL and "the limit is 64" in msg  # decode keeps its row limit, prefill has none
    with pytest.raises(ValueError, match="v_scale must be 16-byte aligned"):
        _lib.check(call(lib, "lbfa_prefill_v8", v_scale=A(4))[0], lib)


def test_front_end_takes_v_bits():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 3"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cuda", v_bits=3)
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 4"):
        lb.LowbitPagedKVCache(4, 64, 2, 64, 1, 2, torch.float16, "cuda", v_bits=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cpu", v_bits=8)
