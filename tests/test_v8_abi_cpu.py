"""C ABI of the fp8 V cache (`lbfa_kvcache_append_v8`, `lbfa_kvcache_paged_append_v8`, `lbfa_decode_v8`, `lbfa_decode_paged_v8`,
`lbfa_prefill_v8`, `lbfa_prefill_paged_v8`): exported, declared, and refused BEFORE the first launch with LBFA_EINVAL and an exact
message, so none of this needs a GPU.  Each entry point is its sibling with `v_scale` behind `v_cache`; the tables hold the two
refusals that are new and a sample of the siblings' (head dim, null cache pointer).  In the style of tests/test_decode_abi_cpu.py."""
import os

import pytest

from cabi_calls import DEFAULTS, V8, A, P, call, check_table, lib  # noqa: F401 (lib: the fixture)

# the default problems (cabi_calls.DEFAULTS) are the siblings' with v_scale behind v_cache
NEW = ["lbfa_kvcache_append_v8", "lbfa_kvcache_paged_append_v8", "lbfa_decode_v8", "lbfa_decode_paged_v8", "lbfa_prefill_v8",
       "lbfa_prefill_paged_v8"]


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
            need = 435200 if "prefill" in name else 17408  # pinned by the siblings' tables for the same problems
            table.append((name, dict(workspace_bytes=16), f"{name}: workspace too small (16 < {need})"))
            table.append((name, dict(Hq=3), "num_qo_heads (3) must be divisible by num_kv_heads (2)"))
        if paged:
            table.append((name, dict(page_size=100), f"{name}: page_size must be a positive multiple of 64, got 100"))
        else:
            table.append((name, dict(capacity=100), f"{name}: capacity must be a positive multiple of 64, got 100"))
    check_table(lib, table)
    st, msg = call(lib, "lbfa_decode_v8", Sq=33)
    assert st == _lib.LBFA_EINVAL and "the limit is 64" in msg  # decode keeps its row limit, prefill has none
    with pytest.raises(ValueError, match="v_scale must be 16-byte aligned"):
        _lib.check(call(lib, "lbfa_prefill_v8", v_scale=A(4))[0], lib)


def test_every_refusal_of_a_sibling_is_the_twin_s(lib):
    """Every row of the three SINGLE_FAULT tables whose entry point has a _v8 sibling, made against the sibling with a valid
    v_scale: the same refusal, with only the name in front of the message changed (a prefix: `lbfa_decode_num_splits` inside a
    message stays)."""
    import test_decode_abi_cpu as dec
    import test_paged_abi_cpu as paged
    import test_prefill_abi_cpu as prefill
    rows = [r for mod in (dec, paged, prefill) for r in mod.SINGLE_FAULT if r[0] in V8]
    assert len(rows) == 176 and {r[0] for r in rows} == set(V8)
    twins = []
    for name, overrides, message in rows:
        prefix = name + ": "
        twins.append((name + "_v8", dict(overrides, v_scale=P),
                      name + "_v8: " + message[len(prefix):] if message.startswith(prefix) else message))
    check_table(lib, twins)


def test_front_end_takes_v_bits():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 3"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cuda", v_bits=3)
    with pytest.raises(ValueError, match="v_bits must be 16 or 8, got 4"):
        lb.LowbitPagedKVCache(4, 64, 2, 64, 1, 2, torch.float16, "cuda", v_bits=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cpu", v_bits=8)
