"""C ABI of the nibble-packed K cache: each of the twelve cache entry points once more as `<name>_k4` (and `<name>_k4_v8` over the
fp8 V cache): exported, declared, with the sibling's signature, and refused BEFORE the first launch with LBFA_EINVAL and an exact
message, so none of this needs a GPU.  The tables hold the refusal that is new (an append whose k_qmax is not 7), k_codes off its
16-byte alignment, and EVERY refusal of the siblings' tables.  In the style of tests/test_v8_abi_cpu.py."""
import os

import pytest

from cabi_calls import DEFAULTS, A, P, call, check_table, lib  # noqa: F401 (lib: the fixture)

BASES = ["lbfa_kvcache_append", "lbfa_kvcache_paged_append", "lbfa_decode", "lbfa_decode_paged", "lbfa_prefill", "lbfa_prefill_paged"]
NEW = [b + s for b in BASES for s in ("_k4", "_k4_v8")]


def sibling(name):
    return name.replace("_k4", "")


# the default problems are the siblings'; an append quantises with k_qmax 7
for _name in NEW:
    DEFAULTS[_name] = dict(DEFAULTS[sibling(_name)], **({"k_qmax": 7} if "append" in _name else {}))


def test_new_symbols_are_exported_and_declared(lib):
    import ctypes
    from lowbit_quant_fa2_paddle_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lowbit_fa.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    assert len(NEW) == 12
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert name in integration, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sibling(name)], name  # the sibling's argument list
        assert len(_lib.SIGNATURES[name][1]) == len(DEFAULTS[name]), name
        # ... with k_codes typed uint8_t* in the header
        decl = header[header.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert "uint8_t* k_codes" in decl and " int8_t* k_codes" not in decl, name
    assert lib.lbfa_version() == 200  # additive: the version does not move


def test_refusals(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    table = []
    for name in NEW:
        paged = "paged" in name
        bad = " / block_table / slots" if paged else ""
        table += [(name, dict(k_codes=None), f"{name}: null pointer"),
                  (name, dict(D=80), "Unsupported head_dim: 80"),
                  (name, dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16")]
        if "append" in name:
            align = f"{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens{bad} 4-byte aligned"
            table += [(name, dict(k_qmax=127), f"{name}: k_qmax must be 7 (the codes of a nibble-packed cache take 4 bits), got 127"),
                      (name, dict(k_qmax=15), f"{name}: k_qmax must be 127 (int8) or 7 (int4 range), got 15"),
                      (name, dict(k_qmax=0), f"{name}: k_qmax must be 127 (int8) or 7 (int4 range), got 0")]
        else:
            ql = " / q_lens" if "prefill" in name else ""
            align = f"{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens{ql}{bad} / lse 4-byte aligned"
            need = 435200 if "prefill" in name else 17408  # the siblings' workspace sizes for the same problems
            table.append((name, dict(workspace_bytes=16), f"{name}: workspace too small (16 < {need})"))
        table += [(name, dict(k_codes=A(off)), align) for off in (1, 4, 8)]
        if name.endswith("_v8"):
            table.append((name, dict(v_scale=A(4)), f"{name}: v_scale must be 16-byte aligned"))
    check_table(lib, table)
    st, msg = call(lib, "lbfa_decode_k4", Sq=33)
    assert st == _lib.LBFA_EINVAL and "the limit is 64" in msg  # decode keeps its row limit, prefill has none
    with pytest.raises(ValueError, match="k_qmax must be 7"):
        _lib.check(call(lib, "lbfa_kvcache_append_k4_v8", k_qmax=127)[0], lib)


def test_every_refusal_of_a_sibling_is_the_twin_s(lib):
    """Every row of the three SINGLE_FAULT tables whose entry point has _k4 siblings, made against both of them (the _k4_v8 one
    with a valid v_scale): the same refusal, with only the name in front of the message changed."""
    import test_decode_abi_cpu as dec
    import test_paged_abi_cpu as paged
    import test_prefill_abi_cpu as prefill
    rows = [r for mod in (dec, paged, prefill) for r in mod.SINGLE_FAULT if r[0] in BASES]
    assert len(rows) == 176 and {r[0] for r in rows} == set(BASES)
    twins = []
    for name, overrides, message in rows:
        prefix = name + ": "
        for suffix in ("_k4", "_k4_v8"):
            twins.append((name + suffix, overrides, name + suffix + ": " + message[len(prefix):] if message.startswith(prefix) else message))
    check_table(lib, twins)


def test_workspace_sizes_and_split_rules_are_the_siblings(lib):
    # there is no _k4 query: the readers take lbfa_decode_workspace_bytes / lbfa_prefill_workspace_bytes as they are
    from lowbit_quant_fa2_paddle_amd import _lib
    assert not any("workspace" in n or "num_splits" in n for n in _lib.SIGNATURES if "_k4" in n)
    assert sum("_k4" in n for n in _lib.SIGNATURES) == 12


def test_front_end_takes_k_packed():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(ValueError, match="k_packed=True needs k_bits=4 .* got k_bits=8"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cuda", k_packed=True)
    with pytest.raises(ValueError, match="k_packed=True needs k_bits=4 .* got k_bits=8"):
        lb.LowbitPagedKVCache(4, 64, 2, 64, 1, 2, torch.float16, "cuda", k_bits=8, k_packed=True)
    with pytest.raises(ValueError, match="k_bits must be 8 or 4, got 2"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cuda", k_bits=2, k_packed=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cpu", k_bits=4, k_packed=True)
