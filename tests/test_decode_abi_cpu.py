"""C ABI of the int8 KV cache and of decode attention (`lbfa_kvcache_mean`, `lbfa_kvcache_append`, `lbfa_decode_num_splits`,
`lbfa_decode_workspace_bytes`, `lbfa_decode`): exported, declared, and every argument refused BEFORE the first launch with
LBFA_EINVAL and an exact message - so none of this needs a GPU.  Tables in the style of tests/test_bwd_abi_cpu.py."""
import os

import pytest

from cabi_calls import A, call, check_table, lib  # noqa: F401 (lib: the fixture)

# the default problems (cabi_calls.DEFAULTS): B 1, Hkv 2, D 64, T / Sq 8, capacity 128
NEW = ["lbfa_kvcache_mean", "lbfa_kvcache_append", "lbfa_decode_num_splits", "lbfa_decode_workspace_bytes", "lbfa_decode"]


def test_new_symbols_are_exported_and_declared(lib):
    import ctypes
    from lowbit_quant_fa2_paddle_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lowbit_fa.h")).read()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert lib.lbfa_version() == 200  # additive: the version does not move


SINGLE_FAULT = [
    ("lbfa_kvcache_mean", dict(k_new=None), "lbfa_kvcache_mean: null pointer"),
    ("lbfa_kvcache_mean", dict(new_lens=None), "lbfa_kvcache_mean: null pointer"),
    ("lbfa_kvcache_mean", dict(km=None), "lbfa_kvcache_mean: null pointer"),
    ("lbfa_kvcache_mean", dict(sk=None), "lbfa_kvcache_mean: null pointer"),
    ("lbfa_kvcache_mean", dict(T=0), "lbfa_kvcache_mean: empty tensor"),
    ("lbfa_kvcache_mean", dict(D=96), "Unsupported head_dim: 96"),
    ("lbfa_kvcache_mean", dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16"),
    ("lbfa_kvcache_mean", dict(k_new=A(8)), "lbfa_kvcache_mean: k_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_kvcache_mean", dict(B=65536), "lbfa_kvcache_mean: grid too large"),

    ("lbfa_kvcache_append", dict(k_new=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(v_new=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(sv=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(k_codes=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(k_scale=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(v_cache=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(k_tail=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(seqlens=None), "lbfa_kvcache_append: null pointer"),
    ("lbfa_kvcache_append", dict(B=0), "lbfa_kvcache_append: empty tensor"),
    ("lbfa_kvcache_append", dict(T=0), "lbfa_kvcache_append: empty tensor"),
    ("lbfa_kvcache_append", dict(D=80), "Unsupported head_dim: 80"),
    ("lbfa_kvcache_append", dict(capacity=100), "lbfa_kvcache_append: capacity must be a positive multiple of 64, got 100"),
    ("lbfa_kvcache_append", dict(capacity=0), "lbfa_kvcache_append: capacity must be a positive multiple of 64, got 0"),
    ("lbfa_kvcache_append", dict(dtype=7), "Input tensors must be in dtype of float16 or bfloat16"),
    ("lbfa_kvcache_append", dict(k_qmax=15), "lbfa_kvcache_append: k_qmax must be 127 (int8) or 7 (int4 range), got 15"),
    ("lbfa_kvcache_append", dict(k_new=A(2)), "lbfa_kvcache_append: k_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_kvcache_append", dict(sv=(1024, 512, 60)), "lbfa_kvcache_append: v_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_kvcache_append", dict(k_codes=A(8)),
     "lbfa_kvcache_append: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens 4-byte aligned"),
    ("lbfa_kvcache_append", dict(km=A(4)),
     "lbfa_kvcache_append: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens 4-byte aligned"),
    ("lbfa_kvcache_append", dict(new_lens=A(2)),
     "lbfa_kvcache_append: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens 4-byte aligned"),
    ("lbfa_kvcache_append", dict(Hkv=65536), "lbfa_kvcache_append: grid too large"),

    ("lbfa_decode", dict(q=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(sq=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(o=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(k_codes=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(k_scale=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(v_cache=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(seqlens=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(workspace=None), "lbfa_decode: null pointer"),
    ("lbfa_decode", dict(Sq=0), "lbfa_decode: empty tensor"),
    ("lbfa_decode", dict(D=96), "Unsupported head_dim: 96"),
    ("lbfa_decode", dict(Hq=3), "num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    ("lbfa_decode", dict(Sq=33),
     "lbfa_decode: Sq * (Hq / Hkv) = 66 query rows per kv head, the limit is 64 (longer queries belong on the dense operator)"),
    ("lbfa_decode", dict(Hq=16, Sq=9),
     "lbfa_decode: Sq * (Hq / Hkv) = 72 query rows per kv head, the limit is 64 (longer queries belong on the dense operator)"),
    ("lbfa_decode", dict(capacity=127), "lbfa_decode: capacity must be a positive multiple of 64, got 127"),
    ("lbfa_decode", dict(max_seqlen_k=129), "lbfa_decode: max_seqlen_k must be in [1, capacity], got 129 (capacity 128)"),
    ("lbfa_decode", dict(max_seqlen_k=0), "lbfa_decode: max_seqlen_k must be in [1, capacity], got 0 (capacity 128)"),
    ("lbfa_decode", dict(num_splits=-1), "lbfa_decode: num_splits must be in [0, 65535] (0: chosen by lbfa_decode_num_splits), got -1"),
    ("lbfa_decode", dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16"),
    ("lbfa_decode", dict(q_qmax=8), "lbfa_decode: q_qmax must be 127 (int8) or 7 (int4 range), got 8"),
    ("lbfa_decode", dict(sm_scale=0.0), "lbfa_decode: sm_scale must be positive"),
    ("lbfa_decode", dict(q=A(8)), "lbfa_decode: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_decode", dict(sq=(2048, 512, 68)), "lbfa_decode: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_decode", dict(o=A(4)), "lbfa_decode: o must be 8-byte aligned with strides that are multiples of 4 elements"),
    ("lbfa_decode", dict(v_cache=A(8)), "lbfa_decode: cache tensors and km must be 16-byte aligned, k_scale / seqlens / lse 4-byte aligned"),
    ("lbfa_decode", dict(lse=A(2)), "lbfa_decode: cache tensors and km must be 16-byte aligned, k_scale / seqlens / lse 4-byte aligned"),
    ("lbfa_decode", dict(workspace_bytes=16), "lbfa_decode: workspace too small (16 < 17408)"),
    ("lbfa_decode", dict(workspace=A(8)), "lbfa_decode: workspace must be 16-byte aligned"),
    ("lbfa_decode", dict(B=65536, workspace_bytes=1 << 40), "lbfa_decode: grid too large"),
]


def test_single_fault_table(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    check_table(lib, SINGLE_FAULT)
    with pytest.raises(ValueError, match="the limit is 64"):
        _lib.check(call(lib, "lbfa_decode", Sq=33)[0], lib)


def _splits(B, Hkv, max_k):
    """the documented rule: min(ceil(1024 / (B Hkv)), tiles / 4, 256), at least 1"""
    tiles = (max_k + 63) // 64
    return max(1, min(-(-1024 // (B * Hkv)), tiles // 4, 256))


def test_split_choice_is_pinned(lib):
    pinned = {(1, 8, 4096): 16, (1, 8, 32768): 128, (1, 8, 131072): 128, (8, 8, 4096): 16, (8, 8, 32768): 16, (64, 8, 4096): 2,
              (64, 8, 131072): 2, (1, 1, 1 << 20): 256, (1, 8, 255): 1, (1, 8, 256): 1, (1, 8, 512): 2, (2048, 1, 65536): 1,
              (1, 8, 1): 1}
    for (B, Hkv, max_k), want in pinned.items():
        assert lib.lbfa_decode_num_splits(B, Hkv, max_k) == want == _splits(B, Hkv, max_k), (B, Hkv, max_k)
    for B in (1, 2, 3, 8, 64, 500):
        for Hkv in (1, 2, 8, 32):
            for max_k in (1, 63, 64, 65, 255, 257, 1000, 4133, 32768, 131072, 1 << 20):
                assert lib.lbfa_decode_num_splits(B, Hkv, max_k) == _splits(B, Hkv, max_k), (B, Hkv, max_k)
    assert lib.lbfa_decode_num_splits(0, 8, 4096) == 1 and lib.lbfa_decode_num_splits(1, 8, 0) == 1


def _align256(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes_are_pinned(lib):
    def want(B, Hq, Hkv, Sq, D, splits):
        if splits <= 1:
            return 0
        rows = B * Hkv * splits * Sq * (Hq // Hkv)
        return _align256(rows * D * 4) + _align256(rows * 16)

    assert lib.lbfa_decode_workspace_bytes(1, 4, 2, 8, 64, 128, 2) == 17408  # the default problem of the table above
    for B, Hq, Hkv, Sq, D in [(1, 32, 8, 1, 128), (8, 32, 8, 1, 128), (2, 4, 4, 16, 64), (3, 8, 2, 4, 64), (1, 8, 1, 8, 128)]:
        for max_k in (64, 4096, 32768):
            for splits in (0, 1, 2, 7, 128):
                eff = splits or _splits(B, Hkv, max_k)
                assert lib.lbfa_decode_workspace_bytes(B, Hq, Hkv, Sq, D, max_k, splits) == want(B, Hq, Hkv, Sq, D, eff), \
                    (B, Hq, Hkv, Sq, D, max_k, splits)
    assert lib.lbfa_decode_workspace_bytes(1, 32, 8, 1, 80, 4096, 4) == 0   # the caller pads to 64 / 128
    assert lib.lbfa_decode_workspace_bytes(1, 30, 8, 1, 64, 4096, 4) == 0   # Hq % Hkv
    assert lib.lbfa_decode_workspace_bytes(0, 32, 8, 1, 64, 4096, 4) == 0


def test_front_end_is_exported_and_forward_only():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    assert lb.sageattn_decode is lb.lowbit_fa_decode
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cpu")
    with pytest.raises(ValueError, match="k_bits"):
        lb.LowbitKVCache(1, 2, 64, 128, torch.float16, "cuda", k_bits=5)
    with pytest.raises(ValueError, match="Unsupported head_dim: 256"):
        lb.LowbitKVCache(1, 2, 256, 128, torch.float16, "cuda")
    q = torch.zeros(1, 2, 1, 64, dtype=torch.float16, requires_grad=True)
    cache = object.__new__(lb.LowbitKVCache)  # no device needed: the grad check comes first
    with pytest.raises(RuntimeError, match="forward-only"):
        lb.lowbit_fa_decode(q, cache)


# ------------------------------------------------------------------------------------------------------------------------
# the ORDER of the checks: calls with two faults that are neighbours in check_append / check_decode - the earlier check's
# message wins.  Over the contiguous and the paged entry point and their _v8 siblings; a fault is a dict of overrides, or
# {paged: overrides} where the two layouts differ.  The texts are those of the library before the cache section of
# lbfa_api.hip described an append and a read once; {name} is the entry point, {lens} / {ids} what the prefill / paged forms add.
# ------------------------------------------------------------------------------------------------------------------------
_BAD_POOL = {False: dict(capacity=100), True: dict(page_size=96)}
_POOL_TEXT = {False: "{name}: capacity must be a positive multiple of 64, got 100", True: "{name}: page_size must be a positive multiple of 64, got 96"}
_HUGE = {False: dict(B=65536, workspace_bytes=1 << 44), True: dict(B=65536, num_slots=65536, workspace_bytes=1 << 44)}
APPEND_ORDER = [  # (the earlier fault, the later fault, the message: the earlier one's)
    (dict(k_codes=None), dict(T=0), "{name}: null pointer"),
    (dict(T=0), dict(D=80), "{name}: empty tensor"),
    (dict(D=80), _BAD_POOL, "Unsupported head_dim: 80"),
    (_BAD_POOL, dict(dtype=7), _POOL_TEXT),
    (dict(dtype=7), dict(k_qmax=15), "Input tensors must be in dtype of float16 or bfloat16"),
    (dict(k_qmax=15), dict(k_new=A(2)), "{name}: k_qmax must be 127 (int8) or 7 (int4 range), got 15"),
    (dict(k_new=A(2)), dict(sv=(1024, 512, 60)), "{name}: k_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    (dict(sv=(1024, 512, 60)), dict(k_codes=A(8)), "{name}: v_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    (dict(k_codes=A(8)), dict(Hkv=65536), "{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens{ids} 4-byte aligned"),
]
APPEND_ORDER_PAGED = [  # inside check_pool
    (dict(page_size=96), dict(num_pages=0), "{name}: page_size must be a positive multiple of 64, got 96"),
    (dict(num_pages=0), dict(page_size=1 << 30), "{name}: num_pages, num_slots and max_pages_per_seq must be at least 1, got 0, 2 and 2"),
    (dict(page_size=1 << 30), dict(B=3), "{name}: max_pages_per_seq * page_size must stay below 2^31 keys"),
    (dict(B=3), dict(dtype=7), "{name}: B (3) exceeds num_slots (2)"),
]
APPEND_ORDER_V8 = [  # the alignment of v_scale sits between the cache tensors' and the grid
    (dict(k_codes=A(8)), dict(v_scale=A(4)), "{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens{ids} 4-byte aligned"),
    (dict(v_scale=A(4)), dict(Hkv=65536), "{name}: v_scale must be 16-byte aligned"),
]
READ_ORDER = [
    (dict(q=None), dict(Sq=0), "{name}: null pointer"),
    (dict(Sq=0), dict(D=96), "{name}: empty tensor"),
    (dict(D=96), dict(Hq=3), "Unsupported head_dim: 96"),
    (dict(Hq=3), _BAD_POOL, "num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    (_BAD_POOL, dict(max_seqlen_k=0), _POOL_TEXT),
    (dict(max_seqlen_k=0), dict(num_splits=-1), {False: "{name}: max_seqlen_k must be in [1, capacity], got 0 (capacity {keys})",
                                                 True: "{name}: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got 0 (limit {keys})"}),
    (dict(num_splits=-1), dict(dtype=2), "{name}: num_splits must be in [0, 65535] (0: chosen by lbfa_{op}_num_splits), got -1"),
    (dict(dtype=2), dict(q_qmax=8), "Input tensors must be in dtype of float16 or bfloat16"),
    (dict(q_qmax=8), dict(sm_scale=0.0), "{name}: q_qmax must be 127 (int8) or 7 (int4 range), got 8"),
    (dict(sm_scale=0.0), dict(q=A(8)), "{name}: sm_scale must be positive"),
    (dict(q=A(8)), dict(o=A(4)), "{name}: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    (dict(o=A(4)), dict(k_codes=A(8)), "{name}: o must be 8-byte aligned with strides that are multiples of 4 elements"),
    (dict(k_codes=A(8)), dict(workspace_bytes=16), "{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens{lens}{ids} / lse 4-byte aligned"),
    (dict(workspace_bytes=16), dict(workspace=A(8)), "{name}: workspace too small (16 < {need})"),
    (dict(workspace=A(8)), _HUGE, "{name}: workspace must be 16-byte aligned"),
    (dict(workspace=None), _HUGE, "{name}: null pointer"),
]
READ_ORDER_DECODE = [  # the row limit sits between the GQA check and the pool's
    (dict(Hq=3), dict(Sq=33), "num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    (dict(Sq=33), _BAD_POOL, "{name}: Sq * (Hq / Hkv) = 66 query rows per kv head, the limit is 64 (longer queries belong on the dense operator)"),
]
READ_ORDER_PREFILL = [  # the grid of the prefill kernel and of the combine sits between the alignments and the workspace
    (dict(k_codes=A(8)), dict(Sq=257 * 128, num_splits=65535), "{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens{lens}{ids} / lse 4-byte aligned"),
    (dict(Sq=257 * 128, num_splits=65535), dict(workspace_bytes=16),
     "{name}: grid too large (Sq * (Hq / Hkv) and ceil(Sq / 128) * num_splits must stay below 2^24, Hq below 65536)"),
]
READ_ORDER_V8 = [
    (dict(k_codes=A(8)), dict(v_scale=A(4)), "{name}: cache tensors and km must be 16-byte aligned, k_scale / seqlens{lens}{ids} / lse 4-byte aligned"),
    (dict(v_scale=A(4)), dict(workspace_bytes=16), "{name}: v_scale must be 16-byte aligned"),
]


def _check_order(lib, names, tables):
    """every (earlier, later, message) of the tables that apply to a name: each fault alone is refused, the later one with
    another message, and both together give the earlier one's"""
    from lowbit_quant_fa2_paddle_amd import _lib
    for name in names:
        paged, prefill = "paged" in name, "prefill" in name
        words = dict(name=name, ids=" / block_table / slots" if paged else "", lens=" / q_lens" if prefill else "",
                     op="prefill" if prefill else "decode", keys=256 if prefill else 128, need=435200 if prefill else 17408)
        rows = [r for applies, table in tables for r in table if applies(name)]
        assert rows, name
        for first, second, message in rows:
            first, second, message = (x[paged] if set(x) == {False, True} else x for x in (first, second, message))
            message = message.format(**words)
            assert call(lib, name, **first) == (_lib.LBFA_EINVAL, message), (name, first)
            st, alone = call(lib, name, **second)
            assert st == _lib.LBFA_EINVAL and alone != message, (name, second, alone)
            assert call(lib, name, **first, **second) == (_lib.LBFA_EINVAL, message), (name, first, second)


def test_append_checks_come_in_order(lib):
    appends = ["lbfa_kvcache_append", "lbfa_kvcache_paged_append", "lbfa_kvcache_append_v8", "lbfa_kvcache_paged_append_v8"]
    _check_order(lib, appends, [(lambda n: True, APPEND_ORDER), (lambda n: "paged" in n, APPEND_ORDER_PAGED),
                                (lambda n: n.endswith("_v8"), APPEND_ORDER_V8)])


def test_read_checks_come_in_order(lib):
    reads = [op + layout + v for op in ("lbfa_decode", "lbfa_prefill") for layout in ("", "_paged") for v in ("", "_v8")]
    _check_order(lib, reads, [(lambda n: True, READ_ORDER), (lambda n: "decode" in n, READ_ORDER_DECODE),
                              (lambda n: "prefill" in n, READ_ORDER_PREFILL), (lambda n: n.endswith("_v8"), READ_ORDER_V8)])
