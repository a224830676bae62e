"""C ABI of cached prefill (`lbfa_prefill_num_splits`, `lbfa_prefill_workspace_bytes`, `lbfa_prefill`, `lbfa_prefill_paged`):
exported, declared, and every argument refused BEFORE the first launch with LBFA_EINVAL and an exact message - none of this
needs a GPU.  Tables in the style of tests/test_decode_abi_cpu.py."""
import os

import pytest

from cabi_calls import A, call, check_table, lib  # noqa: F401 (lib: the fixture)

# the default problems (cabi_calls.DEFAULTS): B 1, Hq 4, Hkv 2, Sq 200 (two Q blocks), D 64, 256 keys of room (pages of 128)
NEW = ["lbfa_prefill_num_splits", "lbfa_prefill_workspace_bytes", "lbfa_prefill", "lbfa_prefill_paged"]


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
    assert "#define LBFA_VERSION 200" in header


_ALIGN = "cache tensors and km must be 16-byte aligned, k_scale / seqlens / q_lens / lse 4-byte aligned"
_ALIGN_P = "cache tensors and km must be 16-byte aligned, k_scale / seqlens / q_lens / block_table / slots / lse 4-byte aligned"
_GRID = "grid too large (Sq * (Hq / Hkv) and ceil(Sq / 128) * num_splits must stay below 2^24, Hq below 65536)"
SINGLE_FAULT = [
    ("lbfa_prefill", dict(q=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(sq=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(o=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(so=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(k_codes=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(k_scale=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(v_cache=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(seqlens=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(workspace=None), "lbfa_prefill: null pointer"),
    ("lbfa_prefill", dict(Sq=0), "lbfa_prefill: empty tensor"),
    ("lbfa_prefill", dict(B=0), "lbfa_prefill: empty tensor"),
    ("lbfa_prefill", dict(D=96), "Unsupported head_dim: 96"),
    ("lbfa_prefill", dict(Hq=3), "num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    ("lbfa_prefill", dict(capacity=127), "lbfa_prefill: capacity must be a positive multiple of 64, got 127"),
    ("lbfa_prefill", dict(capacity=0), "lbfa_prefill: capacity must be a positive multiple of 64, got 0"),
    ("lbfa_prefill", dict(max_seqlen_k=257), "lbfa_prefill: max_seqlen_k must be in [1, capacity], got 257 (capacity 256)"),
    ("lbfa_prefill", dict(max_seqlen_k=0), "lbfa_prefill: max_seqlen_k must be in [1, capacity], got 0 (capacity 256)"),
    ("lbfa_prefill", dict(num_splits=-1), "lbfa_prefill: num_splits must be in [0, 65535] (0: chosen by lbfa_prefill_num_splits), got -1"),
    ("lbfa_prefill", dict(num_splits=65536), "lbfa_prefill: num_splits must be in [0, 65535] (0: chosen by lbfa_prefill_num_splits), got 65536"),
    ("lbfa_prefill", dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16"),
    ("lbfa_prefill", dict(q_qmax=8), "lbfa_prefill: q_qmax must be 127 (int8) or 7 (int4 range), got 8"),
    ("lbfa_prefill", dict(sm_scale=0.0), "lbfa_prefill: sm_scale must be positive"),
    ("lbfa_prefill", dict(q=A(8)), "lbfa_prefill: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_prefill", dict(sq=(51200, 12800, 68)), "lbfa_prefill: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    ("lbfa_prefill", dict(o=A(4)), "lbfa_prefill: o must be 8-byte aligned with strides that are multiples of 4 elements"),
    ("lbfa_prefill", dict(v_cache=A(8)), "lbfa_prefill: " + _ALIGN),
    ("lbfa_prefill", dict(km=A(8)), "lbfa_prefill: " + _ALIGN),
    ("lbfa_prefill", dict(q_lens=A(2)), "lbfa_prefill: " + _ALIGN),
    ("lbfa_prefill", dict(lse=A(2)), "lbfa_prefill: " + _ALIGN),
    ("lbfa_prefill", dict(workspace_bytes=16), "lbfa_prefill: workspace too small (16 < 435200)"),
    ("lbfa_prefill", dict(workspace=A(8)), "lbfa_prefill: workspace must be 16-byte aligned"),
    ("lbfa_prefill", dict(B=65536, workspace_bytes=1 << 44), "lbfa_prefill: grid too large"),
    ("lbfa_prefill", dict(Hq=65536, Hkv=1, num_splits=1), "lbfa_prefill: " + _GRID),
    ("lbfa_prefill", dict(Sq=1 << 30, Hq=8, Hkv=2, num_splits=1), "lbfa_prefill: " + _GRID),
    ("lbfa_prefill", dict(Sq=1 << 23, num_splits=1), "lbfa_prefill: " + _GRID),            # the combine's grid: M = 2^24 rows
    ("lbfa_prefill", dict(Sq=257 * 128, num_splits=65535), "lbfa_prefill: " + _GRID),     # 257 Q blocks x 65535 slices >= 2^24
    ("lbfa_prefill_paged", dict(Sq=257 * 128, num_splits=65535), "lbfa_prefill_paged: " + _GRID),

    ("lbfa_prefill_paged", dict(block_table=None), "lbfa_prefill_paged: null pointer"),
    ("lbfa_prefill_paged", dict(q=None), "lbfa_prefill_paged: null pointer"),
    ("lbfa_prefill_paged", dict(Sq=0), "lbfa_prefill_paged: empty tensor"),
    ("lbfa_prefill_paged", dict(D=80), "Unsupported head_dim: 80"),
    ("lbfa_prefill_paged", dict(page_size=100), "lbfa_prefill_paged: page_size must be a positive multiple of 64, got 100"),
    ("lbfa_prefill_paged", dict(num_pages=0),
     "lbfa_prefill_paged: num_pages, num_slots and max_pages_per_seq must be at least 1, got 0, 2 and 2"),
    ("lbfa_prefill_paged", dict(max_pages_per_seq=1 << 25), "lbfa_prefill_paged: max_pages_per_seq * page_size must stay below 2^31 keys"),
    ("lbfa_prefill_paged", dict(B=3), "lbfa_prefill_paged: B (3) exceeds num_slots (2)"),
    ("lbfa_prefill_paged", dict(max_seqlen_k=257),
     "lbfa_prefill_paged: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got 257 (limit 256)"),
    ("lbfa_prefill_paged", dict(num_splits=-2),
     "lbfa_prefill_paged: num_splits must be in [0, 65535] (0: chosen by lbfa_prefill_num_splits), got -2"),
    ("lbfa_prefill_paged", dict(q_qmax=15), "lbfa_prefill_paged: q_qmax must be 127 (int8) or 7 (int4 range), got 15"),
    ("lbfa_prefill_paged", dict(block_table=A(2)), "lbfa_prefill_paged: " + _ALIGN_P),
    ("lbfa_prefill_paged", dict(slots=A(2)), "lbfa_prefill_paged: " + _ALIGN_P),
    ("lbfa_prefill_paged", dict(q_lens=A(1)), "lbfa_prefill_paged: " + _ALIGN_P),
    ("lbfa_prefill_paged", dict(workspace_bytes=100), "lbfa_prefill_paged: workspace too small (100 < 435200)"),
]


def test_single_fault_table(lib):
    check_table(lib, SINGLE_FAULT)


def test_decode_still_refuses_long_queries(lib):
    st, msg = call(lib, "lbfa_decode", Sq=33)
    assert st == 1 and "the limit is 64" in msg


def _splits(B, Hq, Sq, max_k):
    """the documented rule: max(1, min(ceil(512 / (B Hq ceil(Sq / 128))), tiles / 4, 256))"""
    tiles = (max_k + 63) // 64
    return max(1, min(-(-512 // (B * Hq * ((Sq + 127) // 128))), tiles // 4, 256))


def test_split_choice_is_pinned(lib):
    pinned = {(1, 32, 128, 4096): 16, (1, 32, 512, 32768): 4, (1, 32, 2048, 131072): 1, (8, 32, 128, 4096): 2,
              (1, 32, 8192, 8192): 1, (1, 1, 1, 1 << 20): 256, (1, 4, 65, 255): 1, (1, 4, 65, 256): 1, (1, 4, 65, 512): 2,
              (1, 1, 129, 1 << 20): 256, (2, 4, 200, 321): 1, (1, 8, 1, 1): 1}
    for (B, Hq, Sq, max_k), want in pinned.items():
        assert lib.lbfa_prefill_num_splits(B, Hq, Sq, max_k) == want == _splits(B, Hq, Sq, max_k), (B, Hq, Sq, max_k)
    for B in (1, 2, 8, 64):
        for Hq in (1, 4, 32):
            for Sq in (1, 64, 128, 129, 2048, 8192):
                for max_k in (1, 63, 64, 65, 255, 257, 4133, 32768, 131072, 1 << 20):
                    assert lib.lbfa_prefill_num_splits(B, Hq, Sq, max_k) == _splits(B, Hq, Sq, max_k), (B, Hq, Sq, max_k)
    assert lib.lbfa_prefill_num_splits(0, 8, 128, 4096) == 1 and lib.lbfa_prefill_num_splits(1, 8, 0, 4096) == 1


def test_the_call_uses_the_prefill_split_rule(lib):
    """num_splits = 0 inside the call is lbfa_prefill_num_splits, not decode's rule: one byte less than
    lbfa_prefill_workspace_bytes(..., 0) is refused with exactly that size (64 slices here; decode's rule would take 256)"""
    for name in ("lbfa_prefill", "lbfa_prefill_paged"):
        kw = dict(capacity=65536) if name == "lbfa_prefill" else dict(page_size=8192, max_pages_per_seq=8)
        assert lib.lbfa_prefill_num_splits(1, 4, 200, 65536) == 64 and lib.lbfa_decode_num_splits(1, 2, 65536) == 256
        need = lib.lbfa_prefill_workspace_bytes(1, 4, 2, 200, 64, 65536, 0)
        assert need == lib.lbfa_prefill_workspace_bytes(1, 4, 2, 200, 64, 65536, 64) > 0
        st, msg = call(lib, name, max_seqlen_k=65536, num_splits=0, workspace_bytes=need - 1, **kw)
        assert st == 1 and msg == f"{name}: workspace too small ({need - 1} < {need})", msg


def _align256(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes_are_pinned(lib):
    def want(B, Hq, Hkv, Sq, D, splits):
        if splits <= 1:
            return 0
        rows = B * Hkv * splits * Sq * (Hq // Hkv)
        return _align256(rows * D * 4) + _align256(rows * 16)

    assert lib.lbfa_prefill_workspace_bytes(1, 4, 2, 200, 64, 256, 2) == 435200  # the default problem of the table above
    for B, Hq, Hkv, Sq, D in [(1, 32, 8, 128, 128), (8, 32, 8, 512, 128), (2, 4, 2, 200, 64), (3, 8, 2, 65, 64)]:
        for max_k in (64, 4096, 32768):
            for splits in (0, 1, 2, 7, 128):
                eff = splits or _splits(B, Hq, Sq, max_k)
                assert lib.lbfa_prefill_workspace_bytes(B, Hq, Hkv, Sq, D, max_k, splits) == want(B, Hq, Hkv, Sq, D, eff), \
                    (B, Hq, Hkv, Sq, D, max_k, splits)
    assert lib.lbfa_prefill_workspace_bytes(1, 32, 8, 128, 80, 4096, 4) == 0   # the caller pads to 64 / 128
    assert lib.lbfa_prefill_workspace_bytes(1, 30, 8, 128, 64, 4096, 4) == 0   # Hq % Hkv


def test_front_end_is_exported_and_forward_only():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    assert lb.sageattn_prefill is lb.lowbit_fa_prefill
    q = torch.zeros(1, 2, 200, 64, dtype=torch.float16, requires_grad=True)
    cache = object.__new__(lb.LowbitKVCache)  # no device needed: the grad check comes first
    with pytest.raises(RuntimeError, match="lowbit_fa_prefill is forward-only"):
        lb.lowbit_fa_prefill(q, cache)
    with pytest.raises(RuntimeError, match="lowbit_fa_decode is forward-only: there is no backward through the KV cache"):
        lb.lowbit_fa_decode(q, cache)
    with pytest.raises(TypeError, match="LowbitKVCache or a LowbitPagedKVCache"):
        lb.lowbit_fa_prefill(q.detach(), object())


def test_grid_limits_hold_the_launch_limit():
    """what the refusals above protect: gridDim.x * 256 threads below 2^32 for the kernel and for the combine"""
    assert ((1 << 24) - 1) * 256 < 1 << 32
