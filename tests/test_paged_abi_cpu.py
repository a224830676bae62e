"""C ABI and host side of the paged int8 KV cache (`lbfa_kvcache_paged_append`, `lbfa_decode_paged`, `PageAllocator`,
`LowbitPagedKVCache`): exported, declared, every host-visible argument refused BEFORE the first launch with LBFA_EINVAL and an
exact message, the page allocator on the host alone, and the front-end refusals that come before any device use - none of this
needs a GPU.  Tables in the style of tests/test_decode_abi_cpu.py."""
import os

import pytest

from cabi_calls import DEFAULTS, A, call, check_table, lib  # noqa: F401 (lib: the fixture)

# the default problems (cabi_calls.DEFAULTS): B 1, Hkv 2, D 64, T / Sq 8, 4 pages of 64 keys, 2 slots of up to 2 pages
NEW = ["lbfa_kvcache_paged_append", "lbfa_decode_paged"]
APP, DEC = NEW
APP_ALIGN = "lbfa_kvcache_paged_append: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens / block_table / slots 4-byte aligned"
DEC_ALIGN = "lbfa_decode_paged: cache tensors and km must be 16-byte aligned, k_scale / seqlens / block_table / slots / lse 4-byte aligned"


def test_new_symbols_are_exported_and_declared(lib):
    import ctypes
    from lowbit_quant_fa2_paddle_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lowbit_fa.h")).read()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert len(_lib.SIGNATURES[name][1]) == len(DEFAULTS[name]), name
    assert lib.lbfa_version() == 200  # additive: the version does not move


def _pool_rows(name):
    return [
        (name, dict(page_size=0), f"{name}: page_size must be a positive multiple of 64, got 0"),
        (name, dict(page_size=96), f"{name}: page_size must be a positive multiple of 64, got 96"),
        (name, dict(page_size=-64), f"{name}: page_size must be a positive multiple of 64, got -64"),
        (name, dict(num_pages=0), f"{name}: num_pages, num_slots and max_pages_per_seq must be at least 1, got 0, 2 and 2"),
        (name, dict(num_slots=0), f"{name}: num_pages, num_slots and max_pages_per_seq must be at least 1, got 4, 0 and 2"),
        (name, dict(max_pages_per_seq=0), f"{name}: num_pages, num_slots and max_pages_per_seq must be at least 1, got 4, 2 and 0"),
        (name, dict(max_pages_per_seq=1 << 26), f"{name}: max_pages_per_seq * page_size must stay below 2^31 keys"),
        (name, dict(B=3), f"{name}: B (3) exceeds num_slots (2)"),
    ]


SINGLE_FAULT = [
    (APP, dict(k_new=None), f"{APP}: null pointer"),
    (APP, dict(v_new=None), f"{APP}: null pointer"),
    (APP, dict(sk=None), f"{APP}: null pointer"),
    (APP, dict(k_codes=None), f"{APP}: null pointer"),
    (APP, dict(k_scale=None), f"{APP}: null pointer"),
    (APP, dict(v_cache=None), f"{APP}: null pointer"),
    (APP, dict(k_tail=None), f"{APP}: null pointer"),
    (APP, dict(seqlens=None), f"{APP}: null pointer"),
    (APP, dict(block_table=None), f"{APP}: null pointer"),
    (APP, dict(B=0), f"{APP}: empty tensor"),
    (APP, dict(T=0), f"{APP}: empty tensor"),
    (APP, dict(D=80), "Unsupported head_dim: 80"),
    *_pool_rows(APP),
    (APP, dict(dtype=7), "Input tensors must be in dtype of float16 or bfloat16"),
    (APP, dict(k_qmax=15), f"{APP}: k_qmax must be 127 (int8) or 7 (int4 range), got 15"),
    (APP, dict(k_new=A(2)), f"{APP}: k_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    (APP, dict(sv=(1024, 512, 60)), f"{APP}: v_new must be 16-byte aligned with strides that are multiples of 8 elements"),
    (APP, dict(k_codes=A(8)), APP_ALIGN),
    (APP, dict(v_cache=A(8)), APP_ALIGN),
    (APP, dict(k_tail=A(4)), APP_ALIGN),
    (APP, dict(km=A(4)), APP_ALIGN),
    (APP, dict(k_scale=A(2)), APP_ALIGN),
    (APP, dict(seqlens=A(1)), APP_ALIGN),
    (APP, dict(new_lens=A(2)), APP_ALIGN),
    (APP, dict(block_table=A(2)), APP_ALIGN),
    (APP, dict(slots=A(3)), APP_ALIGN),
    (APP, dict(Hkv=65536), f"{APP}: grid too large"),

    (DEC, dict(q=None), f"{DEC}: null pointer"),
    (DEC, dict(sq=None), f"{DEC}: null pointer"),
    (DEC, dict(o=None), f"{DEC}: null pointer"),
    (DEC, dict(k_codes=None), f"{DEC}: null pointer"),
    (DEC, dict(k_scale=None), f"{DEC}: null pointer"),
    (DEC, dict(v_cache=None), f"{DEC}: null pointer"),
    (DEC, dict(seqlens=None), f"{DEC}: null pointer"),
    (DEC, dict(block_table=None), f"{DEC}: null pointer"),
    (DEC, dict(workspace=None), f"{DEC}: null pointer"),
    (DEC, dict(Sq=0), f"{DEC}: empty tensor"),
    (DEC, dict(D=96), "Unsupported head_dim: 96"),
    (DEC, dict(Hq=3), "num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    (DEC, dict(Sq=33), f"{DEC}: Sq * (Hq / Hkv) = 66 query rows per kv head, the limit is 64 (longer queries belong on the dense operator)"),
    *_pool_rows(DEC),
    (DEC, dict(max_seqlen_k=129), f"{DEC}: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got 129 (limit 128)"),
    (DEC, dict(max_seqlen_k=0), f"{DEC}: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got 0 (limit 128)"),
    (DEC, dict(max_pages_per_seq=1), f"{DEC}: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got 128 (limit 64)"),
    (DEC, dict(num_splits=-1), f"{DEC}: num_splits must be in [0, 65535] (0: chosen by lbfa_decode_num_splits), got -1"),
    (DEC, dict(dtype=2), "Input tensors must be in dtype of float16 or bfloat16"),
    (DEC, dict(q_qmax=8), f"{DEC}: q_qmax must be 127 (int8) or 7 (int4 range), got 8"),
    (DEC, dict(sm_scale=0.0), f"{DEC}: sm_scale must be positive"),
    (DEC, dict(q=A(8)), f"{DEC}: q must be 16-byte aligned with strides that are multiples of 8 elements"),
    (DEC, dict(o=A(4)), f"{DEC}: o must be 8-byte aligned with strides that are multiples of 4 elements"),
    (DEC, dict(k_codes=A(8)), DEC_ALIGN),
    (DEC, dict(v_cache=A(8)), DEC_ALIGN),
    (DEC, dict(km=A(8)), DEC_ALIGN),
    (DEC, dict(k_scale=A(2)), DEC_ALIGN),
    (DEC, dict(seqlens=A(2)), DEC_ALIGN),
    (DEC, dict(block_table=A(1)), DEC_ALIGN),
    (DEC, dict(slots=A(2)), DEC_ALIGN),
    (DEC, dict(lse=A(2)), DEC_ALIGN),
    (DEC, dict(workspace_bytes=16), f"{DEC}: workspace too small (16 < 17408)"),
    (DEC, dict(workspace=A(8)), f"{DEC}: workspace must be 16-byte aligned"),
    (DEC, dict(B=65536, num_slots=65536, workspace_bytes=1 << 40), f"{DEC}: grid too large"),
]


def test_single_fault_table(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    check_table(lib, SINGLE_FAULT)
    with pytest.raises(ValueError, match="exceeds num_slots"):
        _lib.check(call(lib, DEC, B=3)[0], lib)


def test_paged_decode_reuses_the_split_rule_and_workspace(lib):
    # the default problem of the table: the byte count lbfa_decode's own table pins for the same B, Hq, Hkv, Sq, D and slices
    assert lib.lbfa_decode_workspace_bytes(1, 4, 2, 8, 64, 128, 2) == 17408


# ------------------------------------------------------------------------------------------------------------------------
# the allocator, on the host alone
# ------------------------------------------------------------------------------------------------------------------------
def _owned(a):
    return [p for pages in a.pages for p in pages]


def _consistent(a):
    """every page is either free or owned by exactly one slot, and each slot holds the pages its bound needs"""
    assert sorted(a.free_pages + _owned(a)) == list(range(a.num_pages))
    for pages, bound in zip(a.pages, a.bound):
        assert len(pages) == -(-bound // a.page_size)


def test_allocator_hands_pages_out_in_page_order():
    from lowbit_quant_fa2_paddle_amd import PageAllocator
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    a = PageAllocator(8, 128, 3, 4, page_order=order)
    assert a.num_free_pages == 8 and a.capacity == 512
    assert a.reserve([0, 2], 130) == [(0, 0, 5), (0, 1, 2), (2, 0, 7), (2, 1, 0)]   # two pages each, slot by slot
    _consistent(a)
    assert a.reserve([2, 0], 126) == []                                            # 256 rows still fit in two pages
    assert a.reserve([0], 1) == [(0, 2, 3)]                                        # row 257 opens the third
    assert a.reserve([1], 0) == [] and a.pages[1] == []
    assert a.bound == [257, 0, 256] and a.num_free_pages == 3
    _consistent(a)
    assert PageAllocator(3, 64, 1, 3).reserve([0], 129) == [(0, 0, 0), (0, 1, 1), (0, 2, 2)]  # the default order


def test_allocator_free_returns_exactly_what_the_slot_held():
    from lowbit_quant_fa2_paddle_amd import PageAllocator
    a = PageAllocator(6, 64, 3, 3, page_order=[4, 1, 5, 0, 2, 3])
    a.reserve([0, 1], 100)
    a.reserve([2], 1)
    assert a.pages == [[4, 1], [5, 0], [2]] and a.free_pages == [3]
    assert a.release(1) == [5, 0]
    assert a.pages == [[4, 1], [], [2]] and a.bound == [100, 0, 1] and a.free_pages == [3, 5, 0]
    _consistent(a)
    assert a.reserve([1], 192) == [(1, 0, 3), (1, 1, 5), (1, 2, 0)]  # the freed pages are used again
    _consistent(a)
    assert a.release(1) == [3, 5, 0] and a.release(1) == []


def test_allocator_exhaustion_and_capacity_leave_the_state_unchanged():
    import copy
    from lowbit_quant_fa2_paddle_amd import PageAllocator
    a = PageAllocator(4, 64, 3, 3)
    a.reserve([0, 1], 65)
    before = copy.deepcopy((a.free_pages, a.pages, a.bound))
    with pytest.raises(RuntimeError, match="out of pages"):
        a.reserve([2, 0], 64)  # slot 2 needs one page and slot 0 a third: none is free
    assert (a.free_pages, a.pages, a.bound) == before
    with pytest.raises(ValueError, match="capacity"):
        a.reserve([2, 0], 128)  # 65 + 128 > 3 * 64, found before slot 2 is given anything
    assert (a.free_pages, a.pages, a.bound) == before
    a.release(1)
    assert a.reserve([2], 128) == [(2, 0, 2), (2, 1, 3)]
    _consistent(a)


@pytest.mark.parametrize("order", [[0, 1, 1, 3], [0, 1, 2], [0, 1, 2, 4], [0, 1, 2, 3, 3], [-1, 0, 1, 2]])
def test_allocator_refuses_a_page_order_that_is_no_permutation(order):
    from lowbit_quant_fa2_paddle_amd import PageAllocator
    with pytest.raises(ValueError, match="permutation"):
        PageAllocator(4, 64, 2, 2, page_order=order)


def test_allocator_refuses_bad_sizes():
    from lowbit_quant_fa2_paddle_amd import PageAllocator
    with pytest.raises(ValueError, match="multiple of 64"):
        PageAllocator(4, 100, 2, 2)
    with pytest.raises(ValueError, match="at least 1"):
        PageAllocator(0, 64, 2, 2)


# ------------------------------------------------------------------------------------------------------------------------
# front-end refusals that come before any device use
# ------------------------------------------------------------------------------------------------------------------------
def test_front_end_refusals_before_any_device_use():
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.LowbitPagedKVCache(4, 64, 2, 64, 2, 2, torch.float16, "cpu")
    with pytest.raises(ValueError, match="permutation"):
        lb.LowbitPagedKVCache(4, 64, 2, 64, 2, 2, torch.float16, "cuda", page_order=[0, 0, 1, 2])
    with pytest.raises(ValueError, match="multiple of 64"):
        lb.LowbitPagedKVCache(4, 32, 2, 64, 2, 2, torch.float16, "cuda")
    paged = object.__new__(lb.LowbitPagedKVCache)  # no device needed: the slots are looked at first
    paged.max_seqs = 4
    kv = torch.zeros(2, 2, 8, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="distinct"):
        paged.append(kv, kv, slots=[1, 1])
    with pytest.raises(ValueError, match=r"in \[0, 4\)"):
        paged.append(kv, kv, slots=[1, 4])
    with pytest.raises(ValueError, match="one slot per row"):
        paged.append(kv, kv, slots=[1])
    with pytest.raises(ValueError, match="all 4 slots"):
        paged.append(kv, kv)
    q = torch.zeros(1, 2, 1, 64, dtype=torch.float16)
    dense = object.__new__(lb.LowbitKVCache)
    with pytest.raises(ValueError, match="slots address the sequences of a LowbitPagedKVCache"):
        lb.lowbit_fa_decode(q, dense, slots=[0])
    with pytest.raises(TypeError, match="LowbitKVCache or a LowbitPagedKVCache"):
        lb.lowbit_fa_decode(q, object())


def test_gather_returns_contiguous_tensors_at_one_block_per_page():
    """page_size 64: the scales of a page are one number per head, and a reshape of the gathered pages would be a strided view
    (no byte-wise comparison possible).  gather() promises contiguous tensors; checked on host tensors, no device needed."""
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    c = object.__new__(lb.LowbitPagedKVCache)
    c.allocator = lb.PageAllocator(8, 64, 3, 4, [5, 2, 7, 0, 3, 6, 1, 4])
    c.allocator.reserve([0], 150)
    c.device, c.num_kv_heads, c.padded_head_dim = torch.device("cpu"), 2, 64
    c.k_codes = torch.arange(8, dtype=torch.int8)[:, None, None, None].expand(8, 2, 64, 64).contiguous()
    c.k_scale = torch.arange(16, dtype=torch.float32).reshape(8, 2, 1)
    c.v = torch.full((8, 2, 64, 64), float("nan"), dtype=torch.float16)
    codes, scales, v = c.gather(0)
    assert codes.shape == (2, 192, 64) and scales.shape == (2, 3) and v.shape == (2, 192, 64)
    assert all(t.is_contiguous() for t in (codes, scales, v))
    assert scales.tolist() == [[10.0, 4.0, 14.0], [11.0, 5.0, 15.0]]  # pages 5, 2, 7 in the slot's order, per head
    assert codes[:, ::64, 0].tolist() == [[5, 2, 7], [5, 2, 7]]
    assert torch.equal(v.view(torch.uint8), v.clone().view(torch.uint8))
