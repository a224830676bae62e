"""Int8 KV cache, split-KV decode attention for short queries and cached prefill for any number of them (torch, forward only).

`LowbitKVCache` keeps K as the int8 codes and per-64-key scales the dense operators' K quantiser produces (bit for bit: a
prefill appended to an empty cache holds exactly the codes `lowbit_fa_qk_int8_pv_fp16_triton` would compute), V as fp16, and
is appended to in place (`lbfa_kvcache_append`).  `lowbit_fa_decode` attends a few new queries (Sq * Hq / Hkv <= 64 rows per kv
head) to the cache with one split-KV kernel (`lbfa_decode`): K and V are read once per GQA group, nothing is re-quantised.

`LowbitPagedKVCache` is the same cache as a pool of fixed-size pages behind one block table per sequence slot
(`lbfa_kvcache_paged_append`, `lbfa_decode_paged`): sequences of any length share the pool, a finished one gives its pages back,
and every sequence has a smooth-K mean of its own.  State and decode results equal the contiguous cache's bit for bit.

`lowbit_fa_prefill` attends ANY number of new queries to either cache (`lbfa_prefill`, `lbfa_prefill_paged`): chunked prefill of
a long prompt, the next turn over a cached prefix, a verify step of more than 64 rows.  Q is quantised in the kernel in the dense
operators' 128-row blocks, the causal mask is bottom-right aligned, query and key lengths are ragged device tensors.

`v_bits=8` (either cache; the default 16 changes nothing) keeps V as OCP e4m3fn codes with ONE fp32 scale per key and kv head
(`lbfa_*_v8`): the decode kernel then streams 2 D + 4 bytes per key instead of 3 D and the cache takes about two thirds of the
memory.  The quantiser of an appended row works on its Dp channels in fp32: `amax = max(max |x|, 1e-7)`, `scale = amax / 448`,
`code = e4m3fn_rne(x / scale)`; a row is written once and never re-quantised, so any append schedule gives the state of a one-shot
append bit for bit, and the K state is exactly that of a `v_bits=16` cache.  A reader sees `V^ = fp16_rne(fp32(decode(code)) *
scale)` (`dequantized_v()`), with `|V^ - V| <= (2^-4 + 2^-10) |V| + 2^-10 scale + 2^-24` per element, and a read equals, bit for
bit, the same read of a `v_bits=16` cache whose `v` holds V^.  `k_bits` and `v_bits` are independent.

`k_packed=True` (either cache, with `k_bits=4` only; the default False changes nothing) keeps the +-7 codes of `k_bits=4` two to a
byte (`lbfa_*_k4`, `lbfa_*_k4_v8`): `k_codes` is uint8 [.., keys, Dp / 2], byte j of a row holds channel 2 j in bits 0..3 and
channel 2 j + 1 in bits 4..7, each nibble the two's-complement 4-bit value of the code (never -8).  Without it `k_bits=4` costs
accuracy and buys nothing: the codes take a byte each.  Packed, the decode kernel streams 2.5 D bytes per key instead of 3 D (with
`v_bits=8`: 1.5 D + 4 instead of 2 D + 4) and the smallest cache takes about half the memory of the default one.  Scales, tail,
`km`, V and the re-quantisation of the open block are the byte cache's; a row is packed from its own codes, so any append schedule
still gives the one-shot state bit for bit, and a read equals, bit for bit, the same read of the byte-per-code `k_bits=4` cache
(an integer score does not depend on the order of its channels).  `unpacked_k_codes()` gives the int8 codes back.

Not here: prefix sharing / copy-on-write between sequences, fp8 P or an fp8 MFMA over the cache (V^ enters the fp16 MFMA), an
int4 MFMA or a packed Q (the nibbles are widened to the int8 MFMA's operands in registers), a backward through the cache, Paddle
tensors, routing `lowbit_fa_decode` calls with more than 64 rows to the prefill kernel (decode keeps refusing them).
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

from . import _lib
from . import quant_per_block as _qpb
from ._tensor import ops_for


def _padded_head_dim(d: int) -> int:
    if d > 128:
        raise ValueError(f"Unsupported head_dim: {d}")
    return 64 if d <= 64 else 128


def _append_operands(cache, k, v, tensor_layout: str):
    """The checks both caches make of the rows offered to `append`: -> ops, k, v (head dim zero-padded, last stride 1),
    (rows, heads, T) and the {batch, head, seq} strides of k and of v"""
    ops = ops_for(k)
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if k.dtype != cache.dtype or v.dtype != cache.dtype:
        raise ValueError("k and v must have the dtype of the cache")
    if k.device != cache.device or v.device != cache.device:
        raise ValueError("k and v must be on the device of the cache")
    if tuple(k.shape) != tuple(v.shape) or k.dim() != 4:
        raise ValueError("k and v must be 4-D tensors of the same shape")
    pad = cache.padded_head_dim - cache.head_dim
    if k.shape[-1] != cache.head_dim:
        raise ValueError(f"head_dim {k.shape[-1]} does not match the cache ({cache.head_dim})")
    if pad:  # only the new tokens are padded
        k, v = ops.pad_last(k, pad), ops.pad_last(v, pad)
    if k.stride(-1) != 1:
        k = k.contiguous()
    if v.stride(-1) != 1:
        v = v.contiguous()
    bht, k3 = _qpb._bhs(ops.shape(k), ops.strides(k), tensor_layout)
    _, v3 = _qpb._bhs(ops.shape(v), ops.strides(v), tensor_layout)
    return ops, k, v, bht, k3, v3


def _new_lens_i32(cache, ops, new_lens, n: int, per: str):
    """new_lens of an append of n rows as an int32 tensor on the cache's device (None stays None)"""
    if new_lens is not None:
        new_lens = new_lens.to(device=cache.device, dtype=ops.torch.int32).contiguous()
        if tuple(new_lens.shape) != (n,):
            raise ValueError(f"new_lens must have one entry per {per}")
    return new_lens


def _first_append_mean(lib, ops, k, k3, new_lens, km, B: int, H: int, T: int, D: int, stream):
    """smooth-K mean of the rows of a first append into km [B, H, D]: lbfa_mean_seq, the mean of the dense operators (the codes
    of a prefill are theirs), or lbfa_kvcache_mean over the first new_lens[b] rows of a ragged one"""
    code = ops.dtype_code(k)
    if new_lens is None:
        ws_bytes = lib.lbfa_mean_seq_workspace_bytes(B, H, T, D)
        ws = ops.torch.empty((max(ws_bytes, 16),), dtype=ops.torch.uint8, device=k.device)
        _lib.check(lib.lbfa_mean_seq(k.data_ptr(), code, km.data_ptr(), ws.data_ptr(), ws_bytes, B, H, T, D, _lib.strides3(k3),
                                     stream), lib)
    else:
        _lib.check(lib.lbfa_kvcache_mean(k.data_ptr(), code, new_lens.data_ptr(), km.data_ptr(), B, H, T, D, _lib.strides3(k3),
                                         stream), lib)


def _unpack_nibbles(packed):
    """uint8 [.., n] of two's-complement nibble pairs (low: even channel) -> int8 [.., 2 n]"""
    import torch
    w = packed.to(torch.int16)
    pair = torch.stack((w & 15, w >> 4), dim=-1)
    return (pair - 16 * (pair >> 3)).to(torch.int8).reshape(*packed.shape[:-1], 2 * packed.shape[-1])


class _CacheState:
    """What the two caches share: the checks of the formats, the state tensors behind a leading shape, and the argument list of
    an entry point."""

    v_bits = 16  # bits of a cached V element; 8 adds `v_scale`
    k_packed = False  # True: `k_codes` holds two 4-bit codes per byte

    def _check_formats(self, k_bits: int, v_bits: int, dtype, k_packed: bool = False):
        import torch
        if k_bits not in (8, 4):
            raise ValueError(f"k_bits must be 8 or 4, got {k_bits}")
        if v_bits not in (16, 8):
            raise ValueError(f"v_bits must be 16 or 8, got {v_bits}")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("dtype must be torch.float16 or torch.bfloat16")
        if k_packed and k_bits != 4:
            raise ValueError(f"k_packed=True needs k_bits=4 (the codes must fit a nibble), got k_bits={k_bits}")
        self.k_packed = bool(k_packed)
        self.v_bits, self.k_qmax = int(v_bits), 127 if k_bits == 8 else 7

    def _allocate(self, num_kv_heads: int, head_dim: int, dtype, device, smooth_k: bool, blocks: int, keys: int, seqs: int):
        """The state of `seqs` sequences whose keys lie in `blocks` runs of `keys` keys per kv head: one run per sequence
        (contiguous) or one per page"""
        import torch
        self.num_kv_heads, self.head_dim = int(num_kv_heads), int(head_dim)
        self.padded_head_dim = _padded_head_dim(self.head_dim)
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} lives on an AMD GPU (gfx950) only; there is no CPU fallback.")
        self.smooth_k = bool(smooth_k)
        H, D = self.num_kv_heads, self.padded_head_dim

        def zeros(shape, dt):
            return torch.zeros(shape, dtype=dt, device=self.device)
        self.k_codes = zeros((blocks, H, keys, D // 2), torch.uint8) if self.k_packed else zeros((blocks, H, keys, D), torch.int8)
        self.k_scale = zeros((blocks, H, keys // _lib.BLKK), torch.float32)
        self.v = zeros((blocks, H, keys, D), torch.uint8 if self.v_bits == 8 else torch.float16)
        if self.v_bits == 8:
            self.v_scale = zeros((blocks, H, keys), torch.float32)
        self.k_tail = zeros((seqs, H, _lib.BLKK, D), dtype)
        self.km = zeros((seqs, H, D), dtype) if self.smooth_k else None
        self.seqlens = zeros((seqs,), torch.int32)

    def dequantized_v(self):
        """Debugging aid (torch ops, read-only): fp16, the shape of `v` with the last dim cut to head_dim: the V the kernels read -
        with `v_bits=8` V^ = fp16(fp32(code) * scale), else `v` itself.  Rows no sequence holds (contiguous cache: at or past
        seqlens[b]) are meaningless."""
        import torch
        v = self.v
        if self.v_bits == 8:
            v = (v.view(torch.float8_e4m3fn).float() * self.v_scale[..., None]).to(torch.float16)
        return v[..., :self.head_dim]

    def unpacked_k_codes(self):
        """Debugging aid (torch ops, read-only): the K codes as int8 in the shape of the byte-per-code cache, [.., keys, Dp] -
        `k_codes` itself unless `k_packed`.  Rows no sequence holds are meaningless."""
        return _unpack_nibbles(self.k_codes) if self.k_packed else self.k_codes

    def _call(self, lib, name: str, head, mid, dims, tail, slot_t=None):
        """Calls entry point `name` (+ "_k4" over a packed K cache, + "_v8" over an fp8 V cache) with the argument list of include/lowbit_fa.h, put together from
        its named pieces:  head (.. v_cache), [v_scale], mid (.. seqlens[, q_lens]), [block_table, slots], dims (.. D),
        capacity | num_slots .. max_pages_per_seq, tail (.. stream)"""
        v8 = self.v_bits == 8
        if isinstance(self, LowbitPagedKVCache):
            table = (self.block_table.data_ptr(), slot_t.data_ptr() if slot_t is not None else None)
            extent = (self.max_seqs, self.num_pages, self.page_size, self.max_pages_per_seq)
        else:
            table, extent = (), (self.capacity,)
        entry = getattr(lib, name + ("_k4" if self.k_packed else "") + ("_v8" if v8 else ""))
        _lib.check(entry(*head, *((self.v_scale.data_ptr(),) if v8 else ()), *mid, *table, *dims, *extent, *tail), lib)

    def _append_rows(self, lib, name: str, ops, k, v, new_lens, n: int, H: int, T: int, k3, v3, stream, slot_t=None):
        """the append entry point `name` for n rows of T new keys"""
        self._call(lib, name,
                   (k.data_ptr(), v.data_ptr(), ops.dtype_code(k), new_lens.data_ptr() if new_lens is not None else None,
                    self.km.data_ptr() if self.smooth_k else None, self.k_codes.data_ptr(), self.k_scale.data_ptr(), self.v.data_ptr()),
                   (self.k_tail.data_ptr(), self.seqlens.data_ptr()), (n, H, T, self.padded_head_dim),
                   (_lib.strides3(k3), _lib.strides3(v3), self.k_qmax, stream), slot_t)


class LowbitKVCache(_CacheState):
    """Pre-allocated cache of `batch` sequences of up to `capacity` keys (rounded up to a multiple of 64).

    State (all on `device`): k_codes int8 [B, Hkv, cap, Dp], k_scale fp32 [B, Hkv, cap / 64], v fp16 [B, Hkv, cap, Dp],
    k_tail [B, Hkv, 64, Dp] (raw rows of the open 64-key block), km [B, Hkv, Dp] or None, seqlens int32 [B]; Dp = head_dim
    zero-padded to 64 / 128.  `km`, the smooth-K mean, is taken from the FIRST append and fixed from then on.
    With `v_bits=8`, v is uint8 [B, Hkv, cap, Dp] (e4m3fn bit patterns) and v_scale fp32 [B, Hkv, cap] holds the scale of each row
    (module docstring); with the default 16 there is no v_scale.  With `k_packed=True` (needs `k_bits=4`), k_codes is uint8
    [B, Hkv, cap, Dp / 2], two codes per byte (module docstring).
    No host read of `seqlens` happens anywhere: the host only tracks an upper bound of the lengths (the rows offered so far)."""

    def __init__(self, batch: int, num_kv_heads: int, head_dim: int, capacity: int, dtype, device, k_bits: int = 8,
                 smooth_k: bool = True, v_bits: int = 16, k_packed: bool = False):
        self._check_formats(k_bits, v_bits, dtype, k_packed)
        if batch <= 0 or num_kv_heads <= 0 or capacity <= 0:
            raise ValueError("batch, num_kv_heads and capacity must be positive")
        self.batch = int(batch)
        self.capacity = (int(capacity) + _lib.BLKK - 1) // _lib.BLKK * _lib.BLKK
        self._allocate(num_kv_heads, head_dim, dtype, device, smooth_k, self.batch, self.capacity, self.batch)
        self.max_seqlen = 0  # host upper bound of seqlens
        self._has_km = False

    def append(self, k, v, tensor_layout: str = "HND", new_lens=None):
        """Append k, v [B, Hkv, T, D] ("HND") or [B, T, Hkv, D] ("NHD"); sequence b takes the first new_lens[b] rows (an int32
        device tensor [B], None: all T).  Returns self."""
        ops, k, v, (B, H, T), k3, v3 = _append_operands(self, k, v, tensor_layout)
        torch = ops.torch
        if B != self.batch or H != self.num_kv_heads:
            raise ValueError(f"expected batch {self.batch} and {self.num_kv_heads} kv heads, got {B} and {H}")
        if T == 0:
            return self
        if self.max_seqlen + T > self.capacity:
            raise ValueError(f"appending {T} tokens to at most {self.max_seqlen} would pass the capacity {self.capacity}")
        new_lens = _new_lens_i32(self, ops, new_lens, self.batch, "sequence")
        lib = _lib.load()
        with ops.device_guard(k):
            stream = ops.stream(k)
            if self.smooth_k and not self._has_km:
                _first_append_mean(lib, ops, k, k3, new_lens, self.km, B, H, T, self.padded_head_dim, stream)
                self._has_km = True
            self._append_rows(lib, "lbfa_kvcache_append", ops, k, v, new_lens, B, H, T, k3, v3, stream)
            # the kernel reads seqlens and does not advance it
            if new_lens is None:
                self.seqlens += T
            else:
                self.seqlens += torch.clamp(new_lens, 0, T)
        self.max_seqlen += T
        return self

    def dequantized_k(self):
        """Debugging aid (torch ops, read-only): fp32 [B, Hkv, capacity, head_dim] = codes * scale (+ km).  Rows at or past
        seqlens[b] are meaningless."""
        k = self.unpacked_k_codes().float() * self.k_scale.repeat_interleave(_lib.BLKK, dim=2)[..., None]
        if self.km is not None:
            k = k + self.km.float()[:, :, None, :]
        return k[..., :self.head_dim]


class PageAllocator:
    """Host side of a paged cache, pure Python (no device, no tensors): a free list of page ids, the pages each sequence slot
    holds in order, and per slot an upper bound of the rows offered so far.  Pages are handed out from the front of the free
    list (initially `page_order`, a permutation of range(num_pages), or range(num_pages)) and come back at its end."""

    def __init__(self, num_pages: int, page_size: int, max_seqs: int, max_pages_per_seq: int,
                 page_order: Optional[Iterable[int]] = None):
        if num_pages < 1 or max_seqs < 1 or max_pages_per_seq < 1:
            raise ValueError("num_pages, max_seqs and max_pages_per_seq must be at least 1")
        if page_size < 1 or page_size % _lib.BLKK:
            raise ValueError(f"page_size must be a positive multiple of {_lib.BLKK}, got {page_size}")
        order = list(range(num_pages)) if page_order is None else [int(x) for x in page_order]
        if sorted(order) != list(range(num_pages)):
            raise ValueError("page_order must be a permutation of range(num_pages)")
        self.num_pages, self.page_size = int(num_pages), int(page_size)
        self.max_seqs, self.max_pages_per_seq = int(max_seqs), int(max_pages_per_seq)
        self.free_pages = order
        self.pages = [[] for _ in range(self.max_seqs)]   # pages of each slot, in sequence order
        self.bound = [0] * self.max_seqs                  # rows offered to each slot: an upper bound of its length

    @property
    def capacity(self) -> int:
        return self.max_pages_per_seq * self.page_size

    @property
    def num_free_pages(self) -> int:
        return len(self.free_pages)

    def reserve(self, slots: Sequence[int], T: int):
        """Make room for T more rows in each of `slots`: -> [(slot, index in the slot's table, page)] of the new table entries.
        All or nothing: ValueError (a slot would pass the capacity) or RuntimeError (out of pages) leave everything as it was."""
        need = []
        for s in slots:
            if self.bound[s] + T > self.capacity:
                raise ValueError(f"appending {T} tokens to at most {self.bound[s]} in slot {s} would pass the capacity "
                                 f"{self.capacity} (max_pages_per_seq * page_size)")
            need.append(-(-(self.bound[s] + T) // self.page_size) - len(self.pages[s]))
        if sum(need) > len(self.free_pages):
            raise RuntimeError(f"out of pages: the append needs {sum(need)} more, {len(self.free_pages)} are free")
        changed = []
        for s, k in zip(slots, need):
            for _ in range(k):
                page = self.free_pages.pop(0)
                changed.append((s, len(self.pages[s]), page))
                self.pages[s].append(page)
            self.bound[s] += T
        return changed

    def release(self, slot: int):
        """Give the pages of `slot` back (in the order it held them) and make it fresh: -> those pages"""
        pages, self.pages[slot], self.bound[slot] = self.pages[slot], [], 0
        self.free_pages.extend(pages)
        return pages


def _slot_list(slots, n: int, max_seqs: int):
    """the slots of a call with n rows: distinct ints in [0, max_seqs); None: all slots in order"""
    if slots is None:
        if n != max_seqs:
            raise ValueError(f"slots=None addresses all {max_seqs} slots, got {n} rows")
        return list(range(max_seqs))
    slots = [int(x) for x in slots]
    if len(slots) != n:
        raise ValueError(f"expected one slot per row ({n}), got {len(slots)}")
    if len(set(slots)) != len(slots):
        raise ValueError(f"slots must be distinct, got {slots}")
    if any(x < 0 or x >= max_seqs for x in slots):
        raise ValueError(f"slots must be in [0, {max_seqs}), got {slots}")
    return slots


class LowbitPagedKVCache(_CacheState):
    """The int8 KV cache as a pool of `num_pages` pages of `page_size` keys (a multiple of 64) shared by up to `max_seqs`
    sequences, each in a slot with a block table of up to `max_pages_per_seq` pages.

    State (public, all on `device`; the layout `lbfa_kvcache_paged_append` / `lbfa_decode_paged` take): k_codes int8
    [num_pages, Hkv, page_size, Dp], k_scale fp32 [num_pages, Hkv, page_size / 64], v fp16 [num_pages, Hkv, page_size, Dp],
    block_table int32 [max_seqs, max_pages_per_seq], k_tail [max_seqs, Hkv, 64, Dp], km [max_seqs, Hkv, Dp] or None, seqlens int32
    [max_seqs].  With `v_bits=8`, v is uint8 [num_pages, Hkv, page_size, Dp] (e4m3fn bit patterns) and v_scale fp32 [num_pages, Hkv,
    page_size] holds the scale of each row, addressed by the same page and row as the codes.  With `k_packed=True` (needs
    `k_bits=4`), k_codes is uint8 [num_pages, Hkv, page_size, Dp / 2], two codes per byte, a 64-key tile 32 Dp contiguous bytes
    inside its page.  `allocator` (a `PageAllocator`) is the host side.  `km` is PER SEQUENCE: a slot that holds nothing is fresh, and
    takes its mean from its first append.  As in `LowbitKVCache` no host read of device lengths happens anywhere: pages are
    allocated for the upper bound of each length."""

    def __init__(self, num_pages: int, page_size: int, num_kv_heads: int, head_dim: int, max_seqs: int, max_pages_per_seq: int,
                 dtype, device, k_bits: int = 8, smooth_k: bool = True, page_order: Optional[Iterable[int]] = None,
                 v_bits: int = 16, k_packed: bool = False):
        import torch
        self._check_formats(k_bits, v_bits, dtype, k_packed)
        if num_kv_heads <= 0:
            raise ValueError("num_kv_heads must be positive")
        self.allocator = PageAllocator(num_pages, page_size, max_seqs, max_pages_per_seq, page_order)
        self.num_pages, self.page_size = self.allocator.num_pages, self.allocator.page_size
        self.max_seqs, self.max_pages_per_seq = self.allocator.max_seqs, self.allocator.max_pages_per_seq
        self._allocate(num_kv_heads, head_dim, dtype, device, smooth_k, self.num_pages, self.page_size, self.max_seqs)
        self.block_table = torch.zeros((self.max_seqs, self.max_pages_per_seq), dtype=torch.int32, device=self.device)

    @property
    def num_free_pages(self) -> int:
        return self.allocator.num_free_pages

    def append(self, k, v, slots=None, tensor_layout: str = "HND", new_lens=None):
        """Append k, v [n, Hkv, T, D] ("HND") or [n, T, Hkv, D] ("NHD") to the sequences in `slots` (n distinct ints; None: all
        max_seqs slots in order); row b takes the first new_lens[b] rows (an int32 device tensor [n], None: all T).  Pages for
        T more rows per slot are taken before the launch: RuntimeError ("out of pages") or ValueError (a slot would pass
        max_pages_per_seq * page_size) leave the cache as it was.  Returns self."""
        slots_given = slots is not None
        slots = _slot_list(slots, int(k.shape[0]), self.max_seqs)
        ops, k, v, (n, H, T), k3, v3 = _append_operands(self, k, v, tensor_layout)
        torch = ops.torch
        if H != self.num_kv_heads:
            raise ValueError(f"expected {self.num_kv_heads} kv heads, got {H}")
        if T == 0:
            return self
        new_lens = _new_lens_i32(self, ops, new_lens, n, "row")
        fresh = [i for i, s in enumerate(slots) if self.allocator.bound[s] == 0]  # rows whose sequence starts here
        changed = self.allocator.reserve(slots, T)  # raises with nothing changed
        lib = _lib.load()
        D = self.padded_head_dim
        with ops.device_guard(k):
            stream = ops.stream(k)
            if changed:  # only the new table entries travel
                flat = torch.tensor([s * self.max_pages_per_seq + i for s, i, _ in changed], dtype=torch.int64, device=self.device)
                self.block_table.view(-1).index_copy_(0, flat, torch.tensor([pg for _, _, pg in changed], dtype=torch.int32,
                                                                           device=self.device))
            slot_t = torch.tensor(slots, dtype=torch.int32, device=self.device) if slots_given else None
            if self.smooth_k and fresh:
                km_new = torch.empty((n, H, D), dtype=self.dtype, device=self.device)
                _first_append_mean(lib, ops, k, k3, new_lens, km_new, n, H, T, D, stream)
                rows = torch.tensor(fresh, dtype=torch.int64, device=self.device)
                self.km.index_copy_(0, torch.tensor([slots[i] for i in fresh], dtype=torch.int64, device=self.device), km_new[rows])
            self._append_rows(lib, "lbfa_kvcache_paged_append", ops, k, v, new_lens, n, H, T, k3, v3, stream, slot_t)
            # the kernel reads seqlens and does not advance it
            add = torch.full((n,), T, dtype=torch.int32, device=self.device) if new_lens is None else torch.clamp(new_lens, 0, T)
            if slot_t is None:
                self.seqlens += add
            else:
                self.seqlens.index_add_(0, slot_t.long(), add)
        return self

    def free(self, slots):
        """Give the pages of `slots` (an int or distinct ints) back to the pool; the slots are fresh again.  Returns self."""
        import torch
        slots = [slots] if isinstance(slots, int) else list(slots)
        slots = _slot_list(slots, len(slots), self.max_seqs)
        for s in slots:
            self.allocator.release(s)
        if slots:
            self.seqlens.index_fill_(0, torch.tensor(slots, dtype=torch.int64, device=self.device), 0)
        return self

    def max_seqlen(self, slots=None) -> int:
        """host upper bound of the lengths of `slots` (None: all)"""
        return max(self.allocator.bound[s] for s in (range(self.max_seqs) if slots is None else slots))

    def gather(self, slot: int):
        """Debugging aid (torch ops, read-only): the sequence in `slot` through its block table as contiguous tensors - codes
        int8 [Hkv, n, Dp], scales fp32 [Hkv, n / 64], V fp16 [Hkv, n, Dp], n = its pages * page_size; with `v_bits=8` V is the
        uint8 codes and a fourth tensor follows, their scales fp32 [Hkv, n]; with `k_packed` the codes are the packed bytes, uint8
        [Hkv, n, Dp / 2].  Rows at or past seqlens[slot] are meaningless."""
        import torch
        idx = torch.tensor(self.allocator.pages[slot], dtype=torch.int64, device=self.device)
        H, D = self.num_kv_heads, self.padded_head_dim
        # (contiguous() : with one 64-key block per page the reshape of the scales is a strided view)
        out = (self.k_codes[idx].transpose(0, 1).reshape(H, -1, self.k_codes.shape[-1]).contiguous(),
               self.k_scale[idx].transpose(0, 1).reshape(H, -1).contiguous(),
               self.v[idx].transpose(0, 1).reshape(H, -1, D).contiguous())
        if self.v_bits == 8:
            out += (self.v_scale[idx].transpose(0, 1).reshape(H, -1).contiguous(),)
        return out


def _attend(who: str, q, cache, tensor_layout, is_causal, sm_scale, return_lse, num_splits, q_bits, slots, q_lens, prefill: bool):
    """What `lowbit_fa_decode` and `lowbit_fa_prefill` share: the checks, the padding, the workspace and the pieces of the
    argument list (`_CacheState._call`).  `prefill` picks lbfa_prefill[_paged] (any Sq, `q_lens`) over lbfa_decode[_paged]."""
    ops = ops_for(q)
    if ops.name != "torch":
        raise TypeError(f"{who} takes torch tensors")
    torch = ops.torch
    paged = isinstance(cache, LowbitPagedKVCache)
    if not paged and not isinstance(cache, LowbitKVCache):
        raise TypeError("cache must be a LowbitKVCache or a LowbitPagedKVCache")
    if slots is not None and not paged:
        raise ValueError("slots address the sequences of a LowbitPagedKVCache; a LowbitKVCache is decoded as a whole batch")
    if torch.is_grad_enabled() and q.requires_grad:
        raise RuntimeError(f"{who} is forward-only: there is no backward through the KV cache "
                           "(call it under torch.no_grad() or detach q)")
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if q_bits not in (8, 4):
        raise ValueError(f"q_bits must be 8 or 4, got {q_bits}")
    if q.dtype != cache.dtype:
        raise ValueError("q must have the dtype of the cache")
    if q.device != cache.device:
        raise ValueError("q must be on the device of the cache")
    if q.dim() != 4 or q.shape[-1] != cache.head_dim:
        raise ValueError(f"q must be 4-D with head_dim {cache.head_dim}")
    head_dim_og = cache.head_dim
    if sm_scale is None:
        sm_scale = 1.0 / head_dim_og ** 0.5
    pad = cache.padded_head_dim - head_dim_og
    if pad:
        q = ops.pad_last(q, pad)
    if q.stride(-1) != 1:
        q = q.contiguous()
    qshape = ops.shape(q)
    (B, Hq, Sq), q3 = _qpb._bhs(qshape, ops.strides(q), tensor_layout)
    if paged:
        slot_list = _slot_list(slots, B, cache.max_seqs)
    elif B != cache.batch:
        raise ValueError(f"expected batch {cache.batch}, got {B}")
    if q_lens is not None:
        try:  # a tensor, or anything torch.as_tensor takes (a list, a numpy array)
            q_lens = torch.as_tensor(q_lens).to(device=cache.device, dtype=torch.int32).contiguous()
        except (TypeError, ValueError, RuntimeError) as e:
            raise TypeError(f"q_lens must be an integer tensor or sequence with one entry per row of q: {e}") from e
        if tuple(q_lens.shape) != (B,):
            raise ValueError("q_lens must have one entry per row of q")
    o = ops.empty(qshape, q.dtype, q)
    (_, _, _), o3 = _qpb._bhs(qshape, ops.strides(o), tensor_layout)
    lse = ops.empty((B, Hq, Sq), ops.float32, q) if return_lse else None
    if 0 in qshape:
        return (o[..., :head_dim_og], lse) if return_lse else o[..., :head_dim_og]
    lib = _lib.load()
    Hkv, D = cache.num_kv_heads, cache.padded_head_dim
    max_k = max(1, min(cache.max_seqlen(slot_list), cache.allocator.capacity) if paged else min(cache.max_seqlen, cache.capacity))
    workspace_bytes = lib.lbfa_prefill_workspace_bytes if prefill else lib.lbfa_decode_workspace_bytes
    ws_bytes = workspace_bytes(B, Hq, Hkv, Sq, D, max_k, int(num_splits))
    ws = ops.empty((max(ws_bytes, 16),), ops.uint8, q)
    with ops.device_guard(q):
        mid = (cache.km.data_ptr() if cache.km is not None else None, cache.seqlens.data_ptr())
        if prefill:
            mid += (q_lens.data_ptr() if q_lens is not None else None,)
        slot_t = torch.tensor(slot_list, dtype=torch.int32, device=cache.device) if slots is not None else None
        cache._call(lib, ("lbfa_prefill" if prefill else "lbfa_decode") + ("_paged" if paged else ""),
                    (q.data_ptr(), ops.dtype_code(q), cache.k_codes.data_ptr(), cache.k_scale.data_ptr(), cache.v.data_ptr()), mid,
                    (o.data_ptr(), lse.data_ptr() if return_lse else None, ws.data_ptr(), ws_bytes, B, Hq, Hkv, Sq, D),
                    (max_k, int(num_splits), _lib.strides3(q3), _lib.strides3(o3), float(sm_scale), 127 if q_bits == 8 else 7,
                     1 if is_causal else 0, ops.stream(q)), slot_t)
    o = o[..., :head_dim_og]
    return (o, lse) if return_lse else o


def lowbit_fa_decode(q, cache, tensor_layout: str = "HND", is_causal: bool = False,
                     sm_scale: Optional[float] = None, return_lse: bool = False, num_splits: int = 0, q_bits: int = 8,
                     slots=None):
    """Attention of the new queries q [B, Hq, Sq, D] ("HND") or [B, Sq, Hq, D] ("NHD") to everything in `cache` (the keys of
    these queries appended first).  Sq * (Hq / Hkv) <= 64.  `is_causal`: bottom-right aligned, query i sees keys
    < seqlens[b] - Sq + 1 + i.  `num_splits`: key slices (0: chosen by `lbfa_decode_num_splits`); results are bitwise
    reproducible for a given value.  Returns o (shape and dtype of q) and, with `return_lse`, the natural-log LSE [B, Hq, Sq]
    fp32.  A sequence with no keys gets zeros and -inf.  Forward only.
    `cache` is a `LowbitKVCache` or a `LowbitPagedKVCache`; with a paged one row b of q attends to the sequence in
    `slots[b]` (distinct ints; None: all slots in order)."""
    return _attend("lowbit_fa_decode", q, cache, tensor_layout, is_causal, sm_scale, return_lse, num_splits, q_bits, slots, None,
                   False)


def lowbit_fa_prefill(q, cache, tensor_layout: str = "HND", is_causal: bool = False,
                      sm_scale: Optional[float] = None, return_lse: bool = False, num_splits: int = 0, q_bits: int = 8,
                      slots=None, q_lens=None):
    """Cached prefill: attention of ANY number of new queries q [B, Hq, Sq, D] ("HND") or [B, Sq, Hq, D] ("NHD") to everything in
    `cache` (the keys of these queries appended first) - a chunk of a long prompt, the next turn of a conversation, a
    speculative-decoding verify step.  For Sq * (Hq / Hkv) <= 64 call `lowbit_fa_decode`.

    `q_lens`: int32 tensor [B] or None (all Sq) - sequence b owns the first q_lens[b] rows of q[b] (clamped to [0, Sq] on the
    device), the counterpart of `append(..., new_lens=)`; rows at or past it come back as zeros with LSE -inf, and the result
    for sequence b equals the call on q[b, :, :q_lens[b]] alone.  Keys at or past `cache.seqlens[b]` are masked.
    Q is quantised inside the kernel in blocks of 128 rows from row 0 of each (batch, head), the last block cut at q_lens[b]:
    codes and scales are those of the dense operators' Q quantiser on the valid rows (`q_bits` 8 or 4), so a cache filled by one
    uniform append and read with Sq == Sk sees exactly the dense operator's Q and K codes.  The arithmetic is the decode kernel's:
    int8 scores x q_scale x k_scale, base-2 online softmax, P rounded to fp16, fp16 MFMA against V, fp32 accumulation.
    `is_causal`: bottom-right aligned, query i of sequence b sees keys < seqlens[b] - q_lens[b] + 1 + i; a query that sees no
    key gives zeros and -inf.  `num_splits`: key slices over the tiles a Q block can see (0: chosen by
    `lbfa_prefill_num_splits`); results are bitwise reproducible for a given value, and equal between a `LowbitKVCache` and a
    `LowbitPagedKVCache` (`slots` as in `lowbit_fa_decode`).  Returns o (shape and dtype of q) and, with `return_lse`, the
    natural-log LSE [B, Hq, Sq] fp32 including the smooth-K correction.  Forward only, torch tensors only."""
    return _attend("lowbit_fa_prefill", q, cache, tensor_layout, is_causal, sm_scale, return_lse, num_splits, q_bits, slots,
                   q_lens, True)


sageattn_decode = lowbit_fa_decode
sageattn_prefill = lowbit_fa_prefill
