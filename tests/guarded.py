"""Guard bands and hostile memory for the containment tests (test infrastructure, pure torch, works on CPU tensors).

The value tests compare what a kernel was supposed to produce.  These helpers look at everything else:

* `GuardArena` - for the duration of a `with` block every `torch.empty` on the test's device is carved, contiguous and 256-byte
  aligned, out of the middle of a larger uint8 buffer full of a sentinel byte, at least 128 KiB of it on either side (more than
  one 128-row x 128-channel fp32 tile, the largest unit any kernel here writes at once).  Every front-end module reaches
  `torch.empty` by attribute at call time, so the one patch covers outputs, workspaces and the backward's gradient buffers.
  `arena.check()` asserts that every guard byte still holds the sentinel and names the allocation and the touched offsets.
* `hostile_view` - an operand with the values of `t` inside a larger buffer whose other elements are NaN / -128 / +inf: before
  row 0, after the last row, between heads and batches, and in the channels past D of every row.
* `guarded_out` - an output view with gaps (doubled strides, 80 channels in 128-channel rows) inside a sentinel buffer, and a
  `check()` that asserts every byte outside the view is untouched.

A stray store of the sentinel byte itself is not seen; 0xA5 is no byte of a zero, of a small integer or of a common float.
tests/test_guarded_cpu.py tests all of this on CPU tensors with fake kernels.
"""
import math

import torch

SENTINEL = 0xA5
GUARD_BYTES = 128 * 1024
ALIGN = 256


def _itemsize(dtype):
    return torch.tensor([], dtype=dtype).element_size()  # (not torch.empty: that name is what the arena patches)


def _touched(buf, keep_mask, sentinel):
    """offsets (int64, sorted) of the bytes of the uint8 `buf` outside `keep_mask` that no longer hold the sentinel"""
    bad = buf != sentinel
    bad &= ~keep_mask
    return torch.nonzero(bad).flatten()


class GuardArena:
    """Context manager: `with GuardArena(monkeypatch, device) as arena: out = op(...)`, then `arena.check()`.

    Only the operator call (and `torch.autograd.grad` for a backward) belongs inside the block: every tensor `torch.empty` makes
    on `device` in there is guarded, whoever asks.  Allocations on other devices, and calls with options the front end never
    uses (`out=`, `pin_memory=`, a memory format, a layout), go to the real `torch.empty`."""

    def __init__(self, monkeypatch, device, guard_bytes=GUARD_BYTES, sentinel=SENTINEL):
        assert guard_bytes >= GUARD_BYTES, "the guard must cover the largest tile a kernel writes at once"
        self.monkeypatch, self.device = monkeypatch, torch.device(device)
        self.guard_bytes, self.sentinel = int(guard_bytes), int(sentinel)
        self.allocations = []  # dicts: order, shape, dtype, nbytes, offset (of the allocation in `buf`), buf, tensor
        self._real = None

    # ---- the patch ---------------------------------------------------------------------------------------------------------
    def __enter__(self):
        assert self._real is None, "GuardArena is not re-entrant"
        self._real = torch.empty
        self.monkeypatch.setattr(torch, "empty", self._empty)
        return self

    def __exit__(self, *exc):
        self.monkeypatch.setattr(torch, "empty", self._real)
        self._real = None
        return False

    def _same_device(self, device):
        d = torch.device(device) if device is not None else torch.device("cpu")
        if d.type != self.device.type:
            return False
        return d.index is None or self.device.index is None or d.index == self.device.index

    def _empty(self, *size, dtype=None, device=None, **kwargs):
        real = self._real
        plain = all(v is None or v is False for v in kwargs.values())
        if not plain or not self._same_device(device):
            return real(*size, dtype=dtype, device=device, **kwargs)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(int(s) for s in size)
        return self.allocate(shape, dtype if dtype is not None else torch.get_default_dtype(), _alloc=real)

    def allocate(self, shape, dtype, _alloc=None):
        """a guarded tensor of `shape` and `dtype` on the arena's device (also usable directly, outside the block)"""
        alloc = _alloc or self._real or torch.empty
        shape = tuple(int(s) for s in shape)
        nbytes = math.prod(shape) * _itemsize(dtype)
        if nbytes == 0:
            return alloc(shape, dtype=dtype, device=self.device)
        total = self.guard_bytes + ALIGN + (nbytes + ALIGN - 1) // ALIGN * ALIGN + self.guard_bytes
        buf = alloc((total,), dtype=torch.uint8, device=self.device)
        buf.fill_(self.sentinel)
        offset = self.guard_bytes + (-(buf.data_ptr() + self.guard_bytes)) % ALIGN
        t = buf[offset:offset + nbytes].view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == 0 and t.is_contiguous()
        assert offset >= self.guard_bytes and total - offset - nbytes >= self.guard_bytes
        self.allocations.append(dict(order=len(self.allocations), shape=shape, dtype=dtype, nbytes=nbytes, offset=offset, buf=buf,
                                     tensor=t))
        return t

    def like(self, t, fill=None):
        """a guarded tensor with the shape, dtype and (unless `fill` is given) the contents of the contiguous tensor `t`"""
        g = self.allocate(tuple(t.shape), t.dtype)
        if fill is None:
            g.copy_(t)
        else:
            g.fill_(fill)
        return g

    # ---- the check ---------------------------------------------------------------------------------------------------------
    def violations(self):
        """-> one dict per allocation whose guards were touched: order, shape, dtype, nbytes, first, last, count.  `first` and
        `last` are byte offsets relative to the allocation's first byte: negative before it, >= nbytes behind it."""
        out = []
        for a in self.allocations:
            keep = torch.zeros(a["buf"].shape, dtype=torch.bool, device=a["buf"].device)
            keep[a["offset"]:a["offset"] + a["nbytes"]] = True
            idx = _touched(a["buf"], keep, self.sentinel)
            if idx.numel():
                out.append(dict(order=a["order"], shape=a["shape"], dtype=a["dtype"], nbytes=a["nbytes"],
                                first=int(idx[0]) - a["offset"], last=int(idx[-1]) - a["offset"], count=int(idx.numel())))
        return out

    def check(self):
        bad = self.violations()
        assert not bad, "guard bytes were written: " + "; ".join(
            f"allocation #{v['order']} {v['shape']} {v['dtype']} ({v['nbytes']} bytes): {v['count']} guard bytes touched, "
            f"first at byte offset {v['first']}, last at {v['last']} relative to the allocation" for v in bad)

    def __len__(self):
        return len(self.allocations)


def hostile_fill(dtype, scale=False):
    """what surrounds an operand: NaN for 16-bit and fp32 data, -128 for int8 codes (outside both code ranges), +inf for scales"""
    if dtype == torch.int8:
        return -128
    return float("inf") if scale else float("nan")


def hostile_view(t, *, before, after, fill=None, check_abi=True):
    """A view with the shape and values of `t` inside a larger buffer of `fill`.  `before` / `after`: padding per dimension, the
    last one included (a D = 80 view in 128-channel rows: after[-1] = 48).  With `check_abi` the view keeps what the C ABI asks of
    an operand: last stride 1, a 16-byte aligned base, every other stride a multiple of 8 elements."""
    before, after = tuple(int(x) for x in before), tuple(int(x) for x in after)
    assert len(before) == len(after) == t.dim(), "one padding per dimension"
    if fill is None:
        fill = hostile_fill(t.dtype)
    full = tuple(b + s + a for b, s, a in zip(before, t.shape, after))
    buf = torch.full(full, fill, dtype=t.dtype, device=t.device)
    view = buf[tuple(slice(b, b + s) for b, s in zip(before, t.shape))]
    view.copy_(t)
    if check_abi:
        if view.stride(-1) != 1 or view.data_ptr() % 16 or any(s % 8 for s in view.stride()[:-1]):
            raise ValueError(f"padding {before} / {after} of a {tuple(t.shape)} {t.dtype} tensor breaks the operand rules: base "
                             f"{view.data_ptr() % 16} mod 16, strides {tuple(view.stride())}")
    return view


def guarded_out(shape, dtype, strides, device, fill=SENTINEL, guard_bytes=GUARD_BYTES):
    """-> (view, check): an output of `shape` with element `strides` (gaps between rows, heads, batches, or behind the channels of
    a row) inside a buffer of the byte `fill` with `guard_bytes` on either side; `check()` asserts that every byte outside the
    view's own elements still holds `fill` and names the first and last touched byte relative to the view's first element."""
    shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
    assert len(shape) == len(strides) and all(s > 0 for s in shape) and all(s >= 0 for s in strides)
    itemsize = _itemsize(dtype)
    extent = sum((n - 1) * s for n, s in zip(shape, strides)) + 1  # elements from the first to the last one of the view
    assert guard_bytes % ALIGN == 0
    buf = torch.full((guard_bytes + ALIGN + extent * itemsize + guard_bytes,), fill, dtype=torch.uint8, device=device)
    offset = guard_bytes + (-(buf.data_ptr() + guard_bytes)) % ALIGN
    view = torch.as_strided(buf[offset:offset + extent * itemsize].view(dtype), shape, strides)
    own = torch.zeros((extent,), dtype=torch.bool, device=device)
    torch.as_strided(own, shape, strides).fill_(True)
    keep = torch.zeros(buf.shape, dtype=torch.bool, device=device)
    keep[offset:offset + extent * itemsize] = own.repeat_interleave(itemsize)

    def check(what=""):
        idx = _touched(buf, keep, fill)
        assert idx.numel() == 0, (f"{what}: {int(idx.numel())} bytes outside the output view {shape} (strides {strides}, {dtype}) were "
                                  f"written, first at byte offset {int(idx[0]) - offset}, last at {int(idx[-1]) - offset} relative to the view")

    check.touched = lambda: [int(i) - offset for i in _touched(buf, keep, fill).tolist()]
    return view, check
