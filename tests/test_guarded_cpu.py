"""The guard-band harness (tests/guarded.py) tested on itself, on CPU tensors: fake kernels that write one element before an
allocation, one behind it, or one into a stride gap must each be reported with the right offset; a clean write passes;
`hostile_view` gives the values of `t` under the C ABI's operand rules; `torch.empty` is restored when the block ends, also when
its body raises.  This is the mutation evidence of the GPU containment tests: what they would say about a kernel that strays."""
import pytest

torch = pytest.importorskip("torch")

import guarded  # noqa: E402

CPU = torch.device("cpu")


def _raw(t, byte_offset, nbytes):
    """the `nbytes` bytes at `byte_offset` from the first element of `t`, as a fake kernel with a wrong address sees them"""
    base = t.untyped_storage()
    start = t.storage_offset() * t.element_size() + byte_offset
    return torch.tensor([], dtype=torch.uint8).set_(base, start, (nbytes,), (1,))


def test_clean_write_passes_and_allocation_is_aligned_and_guarded(monkeypatch):
    with guarded.GuardArena(monkeypatch, CPU) as arena:
        a = torch.empty((3, 5, 7), dtype=torch.float16, device="cpu")
        b = torch.empty(129, 80, dtype=torch.float32)          # sizes as separate integers, default device
        c = torch.empty((0, 4), dtype=torch.int8)              # nothing to guard
    assert len(arena) == 2 and c.numel() == 0
    for t, shape in ((a, (3, 5, 7)), (b, (129, 80))):
        assert tuple(t.shape) == shape and t.is_contiguous() and t.data_ptr() % 256 == 0
        t.fill_(1.5)                                           # the whole extent, first and last byte included
    for al in arena.allocations:
        assert al["offset"] >= 128 * 1024 and al["buf"].numel() - al["offset"] - al["nbytes"] >= 128 * 1024
        assert torch.all(al["buf"][:al["offset"]] == guarded.SENTINEL)
    arena.check()
    assert arena.violations() == []


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int8])
@pytest.mark.parametrize("where", ["before", "after", "far_after"])
def test_one_element_overrun_is_reported_with_its_offset(monkeypatch, dtype, where):
    with guarded.GuardArena(monkeypatch, CPU) as arena:
        torch.empty((4, 4), dtype=torch.float32, device=CPU).zero_()      # allocation #0 stays clean
        out = torch.empty((2, 129, 40), dtype=dtype, device=CPU)
    out.zero_()
    es, nbytes = out.element_size(), out.numel() * out.element_size()
    off = {"before": -es, "after": nbytes, "far_after": nbytes + 128 * 1024 - es}[where]  # the last byte a guard still covers
    _raw(out, off, es).fill_(0)  # the fake kernel: one element, one row too early / too far
    v = arena.violations()
    assert len(v) == 1 and v[0]["order"] == 1 and v[0]["shape"] == (2, 129, 40) and v[0]["dtype"] == dtype
    assert (v[0]["first"], v[0]["last"], v[0]["count"]) == (off, off + es - 1, es)
    with pytest.raises(AssertionError, match=rf"allocation #1 \(2, 129, 40\).*first at byte offset {off}, last at {off + es - 1} "):
        arena.check()


def test_arena_restores_torch_empty_also_when_the_body_raises(monkeypatch):
    real = torch.empty
    with guarded.GuardArena(monkeypatch, CPU):
        assert torch.empty is not real
    assert torch.empty is real
    with pytest.raises(RuntimeError, match="boom"):
        with guarded.GuardArena(monkeypatch, CPU):
            torch.empty((8,), dtype=torch.uint8)
            raise RuntimeError("boom")
    assert torch.empty is real
    assert torch.empty((2, 2)).untyped_storage().nbytes() == 16  # a plain allocation again


def test_arena_leaves_other_devices_and_unusual_calls_alone(monkeypatch):
    with guarded.GuardArena(monkeypatch, CPU) as arena:
        m = torch.empty((4,), dtype=torch.float32, device="meta")
        p = torch.empty((4, 4, 4, 4), dtype=torch.float32, memory_format=torch.channels_last)
    assert m.device.type == "meta" and p.is_contiguous(memory_format=torch.channels_last) and len(arena) == 0


def test_arena_backed_copy_of_a_tensor(monkeypatch):
    arena = guarded.GuardArena(monkeypatch, CPU)
    src = torch.arange(24, dtype=torch.int32).view(2, 3, 4)
    g = arena.like(src)
    assert torch.equal(g, src) and g.data_ptr() % 256 == 0
    arena.check()
    _raw(g, -4, 4).fill_(7)
    assert arena.violations()[0]["first"] == -4


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("D", [40, 64, 80, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hostile_view_keeps_values_and_operand_rules(layout, D, dtype):
    B, H, S = 2, 3, 5
    Dbuf = 64 if D <= 64 else 128
    shape = (B, H, S, D) if layout == "HND" else (B, S, H, D)
    t = torch.randn(shape, generator=torch.Generator().manual_seed(D)).to(dtype)
    hv = guarded.hostile_view(t, before=(1, 1, 2, 0), after=(1, 2, 1, Dbuf - D))
    assert tuple(hv.shape) == shape and hv.dtype == dtype and torch.equal(hv, t)
    assert hv.stride(-1) == 1 and hv.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in hv.stride()[:3])
    assert hv.stride(2) == Dbuf and hv.stride(1) == (shape[2] + 3) * Dbuf
    # everything around it is NaN: before row 0, behind the last row, between heads and batches, in the channels past D
    base = hv._base
    assert tuple(base.shape) == (B + 2, shape[1] + 3, shape[2] + 3, Dbuf)
    own = torch.zeros(base.shape, dtype=torch.bool)
    own[1:1 + B, 1:1 + shape[1], 2:2 + shape[2], :D] = True
    assert torch.isnan(base[~own]).all() and not torch.isnan(base[own]).any()
    assert int((~own).sum()) == base.numel() - t.numel()
    if D < Dbuf:
        assert torch.isnan(base[1, 1, 2, D:]).all()  # the channels D .. Dbuf - 1 of the first row


def test_hostile_view_codes_scales_and_refusals():
    codes = torch.randint(-127, 128, (2, 2, 65, 64), dtype=torch.int8)
    hv = guarded.hostile_view(codes, before=(0, 1, 1, 0), after=(0, 0, 1, 64))
    assert torch.equal(hv, codes) and hv.data_ptr() % 16 == 0 and int((hv._base == -128).sum()) >= hv._base.numel() - codes.numel()
    scale = torch.rand(2, 2, 3)
    hs = guarded.hostile_view(scale, before=(1, 0, 0), after=(1, 0, 0), fill=guarded.hostile_fill(scale.dtype, scale=True),
                              check_abi=False)
    assert torch.equal(hs, scale) and hs.is_contiguous() and torch.isinf(hs._base[0]).all() and torch.isinf(hs._base[-1]).all()
    with pytest.raises(ValueError, match="operand rules"):  # a 4-channel shift of the base: 8 bytes, not 16
        guarded.hostile_view(torch.zeros(2, 2, 4, 64, dtype=torch.float16), before=(0, 0, 0, 4), after=(0, 0, 0, 4))
    with pytest.raises(ValueError, match="operand rules"):  # rows of 68 elements
        guarded.hostile_view(torch.zeros(2, 2, 4, 64, dtype=torch.float16), before=(0, 0, 0, 0), after=(0, 0, 0, 4))


def test_guarded_out_reports_a_store_into_a_stride_gap():
    # 80 channels in 128-channel rows, doubled token and head strides: the entry points that take output strides
    B, H, S, D, Dbuf = 2, 2, 3, 80, 128
    strides = (H * 2 * S * 2 * Dbuf, S * 2 * 2 * Dbuf, 2 * Dbuf, 1)
    o, check = guarded_out_cpu((B, H, S, D), torch.float16, strides)
    assert tuple(o.shape) == (B, H, S, D) and tuple(o.stride()) == strides and o.data_ptr() % 256 == 0
    o.fill_(1.0)  # a clean kernel: every element of the view, nothing else
    check("clean")
    assert check.touched() == []
    # channel 80 of row (0, 1, 2): the O store without its `d0 >= d_valid` test
    gap = (1 * strides[1] + 2 * strides[2] + D) * 2
    _raw(o, gap, 2).fill_(0)
    assert check.touched() == [gap, gap + 1]
    with pytest.raises(AssertionError, match=rf"2 bytes outside the output view .*first at byte offset {gap}, last at {gap + 1} "):
        check("gap")


@pytest.mark.parametrize("where", ["before", "after", "row_gap"])
def test_guarded_out_reports_strays_around_and_between_rows(where):
    strides = (2 * 5 * 64, 2 * 64, 1)  # [4, 5, 64] with every other token row a gap
    o, check = guarded_out_cpu((4, 5, 64), torch.float32, strides)
    o.zero_()
    extent = (3 * strides[0] + 4 * strides[1] + 63 + 1) * 4
    off = {"before": -4, "after": extent, "row_gap": (strides[1] // 2) * 4}[where]
    _raw(o, off, 4).fill_(0)
    assert check.touched() == [off, off + 1, off + 2, off + 3]
    with pytest.raises(AssertionError, match=rf"first at byte offset {off}, last at {off + 3} "):
        check(where)


def guarded_out_cpu(shape, dtype, strides):
    return guarded.guarded_out(shape, dtype, strides, CPU)
