"""Argument validation of the packed-batch C ABI (`lbfa_backward_varlen`, `lbfa_forward_varlen_lse`): LBFA_EINVAL with a
message before any launch (no GPU needed - every case below is rejected before the first launch)."""
import ctypes
import os

import pytest

from cabi_calls import A, check_table


@pytest.fixture(scope="module")
def lib():
    from lowbit_quant_fa2_paddle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_backward_varlen_workspace_bytes(lib):
    need = lib.lbfa_backward_varlen_workspace_bytes(3, 4, 2, 300, 280, 200, 150, 64, 127, 1)
    plain = lib.lbfa_backward_varlen_workspace_bytes(3, 4, 2, 300, 280, 200, 150, 64, 127, 0)
    assert need > plain > 0  # mean and correction only with smooth-K
    # codes [total, H, D] + padded scales [B, H, max_blocks] + lse2 / delta [Hq, total_q]
    assert plain >= 300 * 4 * 64 + 280 * 2 * 64 + 2 * 4 * 4 * 300
    assert lib.lbfa_backward_varlen_workspace_bytes(3, 4, 2, 300, 280, 200, 150, 80, 127, 1) == 0  # the caller pads
    assert lib.lbfa_backward_varlen_workspace_bytes(3, 4, 2, 300, 280, 200, 150, 64, 0, 1) == 0  # always quantised
    assert lib.lbfa_backward_varlen_workspace_bytes(0, 4, 2, 300, 280, 200, 150, 64, 127, 1) == 0
    assert lib.lbfa_backward_varlen_workspace_bytes(3, 4, 2, 0, 280, 200, 150, 64, 127, 1) == 0


def test_backward_varlen_argument_validation_messages(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    s = _lib.strides2((64, 128))
    ws = 1 << 15

    def call(q=p, lse=p, dlse=None, dq=p, cu=p, dtype=0, work=ws, B=1, Hq=2, Hkv=2, tq=8, tk=8, mq=8, mk=8, D=64, sq=s, sm=0.125,
             qq=127, kq=127):
        return lib.lbfa_backward_varlen(q, p, p, p, p, dtype, lse, dlse, dq, p, p, cu, p, p, work, B, Hq, Hkv, tq, tk, mq, mk, D,
                                        sq, s, s, s, s, s, s, s, sm, qq, kq, 0, 1, None)

    cases = [
        (dict(q=None), b"null pointer"),
        (dict(lse=None), b"null pointer"),
        (dict(cu=None), b"null pointer"),
        (dict(sq=None), b"null pointer"),
        (dict(tq=0), b"empty batch"),
        (dict(mk=0), b"empty batch"),
        (dict(B=0), b"empty batch"),
        (dict(D=96), b"Unsupported head_dim: 96"),
        (dict(Hq=3), b"divisible"),
        (dict(dtype=5), b"float16 or bfloat16"),
        (dict(qq=0), b"q_qmax / k_qmax must each be 127 or 7"),
        (dict(kq=15), b"q_qmax / k_qmax must each be 127 or 7"),
        (dict(sm=0.0), b"sm_scale must be positive"),
        (dict(q=p + 8), b"q must be 16-byte aligned"),
        (dict(sq=_lib.strides2((64, 60))), b"q must be 16-byte aligned"),
        (dict(dq=p + 1), b"2-byte aligned"),
        (dict(lse=p + 2), b"4-byte aligned"),
        (dict(dlse=p + 2), b"4-byte aligned"),
        (dict(work=16), b"workspace too small"),
        (dict(work=ws, tq=(1 << 30), Hq=2), b"lbfa_backward_varlen"),
    ]
    for kw, msg in cases:
        st = call(**kw)
        assert st == _lib.LBFA_EINVAL, kw
        assert msg in lib.lbfa_last_error(), (kw, lib.lbfa_last_error())
    with pytest.raises(ValueError, match="Unsupported head_dim: 96"):
        _lib.check(call(D=96), lib)


def test_forward_varlen_lse_argument_validation(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    s = _lib.strides2((64, 128))
    ws = lib.lbfa_forward_varlen_workspace_bytes(1, 2, 2, 8, 8, 8, 8, 64)
    assert 0 < ws <= 1 << 15

    def call(lse=p, q=p, work=ws, D=64, qq=127):
        return lib.lbfa_forward_varlen_lse(q, p, p, 0, p, lse, p, p, p, work, 1, 2, 2, 8, 8, 8, 8, D, s, s, s, s, 0.125, qq, 127,
                                           0, 1, None)

    for kw, msg in [(dict(lse=p + 2), b"lse must be 4-byte aligned"), (dict(q=None), b"lbfa_forward_varlen_lse: null pointer"),
                    (dict(work=16), b"lbfa_forward_varlen_lse: workspace too small"), (dict(D=160), b"Unsupported head_dim"),
                    (dict(qq=15), b"lbfa_forward_varlen_lse: q_qmax must be 127")]:
        assert call(**kw) == _lib.LBFA_EINVAL, kw
        assert msg in lib.lbfa_last_error(), (kw, lib.lbfa_last_error())


# status and full text of lbfa_last_error() for calls with one thing wrong (tests/cabi_calls.py): every check of every entry
# point that can fire without a GPU, the 2 GiB operand windows on both sides of their limit (the largest accepted stride or
# length is shown by the NEXT check firing: the grid-size check, which needs integers only).  (name, overrides, message)
SINGLE_FAULT = [
    ("lbfa_forward_varlen", dict(q=None),
     'lbfa_forward_varlen: null pointer'),
    ("lbfa_forward_varlen", dict(cu_q=None),
     'lbfa_forward_varlen: null pointer'),
    ("lbfa_forward_varlen", dict(workspace=None),
     'lbfa_forward_varlen: null pointer'),
    ("lbfa_forward_varlen", dict(so=None),
     'lbfa_forward_varlen: null pointer'),
    ("lbfa_forward_varlen", dict(B=0),
     'lbfa_forward_varlen: empty batch'),
    ("lbfa_forward_varlen", dict(total_k=0),
     'lbfa_forward_varlen: empty batch'),
    ("lbfa_forward_varlen", dict(max_q=0),
     'lbfa_forward_varlen: empty batch'),
    ("lbfa_forward_varlen", dict(D=36),
     'Unsupported head_dim: 36'),
    ("lbfa_forward_varlen", dict(D=136),
     'Unsupported head_dim: 136'),
    ("lbfa_forward_varlen", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_forward_varlen", dict(workspace_bytes=16),
     'lbfa_forward_varlen: workspace too small (16 < 2560)'),
    ("lbfa_forward_varlen", dict(workspace=A(8)),
     'lbfa_forward_varlen: workspace must be 16-byte aligned'),
    ("lbfa_forward_varlen", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_forward_varlen", dict(q_qmax=15),
     'lbfa_forward_varlen: q_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward_varlen", dict(k_qmax=15),
     'lbfa_forward_varlen: k_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward_varlen", dict(q=A(8)),
     'lbfa_forward_varlen: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen", dict(v=A(8)),
     'lbfa_forward_varlen: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen", dict(o=A(4)),
     'lbfa_forward_varlen: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen", dict(sq=(64, 60)),
     'lbfa_forward_varlen: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen", dict(sk=(64, 60)),
     'lbfa_forward_varlen: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen", dict(sv=(64, 60)),
     'lbfa_forward_varlen: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen", dict(so=(62, 128)),
     'lbfa_forward_varlen: o strides must be multiples of 4 elements'),
    ("lbfa_forward_varlen", dict(sq=(64, 7895160)),
     'lbfa_forward_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen", dict(sq=(64, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen: grid too large'),
    ("lbfa_forward_varlen", dict(sv=(64, 7895160)),
     'lbfa_forward_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen", dict(sv=(64, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen: grid too large'),
    ("lbfa_forward_varlen", dict(max_k=16777088, workspace_bytes=4611686018427387904, sv=(64, 8)),
     'lbfa_forward_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen", dict(max_k=16777087, workspace_bytes=4611686018427387904, sv=(64, 8), B=65536, Hq=65536, Hkv=2),
     'lbfa_forward_varlen: grid too large'),
    ("lbfa_forward_varlen", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen: grid too large'),
    ("lbfa_forward_varlen_lse", dict(q=None),
     'lbfa_forward_varlen_lse: null pointer'),
    ("lbfa_forward_varlen_lse", dict(cu_q=None),
     'lbfa_forward_varlen_lse: null pointer'),
    ("lbfa_forward_varlen_lse", dict(workspace=None),
     'lbfa_forward_varlen_lse: null pointer'),
    ("lbfa_forward_varlen_lse", dict(so=None),
     'lbfa_forward_varlen_lse: null pointer'),
    ("lbfa_forward_varlen_lse", dict(B=0),
     'lbfa_forward_varlen_lse: empty batch'),
    ("lbfa_forward_varlen_lse", dict(total_k=0),
     'lbfa_forward_varlen_lse: empty batch'),
    ("lbfa_forward_varlen_lse", dict(max_q=0),
     'lbfa_forward_varlen_lse: empty batch'),
    ("lbfa_forward_varlen_lse", dict(D=36),
     'Unsupported head_dim: 36'),
    ("lbfa_forward_varlen_lse", dict(D=136),
     'Unsupported head_dim: 136'),
    ("lbfa_forward_varlen_lse", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_forward_varlen_lse", dict(workspace_bytes=16),
     'lbfa_forward_varlen_lse: workspace too small (16 < 2560)'),
    ("lbfa_forward_varlen_lse", dict(workspace=A(8)),
     'lbfa_forward_varlen_lse: workspace must be 16-byte aligned'),
    ("lbfa_forward_varlen_lse", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_forward_varlen_lse", dict(q_qmax=15),
     'lbfa_forward_varlen_lse: q_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward_varlen_lse", dict(k_qmax=15),
     'lbfa_forward_varlen_lse: k_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward_varlen_lse", dict(q=A(8)),
     'lbfa_forward_varlen_lse: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen_lse", dict(v=A(8)),
     'lbfa_forward_varlen_lse: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen_lse", dict(o=A(4)),
     'lbfa_forward_varlen_lse: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_forward_varlen_lse", dict(sq=(64, 60)),
     'lbfa_forward_varlen_lse: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen_lse", dict(sk=(64, 60)),
     'lbfa_forward_varlen_lse: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen_lse", dict(sv=(64, 60)),
     'lbfa_forward_varlen_lse: q / k / v strides must be multiples of 8 elements'),
    ("lbfa_forward_varlen_lse", dict(so=(62, 128)),
     'lbfa_forward_varlen_lse: o strides must be multiples of 4 elements'),
    ("lbfa_forward_varlen_lse", dict(sq=(64, 7895160)),
     'lbfa_forward_varlen_lse: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen_lse", dict(sq=(64, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen_lse: grid too large'),
    ("lbfa_forward_varlen_lse", dict(sv=(64, 7895160)),
     'lbfa_forward_varlen_lse: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen_lse", dict(sv=(64, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen_lse: grid too large'),
    ("lbfa_forward_varlen_lse", dict(max_k=16777088, workspace_bytes=4611686018427387904, sv=(64, 8)),
     'lbfa_forward_varlen_lse: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_forward_varlen_lse", dict(max_k=16777087, workspace_bytes=4611686018427387904, sv=(64, 8), B=65536, Hq=65536, Hkv=2),
     'lbfa_forward_varlen_lse: grid too large'),
    ("lbfa_forward_varlen_lse", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward_varlen_lse: grid too large'),
    ("lbfa_forward_varlen_lse", dict(lse=A(2)),
     'lbfa_forward_varlen_lse: lse must be 4-byte aligned'),
    ("lbfa_backward_varlen", dict(k=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(dout=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(dv=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(cu_k=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(workspace=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(sdk=None),
     'lbfa_backward_varlen: null pointer'),
    ("lbfa_backward_varlen", dict(total_k=0),
     'lbfa_backward_varlen: empty batch'),
    ("lbfa_backward_varlen", dict(max_q=0),
     'lbfa_backward_varlen: empty batch'),
    ("lbfa_backward_varlen", dict(D=40),
     'lbfa_backward_varlen: Unsupported head_dim: 40 (64 or 128; pad other head dims with zeros)'),
    ("lbfa_backward_varlen", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_backward_varlen", dict(dtype=2),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_backward_varlen", dict(q_qmax=15),
     'lbfa_backward_varlen: q_qmax / k_qmax must each be 127 or 7, got 15 / 127'),
    ("lbfa_backward_varlen", dict(k_qmax=0),
     'lbfa_backward_varlen: q_qmax / k_qmax must each be 127 or 7, got 127 / 0'),
    ("lbfa_backward_varlen", dict(sm_scale=-1.0),
     'lbfa_backward_varlen: sm_scale must be positive'),
    ("lbfa_backward_varlen", dict(k=A(8)),
     'lbfa_backward_varlen: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(sk=(64, 60)),
     'lbfa_backward_varlen: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(v=A(8)),
     'lbfa_backward_varlen: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(sv=(64, 60)),
     'lbfa_backward_varlen: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(o=A(8)),
     'lbfa_backward_varlen: o must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(so=(64, 60)),
     'lbfa_backward_varlen: o must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(dout=A(8)),
     'lbfa_backward_varlen: dout must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(sdout=(64, 60)),
     'lbfa_backward_varlen: dout must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward_varlen", dict(dk=A(1)),
     'lbfa_backward_varlen: dq / dk / dv must be 2-byte aligned'),
    ("lbfa_backward_varlen", dict(dv=A(1)),
     'lbfa_backward_varlen: dq / dk / dv must be 2-byte aligned'),
    ("lbfa_backward_varlen", dict(workspace_bytes=16),
     'lbfa_backward_varlen: workspace too small (16 < 4352)'),
    ("lbfa_backward_varlen", dict(workspace=A(8)),
     'lbfa_backward_varlen: workspace must be 16-byte aligned'),
    ("lbfa_backward_varlen", dict(workspace_bytes=4611686018427387904, total_q=1073741824),
     'lbfa_backward_varlen: grid too large'),
    ("lbfa_backward_varlen", dict(workspace_bytes=4611686018427387904, total_k=1073741824),
     'lbfa_backward_varlen: grid too large'),
    ("lbfa_backward_varlen", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_backward_varlen: grid too large'),
]


# value of every workspace-size function on a grid of shapes, invalid ones (-> 0) included: (arguments, bytes)
WORKSPACE_SIZES = {
    "lbfa_forward_varlen_workspace_bytes_dt": [
        ((3, 4, 2, 300, 280, 200, 150, 40, 0), 38400),
        ((3, 4, 2, 300, 280, 200, 150, 40, 1), 110080),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40, 0), 20675072),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40, 1), 61635072),
        ((3, 4, 2, 300, 280, 200, 150, 64, 0), 38400),
        ((3, 4, 2, 300, 280, 200, 150, 64, 1), 110080),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64, 0), 20675072),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64, 1), 61635072),
        ((3, 4, 2, 300, 280, 200, 150, 96, 0), 76544),
        ((3, 4, 2, 300, 280, 200, 150, 96, 1), 219904),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96, 0), 41319936),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96, 1), 123239936),
        ((3, 4, 2, 300, 280, 200, 150, 128, 0), 76544),
        ((3, 4, 2, 300, 280, 200, 150, 128, 1), 219904),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128, 0), 41319936),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128, 1), 123239936),
        ((1, 2, 2, 0, 8, 8, 8, 64, 0), 0),
        ((1, 2, 2, 8, 8, 8, 8, 36, 0), 0),
    ],
    "lbfa_forward_varlen_workspace_bytes": [
        ((3, 4, 2, 300, 280, 200, 150, 40), 110080),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40), 61635072),
        ((3, 4, 2, 300, 280, 200, 150, 64), 110080),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64), 61635072),
        ((3, 4, 2, 300, 280, 200, 150, 96), 219904),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96), 123239936),
        ((3, 4, 2, 300, 280, 200, 150, 128), 219904),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128), 123239936),
    ],
    "lbfa_backward_varlen_workspace_bytes": [
        ((3, 4, 2, 300, 280, 200, 150, 40, 127, 1), 0),
        ((3, 4, 2, 300, 280, 200, 150, 40, 7, 0), 0),
        ((3, 4, 2, 300, 280, 200, 150, 40, 0, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40, 127, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40, 7, 0), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 40, 0, 1), 0),
        ((3, 4, 2, 300, 280, 200, 150, 64, 127, 1), 125184),
        ((3, 4, 2, 300, 280, 200, 150, 64, 7, 0), 122880),
        ((3, 4, 2, 300, 280, 200, 150, 64, 0, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64, 127, 1), 23557120),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64, 7, 0), 23392256),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 64, 0, 1), 0),
        ((3, 4, 2, 300, 280, 200, 150, 96, 127, 1), 0),
        ((3, 4, 2, 300, 280, 200, 150, 96, 7, 0), 0),
        ((3, 4, 2, 300, 280, 200, 150, 96, 0, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96, 127, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96, 7, 0), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 96, 0, 1), 0),
        ((3, 4, 2, 300, 280, 200, 150, 128, 127, 1), 240128),
        ((3, 4, 2, 300, 280, 200, 150, 128, 7, 0), 235520),
        ((3, 4, 2, 300, 280, 200, 150, 128, 0, 1), 0),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128, 127, 1), 46761984),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128, 7, 0), 46432256),
        ((2, 8, 8, 5000, 40000, 4000, 30000, 128, 0, 1), 0),
        ((1, 2, 2, 8, 8, 8, 0, 64, 127, 1), 0),
    ],
}


def test_single_fault_messages(lib):
    check_table(lib, SINGLE_FAULT)


def test_workspace_sizes_pinned(lib):
    for fn, rows in WORKSPACE_SIZES.items():
        for args, size in rows:
            assert getattr(lib, fn)(*args) == size, (fn, args)
