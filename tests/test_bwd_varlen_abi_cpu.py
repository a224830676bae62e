"""Argument validation of the packed-batch C ABI (`lbfa_backward_varlen`, `lbfa_forward_varlen_lse`): LBFA_EINVAL with a
message before any launch (no GPU needed - every case below is rejected before the first launch)."""
import ctypes
import os

import pytest


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
