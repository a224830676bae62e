"""Argument validation of the backward C ABI (`lbfa_backward`): LBFA_EINVAL with a message before any launch (no GPU
needed - every case below is rejected before the first launch)."""
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


def test_backward_workspace_bytes(lib):
    need_q = lib.lbfa_backward_workspace_bytes(1, 4, 2, 100, 100, 64, 127, 1)
    need_f = lib.lbfa_backward_workspace_bytes(1, 4, 2, 100, 100, 64, 0, 0)
    assert need_q > need_f > 0  # codes, scales, mean and correction only when quantised
    assert lib.lbfa_backward_workspace_bytes(1, 4, 2, 100, 100, 80, 127, 1) == 0  # the caller pads to 64 / 128
    assert lib.lbfa_backward_workspace_bytes(0, 4, 2, 100, 100, 64, 127, 1) == 0


def test_backward_argument_validation_messages(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    s = _lib.strides3((1024, 512, 64))
    ws = 1 << 15

    def call(q=p, lse=p, dq=p, dtype=0, work=ws, B=1, Hq=2, Hkv=2, Sq=8, Sk=8, D=64, sq=s, sm=0.125, qq=127, kq=127, causal=0):
        return lib.lbfa_backward(q, p, p, p, p, dtype, lse, None, dq, p, p, p, work, B, Hq, Hkv, Sq, Sk, D,
                                 sq, s, s, s, s, s, s, s, sm, qq, kq, causal, 1, None)

    cases = [
        (dict(q=None), b"null pointer"),
        (dict(lse=None), b"null pointer"),
        (dict(sq=None), b"null pointer"),
        (dict(Sq=0), b"empty tensor"),
        (dict(D=96), b"Unsupported head_dim: 96"),
        (dict(Hq=3), b"divisible"),
        (dict(dtype=5), b"float16 or bfloat16"),
        (dict(qq=15), b"q_qmax / k_qmax"),
        (dict(qq=0), b"q_qmax / k_qmax"),
        (dict(causal=1, Sk=16), b"qo_len and kv_len must be equal"),
        (dict(sm=0.0), b"sm_scale must be positive"),
        (dict(q=p + 8), b"q must be 16-byte aligned"),
        (dict(sq=_lib.strides3((1024, 512, 60))), b"q must be 16-byte aligned"),
        (dict(dq=p + 1), b"2-byte aligned"),
        (dict(lse=p + 2), b"4-byte aligned"),
        (dict(work=16), b"workspace too small"),
    ]
    for kw, msg in cases:
        st = call(**kw)
        assert st == _lib.LBFA_EINVAL, kw
        assert msg in lib.lbfa_last_error(), (kw, lib.lbfa_last_error())
    with pytest.raises(ValueError, match="Unsupported head_dim: 96"):
        _lib.check(call(D=96), lib)
