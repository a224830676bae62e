"""Argument validation of the backward C ABI (`lbfa_backward`): LBFA_EINVAL with a message before any launch (no GPU
needed - every case below is rejected before the first launch)."""
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


# status and full text of lbfa_last_error() for calls with one thing wrong (tests/cabi_calls.py): every check of every entry
# point that can fire without a GPU, the 2 GiB operand windows on both sides of their limit (the largest accepted stride or
# length is shown by the NEXT check firing: the grid-size check, which needs integers only).  (name, overrides, message)
SINGLE_FAULT = [
    ("lbfa_backward", dict(k=None),
     'lbfa_backward: null pointer'),
    ("lbfa_backward", dict(dout=None),
     'lbfa_backward: null pointer'),
    ("lbfa_backward", dict(dv=None),
     'lbfa_backward: null pointer'),
    ("lbfa_backward", dict(workspace=None),
     'lbfa_backward: null pointer'),
    ("lbfa_backward", dict(sdk=None),
     'lbfa_backward: null pointer'),
    ("lbfa_backward", dict(B=0),
     'lbfa_backward: empty tensor'),
    ("lbfa_backward", dict(Sk=0),
     'lbfa_backward: empty tensor'),
    ("lbfa_backward", dict(D=40),
     'lbfa_backward: Unsupported head_dim: 40 (64 or 128; pad other head dims with zeros)'),
    ("lbfa_backward", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_backward", dict(dtype=2),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_backward", dict(q_qmax=0),
     'lbfa_backward: q_qmax / k_qmax must both be 0 (un-quantised) or each 127 / 7, got 0 / 127'),
    ("lbfa_backward", dict(k_qmax=0),
     'lbfa_backward: q_qmax / k_qmax must both be 0 (un-quantised) or each 127 / 7, got 127 / 0'),
    ("lbfa_backward", dict(k_qmax=15),
     'lbfa_backward: q_qmax / k_qmax must both be 0 (un-quantised) or each 127 / 7, got 127 / 15'),
    ("lbfa_backward", dict(causal=1, Sk=16),
     'qo_len and kv_len must be equal for causal attention'),
    ("lbfa_backward", dict(sm_scale=-1.0),
     'lbfa_backward: sm_scale must be positive'),
    ("lbfa_backward", dict(k=A(8)),
     'lbfa_backward: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(sk=(1024, 512, 60)),
     'lbfa_backward: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(v=A(8)),
     'lbfa_backward: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(sv=(1024, 512, 60)),
     'lbfa_backward: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(o=A(8)),
     'lbfa_backward: o must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(so=(1024, 512, 60)),
     'lbfa_backward: o must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(dout=A(8)),
     'lbfa_backward: dout must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(sdout=(1024, 512, 60)),
     'lbfa_backward: dout must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_backward", dict(dk=A(1)),
     'lbfa_backward: dq / dk / dv must be 2-byte aligned'),
    ("lbfa_backward", dict(dv=A(1)),
     'lbfa_backward: dq / dk / dv must be 2-byte aligned'),
    ("lbfa_backward", dict(dlse=A(2)),
     'lbfa_backward: lse / dlse must be 4-byte aligned'),
    ("lbfa_backward", dict(workspace_bytes=16),
     'lbfa_backward: workspace too small (16 < 4352)'),
    ("lbfa_backward", dict(workspace_bytes=16, q_qmax=0, k_qmax=0),
     'lbfa_backward: workspace too small (16 < 512)'),
    ("lbfa_backward", dict(workspace=A(8)),
     'lbfa_backward: workspace must be 16-byte aligned'),
    ("lbfa_backward", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=65536),
     'lbfa_backward: grid too large'),
    ("lbfa_backward", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_backward: grid too large'),
    ("lbfa_backward", dict(workspace_bytes=4611686018427387904, B=16, Hq=1048576, Hkv=1048576, Sq=128),
     'lbfa_backward: grid too large'),
]


# value of every workspace-size function on a grid of shapes, invalid ones (-> 0) included: (arguments, bytes)
WORKSPACE_SIZES = {
    "lbfa_backward_workspace_bytes": [
        ((2, 8, 2, 300, 1000, 40, 127, 1), 0),
        ((2, 8, 2, 300, 1000, 40, 7, 0), 0),
        ((2, 8, 2, 300, 1000, 40, 0, 1), 0),
        ((2, 8, 2, 300, 1000, 40, 0, 0), 0),
        ((1, 4, 4, 128, 20000, 40, 127, 1), 0),
        ((1, 4, 4, 128, 20000, 40, 7, 0), 0),
        ((1, 4, 4, 128, 20000, 40, 0, 1), 0),
        ((1, 4, 4, 128, 20000, 40, 0, 0), 0),
        ((2, 8, 2, 300, 1000, 64, 127, 1), 610816),
        ((2, 8, 2, 300, 1000, 64, 7, 0), 602112),
        ((2, 8, 2, 300, 1000, 64, 0, 1), 38400),
        ((2, 8, 2, 300, 1000, 64, 0, 0), 38400),
        ((1, 4, 4, 128, 20000, 64, 127, 1), 5203712),
        ((1, 4, 4, 128, 20000, 64, 7, 0), 5162240),
        ((1, 4, 4, 128, 20000, 64, 0, 1), 4096),
        ((1, 4, 4, 128, 20000, 64, 0, 0), 4096),
        ((2, 8, 2, 300, 1000, 96, 127, 1), 0),
        ((2, 8, 2, 300, 1000, 96, 7, 0), 0),
        ((2, 8, 2, 300, 1000, 96, 0, 1), 0),
        ((2, 8, 2, 300, 1000, 96, 0, 0), 0),
        ((1, 4, 4, 128, 20000, 96, 127, 1), 0),
        ((1, 4, 4, 128, 20000, 96, 7, 0), 0),
        ((1, 4, 4, 128, 20000, 96, 0, 1), 0),
        ((1, 4, 4, 128, 20000, 96, 0, 0), 0),
        ((2, 8, 2, 300, 1000, 128, 127, 1), 1182720),
        ((2, 8, 2, 300, 1000, 128, 7, 0), 1165312),
        ((2, 8, 2, 300, 1000, 128, 0, 1), 38400),
        ((2, 8, 2, 300, 1000, 128, 0, 0), 38400),
        ((1, 4, 4, 128, 20000, 128, 127, 1), 10397952),
        ((1, 4, 4, 128, 20000, 128, 7, 0), 10315008),
        ((1, 4, 4, 128, 20000, 128, 0, 1), 4096),
        ((1, 4, 4, 128, 20000, 128, 0, 0), 4096),
        ((1, 2, 0, 8, 8, 64, 127, 1), 0),
    ],
}


def test_single_fault_messages(lib):
    check_table(lib, SINGLE_FAULT)


def test_workspace_sizes_pinned(lib):
    for fn, rows in WORKSPACE_SIZES.items():
        for args, size in rows:
            assert getattr(lib, fn)(*args) == size, (fn, args)
