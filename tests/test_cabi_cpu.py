"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/lowbit_fa.h declares, and
rejects bad arguments with the reference's messages before touching the GPU (no compute calls here)."""
import ctypes
import os
import re

import pytest

from cabi_calls import A, check_table

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lowbit_fa.h")


def _declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lbfa_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from lowbit_quant_fa2_paddle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    declared = _declared_symbols()
    assert declared, "no declarations parsed from the header"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/lowbit_fa.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared, "ctypes SIGNATURES out of sync with the header"
    assert lib.lbfa_version() == 200


def test_sizes_are_pure_functions(lib):
    # [B,H,nsplit,D] fp64 partial sums with 256-row splits up to 16K keys
    assert lib.lbfa_mean_seq_workspace_bytes(4, 32, 4096, 64) == 4 * 32 * 16 * 64 * 8
    assert lib.lbfa_mean_seq_workspace_bytes(0, 32, 4096, 64) == 0
    assert lib.lbfa_v_fp8_bytes(1, 2, 100, 64) == 1 * 2 * 2 * 64 * 64 + 1 * 2 * 64 * 4


def test_argument_validation_messages(lib):
    from lowbit_quant_fa2_paddle_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    s = _lib.strides3((1024, 512, 64))
    # unsupported head_dim -> the reference's ValueError text (src/core.py:287)
    st = lib.lbfa_attn_fwd(p, p, p, 0, p, 0, None, p, p, None, 1, 2, 2, 8, 8, 96, s, s, s, s, 0, None)
    assert st == _lib.LBFA_EINVAL and b"Unsupported head_dim: 96" in lib.lbfa_last_error()
    with pytest.raises(ValueError, match="Unsupported head_dim: 96"):
        _lib.check(st, lib)
    # GQA divisibility (src/core.py docstring :257), causal needs Sq == Sk (causal forward :389)
    st = lib.lbfa_attn_fwd(p, p, p, 0, p, 0, None, p, p, None, 1, 3, 2, 8, 8, 64, s, s, s, s, 0, None)
    assert st == _lib.LBFA_EINVAL and b"divisible" in lib.lbfa_last_error()
    st = lib.lbfa_attn_fwd(p, p, p, 0, p, 0, None, p, p, None, 1, 2, 2, 8, 16, 64, s, s, s, s, 1, None)
    assert st == _lib.LBFA_EINVAL and b"qo_len and kv_len must be equal" in lib.lbfa_last_error()
    # fp8 V needs v_scale
    st = lib.lbfa_attn_fwd(p, p, p, 2, p, 0, None, p, p, None, 1, 2, 2, 8, 8, 64, s, s, None, s, 0, None)
    assert st == _lib.LBFA_EINVAL and b"v_scale" in lib.lbfa_last_error()
    # quantiser: dtype / qmax / blk
    st = lib.lbfa_quant_per_block(p, 5, None, 1, p, p, 1.0, 127, 128, 1, 1, 8, 64, s, s, None, 1, None, None)
    assert st == _lib.LBFA_EINVAL and b"float16 or bfloat16" in lib.lbfa_last_error()
    st = lib.lbfa_quant_per_block(p, 0, None, 1, p, p, 1.0, 15, 128, 1, 1, 8, 64, s, s, None, 1, None, None)
    assert st == _lib.LBFA_EINVAL and b"qmax" in lib.lbfa_last_error()
    st = lib.lbfa_quant_per_block(p, 0, None, 1, p, p, 1.0, 127, 32, 1, 1, 8, 64, s, s, None, 1, None, None)
    assert st == _lib.LBFA_EINVAL and b"blk" in lib.lbfa_last_error()
    st = lib.lbfa_mean_seq(p, 0, p, p, 0, 1, 1, 8, 64, s, None)
    assert st == _lib.LBFA_EINVAL and b"workspace" in lib.lbfa_last_error()


def test_one_call_and_varlen_validation(lib):
    """The one-call, packed-varlen and un-quantised entry points reject bad arguments before any launch."""
    from lowbit_quant_fa2_paddle_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    s3, s2 = _lib.strides3((1024, 512, 64)), _lib.strides2((64, 128))
    # workspace sizes: pure functions; head dims that are multiples of 8 are accepted, others are not
    need = lib.lbfa_forward_workspace_bytes(1, 2, 2, 8, 8, 64, 0, 1, 0)
    assert need > 0 and lib.lbfa_forward_workspace_bytes(1, 2, 2, 8, 8, 80, 0, 1, 0) > need
    assert lib.lbfa_forward_workspace_bytes(1, 2, 2, 8, 8, 36, 0, 1, 0) == 0
    assert lib.lbfa_forward_varlen_workspace_bytes(2, 2, 2, 16, 16, 8, 8, 64) > 0
    # lbfa_forward
    st = lib.lbfa_forward(p, p, p, 0, p, None, p, need, 1, 2, 2, 8, 8, 36, s3, s3, s3, s3, 0.125, 127, 127, 0, 0, 1, None)
    assert st == _lib.LBFA_EINVAL and b"Unsupported head_dim: 36" in lib.lbfa_last_error()
    st = lib.lbfa_forward(p, p, p, 0, p, None, p, 16, 1, 2, 2, 8, 8, 64, s3, s3, s3, s3, 0.125, 127, 127, 0, 0, 1, None)
    assert st == _lib.LBFA_EINVAL and b"workspace too small" in lib.lbfa_last_error()
    st = lib.lbfa_forward(p, p, p, 0, p, None, p, need, 1, 3, 2, 8, 8, 64, s3, s3, s3, s3, 0.125, 127, 127, 0, 0, 1, None)
    assert st == _lib.LBFA_EINVAL and b"divisible" in lib.lbfa_last_error()
    # packed batches
    st = lib.lbfa_forward_varlen(p, p, p, 0, p, None, p, p, 1 << 15, 2, 2, 2, 16, 16, 8, 8, 64, s2, s2, s2, s2, 0.125, 127, 127, 0, 1, None)
    assert st == _lib.LBFA_EINVAL and b"null pointer" in lib.lbfa_last_error()
    st = lib.lbfa_forward_varlen(p, p, p, 0, p, p, p, p, 1 << 15, 2, 2, 2, 16, 16, 8, 8, 136, s2, s2, s2, s2, 0.125, 127, 127, 0, 1, None)
    assert st == _lib.LBFA_EINVAL and b"Unsupported head_dim: 136" in lib.lbfa_last_error()
    st = lib.lbfa_quant_per_block_varlen(p, 0, None, 1, p, p, p, None, 1.0, 127, 128, 2, 8, 2, 64, s2, s2, None)
    assert st == _lib.LBFA_EINVAL and b"null pointer" in lib.lbfa_last_error()
    st = lib.lbfa_attn_fwd_varlen(p, p, p, 2, p, 0, p, p, p, p, p, p, 2, 2, 2, 8, 8, 64, s2, s2, s2, s2, 0, None)
    assert st == _lib.LBFA_EINVAL and b"v must be float16" in lib.lbfa_last_error()
    # the attention entry points take fp16 (or e4m3) V, as the reference's kernel does: bf16 is cast first (src/core.py:307-308)
    st = lib.lbfa_attn_fwd_varlen(p, p, p, 1, p, 0, p, p, p, p, p, p, 2, 2, 2, 8, 8, 64, s2, s2, s2, s2, 0, None)
    assert st == _lib.LBFA_EINVAL and b"lbfa_cast_bf16_to_f16" in lib.lbfa_last_error()
    st = lib.lbfa_attn_fwd(p, p, p, 1, p, 0, None, p, p, None, 1, 2, 2, 8, 8, 64, s3, s3, s3, s3, 0, None)
    assert st == _lib.LBFA_EINVAL and b"lbfa_cast_bf16_to_f16" in lib.lbfa_last_error()
    st = lib.lbfa_cast_bf16_to_f16(p, p, 1, 2, 8, 36, s3, s3, None)
    assert st == _lib.LBFA_EINVAL and b"multiple of 8" in lib.lbfa_last_error()
    # the router's statistic (lbfa_absmax): null output, dtype, head dim, alignment
    st = lib.lbfa_absmax(p, 0, None, 1, 2, 8, 64, s3, None)
    assert st == _lib.LBFA_EINVAL and b"null pointer" in lib.lbfa_last_error()
    st = lib.lbfa_absmax(p, 2, p, 1, 2, 8, 64, s3, None)
    assert st == _lib.LBFA_EINVAL and b"float16 or bfloat16" in lib.lbfa_last_error()
    st = lib.lbfa_absmax(p, 0, p, 1, 2, 8, 36, s3, None)
    assert st == _lib.LBFA_EINVAL and b"multiple of 8" in lib.lbfa_last_error()
    st = lib.lbfa_absmax(p + 2, 0, p, 1, 2, 8, 64, s3, None)
    assert st == _lib.LBFA_EINVAL and b"16-byte aligned" in lib.lbfa_last_error()
    # a bf16 V is cast into the workspace (not for fp8 PV, whose V quantiser reads bf16 itself): the dtype-aware size is larger
    f16, bf16 = _lib.LBFA_F16, _lib.LBFA_BF16
    assert lib.lbfa_forward_workspace_bytes_dt(1, 2, 2, 8, 8, 128, bf16, 0, 1, 0) > lib.lbfa_forward_workspace_bytes_dt(1, 2, 2, 8, 8, 128, f16, 0, 1, 0)
    assert lib.lbfa_forward_workspace_bytes_dt(1, 2, 2, 8, 8, 64, bf16, 1, 1, 0) == lib.lbfa_forward_workspace_bytes_dt(1, 2, 2, 8, 8, 64, f16, 1, 1, 0)
    assert lib.lbfa_forward_workspace_bytes(1, 2, 2, 8, 8, 128, 0, 1, 0) == lib.lbfa_forward_workspace_bytes_dt(1, 2, 2, 8, 8, 128, bf16, 0, 1, 0)
    assert lib.lbfa_forward_varlen_workspace_bytes_dt(2, 2, 2, 16, 16, 8, 8, 128, bf16) > lib.lbfa_forward_varlen_workspace_bytes_dt(2, 2, 2, 16, 16, 8, 8, 128, f16)
    # un-quantised kernel
    st = lib.lbfa_sdpa_fwd(p, p, p, 0, p, None, 1, 2, 2, 8, 16, 64, s3, s3, s3, s3, 0.125, 1, None)
    assert st == _lib.LBFA_EINVAL and b"qo_len and kv_len must be equal" in lib.lbfa_last_error()
    st = lib.lbfa_sdpa_fwd(p, p, p, 2, p, None, 1, 2, 2, 8, 8, 64, s3, s3, s3, s3, 0.125, 0, None)
    assert st == _lib.LBFA_EINVAL and b"float16 or bfloat16" in lib.lbfa_last_error()
    st = lib.lbfa_sdpa_fwd(p, p, p, 0, p, None, 1, 2, 2, 8, 8, 64, s3, s3, s3, s3, -0.125, 0, None)
    assert st == _lib.LBFA_EINVAL and b"sm_scale must be positive" in lib.lbfa_last_error()


def test_api_surface_matches_reference():
    """Every name the reference package exports (src/__init__.py:1-17) is importable from the package root."""
    import lowbit_quant_fa2_paddle_amd as lb
    for name in ["sageattn", "sageattn_varlen", "sageattn_qk_int8_pv_fp16_triton", "sageattn_qk_int8_pv_fp16_cuda",
                 "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int4_pv_fp16_triton", "lowbit_fa_attn", "lowbit_fa_varlen",
                 "lowbit_fa_multi_precision", "lowbit_fa_qk_int8_pv_fp16_triton", "lowbit_fa_qk_int8_pv_fp16_cuda",
                 "lowbit_fa_qk_int8_pv_fp8_cuda", "lowbit_fa_qk_int4_pv_fp16_triton"]:
        assert callable(getattr(lb, name)), name
    assert lb.lowbit_fa_qk_int8_pv_fp16_triton is lb.sageattn_qk_int8_pv_fp16_triton


def test_host_checks_without_gpu():
    """Host-side checks of src/core.py:269-290 fire before any device work; CPU tensors are refused loudly."""
    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    q = torch.zeros(1, 2, 16, 64, dtype=torch.float32)
    with pytest.raises(AssertionError, match="float16 or torch.bfloat16"):
        lb.lowbit_fa_qk_int8_pv_fp16_triton(q, q, q)
    q16 = q.half()
    with pytest.raises(AssertionError, match="same dtype"):
        lb.lowbit_fa_qk_int8_pv_fp16_triton(q16, q16, q16.bfloat16())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.lowbit_fa_qk_int8_pv_fp16_triton(q16, q16, q16)
    with pytest.raises(ValueError, match="Unsupported quantization backend"):
        lb.lowbit_fa_qk_int8_pv_fp16_triton(q16, q16, q16, quantization_backend="x")
    with pytest.raises(AssertionError, match="qk_quant_gran"):
        lb.lowbit_fa_qk_int8_pv_fp8_cuda(q16, q16, q16, qk_quant_gran="per_block")


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the package may import it."""
    pkg = os.path.join(ROOT, "lowbit_quant_fa2_paddle_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(dirpath, f)


# status and full text of lbfa_last_error() for calls with one thing wrong (tests/cabi_calls.py): every check of every entry
# point that can fire without a GPU, the 2 GiB operand windows on both sides of their limit (the largest accepted stride or
# length is shown by the NEXT check firing: the grid-size check, which needs integers only).  (name, overrides, message)
SINGLE_FAULT = [
    ("lbfa_absmax", dict(x=None),
     'lbfa_absmax: null pointer'),
    ("lbfa_absmax", dict(out=None),
     'lbfa_absmax: null pointer'),
    ("lbfa_absmax", dict(sx=None),
     'lbfa_absmax: null pointer'),
    ("lbfa_absmax", dict(B=0),
     'lbfa_absmax: empty tensor or head_dim 64 not a multiple of 8'),
    ("lbfa_absmax", dict(D=36),
     'lbfa_absmax: empty tensor or head_dim 36 not a multiple of 8'),
    ("lbfa_absmax", dict(D=0),
     'lbfa_absmax: empty tensor or head_dim 0 not a multiple of 8'),
    ("lbfa_absmax", dict(dtype=2),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_absmax", dict(x=A(2)),
     'lbfa_absmax: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_absmax", dict(sx=(1024, 512, 60)),
     'lbfa_absmax: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_mean_seq", dict(x=None),
     'lbfa_mean_seq: null pointer'),
    ("lbfa_mean_seq", dict(mean_out=None),
     'lbfa_mean_seq: null pointer'),
    ("lbfa_mean_seq", dict(workspace=None),
     'lbfa_mean_seq: null pointer'),
    ("lbfa_mean_seq", dict(sx=None),
     'lbfa_mean_seq: null pointer'),
    ("lbfa_mean_seq", dict(D=96),
     'Unsupported head_dim: 96 (or empty tensor 1x2x8)'),
    ("lbfa_mean_seq", dict(S=0),
     'Unsupported head_dim: 64 (or empty tensor 1x2x0)'),
    ("lbfa_mean_seq", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_mean_seq", dict(workspace_bytes=0),
     'lbfa_mean_seq: workspace too small'),
    ("lbfa_mean_seq", dict(x=A(8)),
     'lbfa_mean_seq: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_mean_seq", dict(sx=(1024, 512, 60)),
     'lbfa_mean_seq: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_quant_per_block", dict(x=None),
     'lbfa_quant_per_block: null pointer'),
    ("lbfa_quant_per_block", dict(out=None),
     'lbfa_quant_per_block: null pointer'),
    ("lbfa_quant_per_block", dict(scale=None),
     'lbfa_quant_per_block: null pointer'),
    ("lbfa_quant_per_block", dict(sx=None),
     'lbfa_quant_per_block: null pointer'),
    ("lbfa_quant_per_block", dict(sout=None),
     'lbfa_quant_per_block: null pointer'),
    ("lbfa_quant_per_block", dict(D=96),
     'Unsupported head_dim: 96 (or empty tensor 1x2x8)'),
    ("lbfa_quant_per_block", dict(B=0),
     'Unsupported head_dim: 64 (or empty tensor 0x2x8)'),
    ("lbfa_quant_per_block", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_quant_per_block", dict(qmax=15),
     'lbfa_quant_per_block: qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_quant_per_block", dict(blk=32),
     'lbfa_quant_per_block: blk must be 128 or 64, got 32'),
    ("lbfa_quant_per_block", dict(mean=A(0), mean_group=0),
     'lbfa_quant_per_block: bad mean_group 0 for H=2'),
    ("lbfa_quant_per_block", dict(mean=A(0), mean_group=3),
     'lbfa_quant_per_block: bad mean_group 3 for H=2'),
    ("lbfa_quant_per_block", dict(rowdot_vec=A(0)),
     'lbfa_quant_per_block: rowdot_vec needs rowdot_out and a rowdot_group dividing H'),
    ("lbfa_quant_per_block", dict(rowdot_vec=A(0), rowdot_out=A(0), rowdot_group=3),
     'lbfa_quant_per_block: rowdot_vec needs rowdot_out and a rowdot_group dividing H'),
    ("lbfa_quant_per_block", dict(x=A(8)),
     'lbfa_quant_per_block: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_quant_per_block", dict(sx=(1024, 512, 60)),
     'lbfa_quant_per_block: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_quant_per_block", dict(out=A(4)),
     'lbfa_quant_per_block: out must be 8-byte aligned with strides that are multiples of 8'),
    ("lbfa_quant_per_block", dict(sout=(1024, 512, 60)),
     'lbfa_quant_per_block: out must be 8-byte aligned with strides that are multiples of 8'),
    ("lbfa_quant_per_block_varlen", dict(cu_scale=None),
     'lbfa_quant_per_block_varlen: null pointer'),
    ("lbfa_quant_per_block_varlen", dict(x=None),
     'lbfa_quant_per_block_varlen: null pointer'),
    ("lbfa_quant_per_block_varlen", dict(cu=None),
     'lbfa_quant_per_block_varlen: null pointer'),
    ("lbfa_quant_per_block_varlen", dict(sout=None),
     'lbfa_quant_per_block_varlen: null pointer'),
    ("lbfa_quant_per_block_varlen", dict(D=96),
     'Unsupported head_dim: 96 (or empty batch 1x2x8)'),
    ("lbfa_quant_per_block_varlen", dict(max_seqlen=0),
     'Unsupported head_dim: 64 (or empty batch 1x2x0)'),
    ("lbfa_quant_per_block_varlen", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_quant_per_block_varlen", dict(qmax=15),
     'lbfa_quant_per_block_varlen: qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_quant_per_block_varlen", dict(blk=32),
     'lbfa_quant_per_block_varlen: blk must be 128 or 64, got 32'),
    ("lbfa_quant_per_block_varlen", dict(mean=A(0), mean_group=3),
     'lbfa_quant_per_block_varlen: bad mean_group 3 for H=2'),
    ("lbfa_quant_per_block_varlen", dict(x=A(8)),
     'lbfa_quant_per_block_varlen: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_quant_per_block_varlen", dict(sx=(64, 60)),
     'lbfa_quant_per_block_varlen: x must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_quant_per_block_varlen", dict(out=A(4)),
     'lbfa_quant_per_block_varlen: out must be 8-byte aligned with strides that are multiples of 8'),
    ("lbfa_quant_per_block_varlen", dict(sout=(64, 60)),
     'lbfa_quant_per_block_varlen: out must be 8-byte aligned with strides that are multiples of 8'),
    ("lbfa_quant_v_fp8", dict(v=None),
     'lbfa_quant_v_fp8: null pointer'),
    ("lbfa_quant_v_fp8", dict(v_fp8=None),
     'lbfa_quant_v_fp8: null pointer'),
    ("lbfa_quant_v_fp8", dict(v_scale=None),
     'lbfa_quant_v_fp8: null pointer'),
    ("lbfa_quant_v_fp8", dict(sv=None),
     'lbfa_quant_v_fp8: null pointer'),
    ("lbfa_quant_v_fp8", dict(D=96),
     'Unsupported head_dim: 96 (or empty tensor 1x2x8)'),
    ("lbfa_quant_v_fp8", dict(H=0),
     'Unsupported head_dim: 64 (or empty tensor 1x0x8)'),
    ("lbfa_quant_v_fp8", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_quant_v_fp8", dict(v=A(8)),
     'lbfa_quant_v_fp8: v / v_fp8 must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_quant_v_fp8", dict(v_fp8=A(8)),
     'lbfa_quant_v_fp8: v / v_fp8 must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_quant_v_fp8", dict(sv=(1024, 512, 60)),
     'lbfa_quant_v_fp8: v / v_fp8 must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_cast_bf16_to_f16", dict(src=None),
     'lbfa_cast_bf16_to_f16: null pointer'),
    ("lbfa_cast_bf16_to_f16", dict(sdst=None),
     'lbfa_cast_bf16_to_f16: null pointer'),
    ("lbfa_cast_bf16_to_f16", dict(D=36),
     'lbfa_cast_bf16_to_f16: bad shape (D must be a multiple of 8)'),
    ("lbfa_cast_bf16_to_f16", dict(B=0),
     'lbfa_cast_bf16_to_f16: bad shape (D must be a multiple of 8)'),
    ("lbfa_cast_bf16_to_f16", dict(src=A(8)),
     'lbfa_cast_bf16_to_f16: tensors must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_cast_bf16_to_f16", dict(dst=A(8)),
     'lbfa_cast_bf16_to_f16: tensors must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_cast_bf16_to_f16", dict(ssrc=(1024, 512, 60)),
     'lbfa_cast_bf16_to_f16: tensors must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_cast_bf16_to_f16", dict(sdst=(1024, 512, 60)),
     'lbfa_cast_bf16_to_f16: tensors must be 16-byte aligned, strides multiples of 8 elements'),
    ("lbfa_attn_fwd", dict(q=None),
     'lbfa_attn_fwd: null pointer'),
    ("lbfa_attn_fwd", dict(q_scale=None),
     'lbfa_attn_fwd: null pointer'),
    ("lbfa_attn_fwd", dict(k_scale=None),
     'lbfa_attn_fwd: null pointer'),
    ("lbfa_attn_fwd", dict(sq=None),
     'lbfa_attn_fwd: null pointer'),
    ("lbfa_attn_fwd", dict(so=None),
     'lbfa_attn_fwd: null pointer'),
    ("lbfa_attn_fwd", dict(Sq=0),
     'lbfa_attn_fwd: empty tensor'),
    ("lbfa_attn_fwd", dict(Hkv=0),
     'lbfa_attn_fwd: empty tensor'),
    ("lbfa_attn_fwd", dict(D=96),
     'Unsupported head_dim: 96'),
    ("lbfa_attn_fwd", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_attn_fwd", dict(v_dtype=1),
     'lbfa_attn_fwd: v must be float16 (cast bfloat16 with lbfa_cast_bf16_to_f16, the `v.to(float16)` of the reference) or e4m3'),
    ("lbfa_attn_fwd", dict(v_dtype=7),
     'lbfa_attn_fwd: bad v_dtype 7'),
    ("lbfa_attn_fwd", dict(o_dtype=2),
     'lbfa_attn_fwd: bad o_dtype 2'),
    ("lbfa_attn_fwd", dict(v_dtype=2),
     'lbfa_attn_fwd: v_scale is required for fp8 V'),
    ("lbfa_attn_fwd", dict(sv=None),
     'lbfa_attn_fwd: strides_v is required for fp16 V'),
    ("lbfa_attn_fwd", dict(causal=1, Sk=16),
     'qo_len and kv_len must be equal for causal attention'),
    ("lbfa_attn_fwd", dict(q=A(8)),
     'lbfa_attn_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd", dict(k=A(8)),
     'lbfa_attn_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd", dict(v=A(8)),
     'lbfa_attn_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd", dict(o=A(4)),
     'lbfa_attn_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd", dict(sq=(1024, 512, 72)),
     'lbfa_attn_fwd: q/k strides must be multiples of 16 elements'),
    ("lbfa_attn_fwd", dict(sk=(1024, 512, 72)),
     'lbfa_attn_fwd: q/k strides must be multiples of 16 elements'),
    ("lbfa_attn_fwd", dict(sv=(1024, 512, 60)),
     'lbfa_attn_fwd: v strides must be multiples of 8 elements'),
    ("lbfa_attn_fwd", dict(so=(1024, 512, 62)),
     'lbfa_attn_fwd: o strides must be multiples of 4 elements'),
    ("lbfa_attn_fwd", dict(sq=(1024, 512, 15790336)),
     'lbfa_attn_fwd: per-(batch,head) operand window exceeds 2 GiB (seq stride x length too large)'),
    ("lbfa_attn_fwd", dict(sq=(1024, 512, 15790320), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd: grid too large'),
    ("lbfa_attn_fwd", dict(sk=(1024, 512, 15790336)),
     'lbfa_attn_fwd: per-(batch,head) operand window exceeds 2 GiB (seq stride x length too large)'),
    ("lbfa_attn_fwd", dict(sk=(1024, 512, 15790320), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd: grid too large'),
    ("lbfa_attn_fwd", dict(sv=(1024, 512, 7895160)),
     'lbfa_attn_fwd: per-(batch,head) operand window exceeds 2 GiB (seq stride x length too large)'),
    ("lbfa_attn_fwd", dict(sv=(1024, 512, 7895152), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd: grid too large'),
    ("lbfa_attn_fwd", dict(v_dtype=2, v_scale=A(0), sv=None, sk=(1024, 512, 16), Sk=33554304),
     'lbfa_attn_fwd: per-(batch,head) operand window exceeds 2 GiB (seq stride x length too large)'),
    ("lbfa_attn_fwd", dict(v_dtype=2, v_scale=A(0), sv=None, sk=(1024, 512, 16), Sk=33554303, B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd: grid too large'),
    ("lbfa_attn_fwd", dict(B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd: grid too large'),
    ("lbfa_forward", dict(q=None),
     'lbfa_forward: null pointer'),
    ("lbfa_forward", dict(workspace=None),
     'lbfa_forward: null pointer'),
    ("lbfa_forward", dict(sv=None),
     'lbfa_forward: null pointer'),
    ("lbfa_forward", dict(B=0),
     'lbfa_forward: empty tensor'),
    ("lbfa_forward", dict(Sk=0),
     'lbfa_forward: empty tensor'),
    ("lbfa_forward", dict(D=36),
     'Unsupported head_dim: 36'),
    ("lbfa_forward", dict(D=136),
     'Unsupported head_dim: 136'),
    ("lbfa_forward", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_forward", dict(workspace_bytes=16),
     'lbfa_forward: workspace too small (16 < 2560)'),
    ("lbfa_forward", dict(workspace=A(8)),
     'lbfa_forward: workspace must be 16-byte aligned'),
    ("lbfa_forward", dict(dtype=5),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_forward", dict(q_qmax=15),
     'lbfa_forward: q_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward", dict(k_qmax=15),
     'lbfa_forward: k_qmax must be 127 (int8) or 7 (int4 range), got 15'),
    ("lbfa_forward", dict(q=A(8)),
     'lbfa_forward: q must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(sq=(1024, 512, 60)),
     'lbfa_forward: q must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(k=A(8)),
     'lbfa_forward: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(sk=(1024, 512, 60)),
     'lbfa_forward: k must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(v=A(8)),
     'lbfa_forward: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(sv=(1024, 512, 60)),
     'lbfa_forward: v must be 16-byte aligned with strides that are multiples of 8 elements'),
    ("lbfa_forward", dict(o=A(4)),
     'lbfa_forward: o must be 8-byte aligned with strides that are multiples of 4 elements'),
    ("lbfa_forward", dict(so=(1024, 512, 62)),
     'lbfa_forward: o must be 8-byte aligned with strides that are multiples of 4 elements'),
    ("lbfa_forward", dict(causal=1, Sk=16),
     'qo_len and kv_len must be equal for causal attention'),
    ("lbfa_forward", dict(sq=(1024, 512, 7895160)),
     'lbfa_forward: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_forward", dict(sq=(1024, 512, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_forward", dict(sv=(1024, 512, 7895160)),
     'lbfa_forward: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_forward", dict(sv=(1024, 512, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_forward", dict(Sk=33554303, workspace_bytes=4611686018427387904, sv=(1024, 512, 8)),
     'lbfa_forward: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_forward", dict(Sk=33554302, workspace_bytes=4611686018427387904, sv=(1024, 512, 8), B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_forward", dict(Sk=33554303, workspace_bytes=4611686018427387904, pv_fp8=1),
     'lbfa_forward: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_forward", dict(Sk=33554302, workspace_bytes=4611686018427387904, pv_fp8=1, sv=(1024, 512, 8796093022208), B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_forward", dict(D=40, sq=(1024, 512, 7895160)),
     'lbfa_forward: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_forward", dict(D=40, sq=(1024, 512, 7895152), workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_forward", dict(workspace_bytes=4611686018427387904, B=65536, Hq=65536, Hkv=1),
     'lbfa_forward: grid too large'),
    ("lbfa_sdpa_fwd", dict(q=None),
     'lbfa_sdpa_fwd: null pointer'),
    ("lbfa_sdpa_fwd", dict(so=None),
     'lbfa_sdpa_fwd: null pointer'),
    ("lbfa_sdpa_fwd", dict(Sq=0),
     'lbfa_sdpa_fwd: empty tensor'),
    ("lbfa_sdpa_fwd", dict(D=36),
     'Unsupported head_dim: 36'),
    ("lbfa_sdpa_fwd", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_sdpa_fwd", dict(dtype=2),
     'Input tensors must be in dtype of float16 or bfloat16'),
    ("lbfa_sdpa_fwd", dict(causal=1, Sk=16),
     'qo_len and kv_len must be equal for causal attention'),
    ("lbfa_sdpa_fwd", dict(sm_scale=0.0),
     'lbfa_sdpa_fwd: sm_scale must be positive (the row maximum is tracked on the unscaled scores)'),
    ("lbfa_sdpa_fwd", dict(sm_scale=float("nan")),
     'lbfa_sdpa_fwd: sm_scale must be positive (the row maximum is tracked on the unscaled scores)'),
    ("lbfa_sdpa_fwd", dict(q=A(8)),
     'lbfa_sdpa_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_sdpa_fwd", dict(v=A(8)),
     'lbfa_sdpa_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_sdpa_fwd", dict(o=A(4)),
     'lbfa_sdpa_fwd: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_sdpa_fwd", dict(sq=(1024, 512, 60)),
     'lbfa_sdpa_fwd: q/k/v strides must be multiples of 8 elements'),
    ("lbfa_sdpa_fwd", dict(sv=(1024, 512, 60)),
     'lbfa_sdpa_fwd: q/k/v strides must be multiples of 8 elements'),
    ("lbfa_sdpa_fwd", dict(so=(1024, 512, 62)),
     'lbfa_sdpa_fwd: o strides must be multiples of 4 elements'),
    ("lbfa_sdpa_fwd", dict(sq=(1024, 512, 7895160)),
     'lbfa_sdpa_fwd: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_sdpa_fwd", dict(sq=(1024, 512, 7895152), B=65536, Hq=65536, Hkv=1),
     'lbfa_sdpa_fwd: grid too large'),
    ("lbfa_sdpa_fwd", dict(sk=(1024, 512, 7895160)),
     'lbfa_sdpa_fwd: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_sdpa_fwd", dict(sk=(1024, 512, 7895152), B=65536, Hq=65536, Hkv=1),
     'lbfa_sdpa_fwd: grid too large'),
    ("lbfa_sdpa_fwd", dict(sv=(1024, 512, 7895160)),
     'lbfa_sdpa_fwd: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_sdpa_fwd", dict(sv=(1024, 512, 7895152), B=65536, Hq=65536, Hkv=1),
     'lbfa_sdpa_fwd: grid too large'),
    ("lbfa_sdpa_fwd", dict(D=40, sq=(1024, 512, 7895168)),
     'lbfa_sdpa_fwd: per-(batch,head) operand window exceeds 2 GiB'),
    ("lbfa_sdpa_fwd", dict(D=40, sq=(1024, 512, 7895160), B=65536, Hq=65536, Hkv=1),
     'lbfa_sdpa_fwd: grid too large'),
    ("lbfa_sdpa_fwd", dict(B=65536, Hq=65536, Hkv=1),
     'lbfa_sdpa_fwd: grid too large'),
    ("lbfa_attn_fwd_varlen", dict(cu_qscale=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(cu_kscale=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(q=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(q_scale=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(cu_k=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(sv=None),
     'lbfa_attn_fwd_varlen: null pointer'),
    ("lbfa_attn_fwd_varlen", dict(B=0),
     'lbfa_attn_fwd_varlen: empty batch'),
    ("lbfa_attn_fwd_varlen", dict(max_k=0),
     'lbfa_attn_fwd_varlen: empty batch'),
    ("lbfa_attn_fwd_varlen", dict(D=96),
     'Unsupported head_dim: 96'),
    ("lbfa_attn_fwd_varlen", dict(Hq=3),
     'num_qo_heads (3) must be divisible by num_kv_heads (2)'),
    ("lbfa_attn_fwd_varlen", dict(v_dtype=1),
     'lbfa_attn_fwd_varlen: v must be float16 (cast bfloat16 with lbfa_cast_bf16_to_f16)'),
    ("lbfa_attn_fwd_varlen", dict(v_dtype=2),
     'lbfa_attn_fwd_varlen: v must be float16 (cast bfloat16 with lbfa_cast_bf16_to_f16)'),
    ("lbfa_attn_fwd_varlen", dict(o_dtype=2),
     'lbfa_attn_fwd_varlen: bad o_dtype 2'),
    ("lbfa_attn_fwd_varlen", dict(q=A(8)),
     'lbfa_attn_fwd_varlen: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd_varlen", dict(o=A(4)),
     'lbfa_attn_fwd_varlen: q/k/v must be 16-byte aligned and o 8-byte aligned'),
    ("lbfa_attn_fwd_varlen", dict(sq=(72, 128)),
     'lbfa_attn_fwd_varlen: q/k strides must be multiples of 16 elements'),
    ("lbfa_attn_fwd_varlen", dict(sk=(72, 128)),
     'lbfa_attn_fwd_varlen: q/k strides must be multiples of 16 elements'),
    ("lbfa_attn_fwd_varlen", dict(sv=(64, 60)),
     'lbfa_attn_fwd_varlen: v strides must be multiples of 8 elements'),
    ("lbfa_attn_fwd_varlen", dict(so=(62, 128)),
     'lbfa_attn_fwd_varlen: o strides must be multiples of 4 elements'),
    ("lbfa_attn_fwd_varlen", dict(sq=(64, 15790336)),
     'lbfa_attn_fwd_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_attn_fwd_varlen", dict(sq=(64, 15790320), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd_varlen: grid too large'),
    ("lbfa_attn_fwd_varlen", dict(sk=(64, 15790336)),
     'lbfa_attn_fwd_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_attn_fwd_varlen", dict(sk=(64, 15790320), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd_varlen: grid too large'),
    ("lbfa_attn_fwd_varlen", dict(sv=(64, 7895160)),
     'lbfa_attn_fwd_varlen: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)'),
    ("lbfa_attn_fwd_varlen", dict(sv=(64, 7895152), B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd_varlen: grid too large'),
    ("lbfa_attn_fwd_varlen", dict(B=65536, Hq=65536, Hkv=1),
     'lbfa_attn_fwd_varlen: grid too large'),
]


# value of every workspace-size function on a grid of shapes, invalid ones (-> 0) included: (arguments, bytes)
WORKSPACE_SIZES = {
    "lbfa_mean_seq_workspace_bytes": [
        ((1, 2, 8, 64), 1024),
        ((2, 4, 300, 128), 16384),
        ((1, 2, 20000, 64), 20480),
        ((3, 2, 70000, 128), 423936),
        ((1, 2, 8, 40), 640),
        ((0, 2, 8, 64), 0),
        ((1, 2, 8, 0), 0),
    ],
    "lbfa_v_fp8_bytes": [
        ((1, 2, 8, 64), 8704),
        ((2, 4, 300, 128), 331776),
        ((1, 2, 20000, 64), 2564608),
        ((3, 2, 70000, 128), 53775360),
        ((1, 2, 8, 40), 5440),
        ((0, 2, 8, 64), 0),
        ((1, 2, 8, 0), 0),
    ],
    "lbfa_forward_workspace_bytes_dt": [
        ((2, 8, 2, 300, 1000, 40, 0, 0, 0, 0), 264960),
        ((2, 8, 2, 300, 1000, 40, 0, 0, 1, 1), 264960),
        ((2, 8, 2, 300, 1000, 40, 0, 1, 1, 0), 529152),
        ((2, 8, 2, 300, 1000, 40, 0, 1, 0, 1), 529152),
        ((2, 8, 2, 300, 1000, 40, 1, 0, 0, 0), 776960),
        ((2, 8, 2, 300, 1000, 40, 1, 0, 1, 1), 776960),
        ((2, 8, 2, 300, 1000, 40, 1, 1, 1, 0), 529152),
        ((2, 8, 2, 300, 1000, 40, 1, 1, 0, 1), 529152),
        ((1, 4, 4, 128, 20000, 40, 0, 0, 0, 0), 5166592),
        ((1, 4, 4, 128, 20000, 40, 0, 0, 1, 1), 5166592),
        ((1, 4, 4, 128, 20000, 40, 0, 1, 1, 0), 10296832),
        ((1, 4, 4, 128, 20000, 40, 0, 1, 0, 1), 10296832),
        ((1, 4, 4, 128, 20000, 40, 1, 0, 0, 0), 15406592),
        ((1, 4, 4, 128, 20000, 40, 1, 0, 1, 1), 15406592),
        ((1, 4, 4, 128, 20000, 40, 1, 1, 1, 0), 10296832),
        ((1, 4, 4, 128, 20000, 40, 1, 1, 0, 1), 10296832),
        ((2, 8, 2, 300, 1000, 64, 0, 0, 0, 0), 264960),
        ((2, 8, 2, 300, 1000, 64, 0, 0, 1, 1), 264960),
        ((2, 8, 2, 300, 1000, 64, 0, 1, 1, 0), 529152),
        ((2, 8, 2, 300, 1000, 64, 0, 1, 0, 1), 529152),
        ((2, 8, 2, 300, 1000, 64, 1, 0, 0, 0), 776960),
        ((2, 8, 2, 300, 1000, 64, 1, 0, 1, 1), 776960),
        ((2, 8, 2, 300, 1000, 64, 1, 1, 1, 0), 529152),
        ((2, 8, 2, 300, 1000, 64, 1, 1, 0, 1), 529152),
        ((1, 4, 4, 128, 20000, 64, 0, 0, 0, 0), 5166592),
        ((1, 4, 4, 128, 20000, 64, 0, 0, 1, 1), 5166592),
        ((1, 4, 4, 128, 20000, 64, 0, 1, 1, 0), 10296832),
        ((1, 4, 4, 128, 20000, 64, 0, 1, 0, 1), 10296832),
        ((1, 4, 4, 128, 20000, 64, 1, 0, 0, 0), 15406592),
        ((1, 4, 4, 128, 20000, 64, 1, 0, 1, 1), 15406592),
        ((1, 4, 4, 128, 20000, 64, 1, 1, 1, 0), 10296832),
        ((1, 4, 4, 128, 20000, 64, 1, 1, 0, 1), 10296832),
        ((2, 8, 2, 300, 1000, 96, 0, 0, 0, 0), 529664),
        ((2, 8, 2, 300, 1000, 96, 0, 0, 1, 1), 529664),
        ((2, 8, 2, 300, 1000, 96, 0, 1, 1, 0), 1058048),
        ((2, 8, 2, 300, 1000, 96, 0, 1, 0, 1), 1058048),
        ((2, 8, 2, 300, 1000, 96, 1, 0, 0, 0), 1553664),
        ((2, 8, 2, 300, 1000, 96, 1, 0, 1, 1), 1553664),
        ((2, 8, 2, 300, 1000, 96, 1, 1, 1, 0), 1058048),
        ((2, 8, 2, 300, 1000, 96, 1, 1, 0, 1), 1058048),
        ((1, 4, 4, 128, 20000, 96, 0, 0, 0, 0), 10328064),
        ((1, 4, 4, 128, 20000, 96, 0, 0, 1, 1), 10328064),
        ((1, 4, 4, 128, 20000, 96, 0, 1, 1, 0), 20588544),
        ((1, 4, 4, 128, 20000, 96, 0, 1, 0, 1), 20588544),
        ((1, 4, 4, 128, 20000, 96, 1, 0, 0, 0), 30808064),
        ((1, 4, 4, 128, 20000, 96, 1, 0, 1, 1), 30808064),
        ((1, 4, 4, 128, 20000, 96, 1, 1, 1, 0), 20588544),
        ((1, 4, 4, 128, 20000, 96, 1, 1, 0, 1), 20588544),
        ((2, 8, 2, 300, 1000, 128, 0, 0, 0, 0), 529664),
        ((2, 8, 2, 300, 1000, 128, 0, 0, 1, 1), 529664),
        ((2, 8, 2, 300, 1000, 128, 0, 1, 1, 0), 1058048),
        ((2, 8, 2, 300, 1000, 128, 0, 1, 0, 1), 1058048),
        ((2, 8, 2, 300, 1000, 128, 1, 0, 0, 0), 1553664),
        ((2, 8, 2, 300, 1000, 128, 1, 0, 1, 1), 1553664),
        ((2, 8, 2, 300, 1000, 128, 1, 1, 1, 0), 1058048),
        ((2, 8, 2, 300, 1000, 128, 1, 1, 0, 1), 1058048),
        ((1, 4, 4, 128, 20000, 128, 0, 0, 0, 0), 10328064),
        ((1, 4, 4, 128, 20000, 128, 0, 0, 1, 1), 10328064),
        ((1, 4, 4, 128, 20000, 128, 0, 1, 1, 0), 20588544),
        ((1, 4, 4, 128, 20000, 128, 0, 1, 0, 1), 20588544),
        ((1, 4, 4, 128, 20000, 128, 1, 0, 0, 0), 30808064),
        ((1, 4, 4, 128, 20000, 128, 1, 0, 1, 1), 30808064),
        ((1, 4, 4, 128, 20000, 128, 1, 1, 1, 0), 20588544),
        ((1, 4, 4, 128, 20000, 128, 1, 1, 0, 1), 20588544),
        ((0, 2, 2, 8, 8, 64, 0, 0, 1, 0), 0),
        ((1, 2, 2, 8, 8, 36, 0, 0, 1, 0), 0),
        ((1, 2, 2, 8, 8, 136, 1, 0, 1, 0), 0),
    ],
    "lbfa_forward_workspace_bytes": [
        ((2, 8, 2, 300, 1000, 40, 0, 1, 0), 776960),
        ((2, 8, 2, 300, 1000, 40, 1, 1, 1), 529152),
        ((1, 4, 4, 128, 20000, 40, 0, 1, 0), 15406592),
        ((1, 4, 4, 128, 20000, 40, 1, 1, 1), 10296832),
        ((2, 8, 2, 300, 1000, 64, 0, 1, 0), 776960),
        ((2, 8, 2, 300, 1000, 64, 1, 1, 1), 529152),
        ((1, 4, 4, 128, 20000, 64, 0, 1, 0), 15406592),
        ((1, 4, 4, 128, 20000, 64, 1, 1, 1), 10296832),
        ((2, 8, 2, 300, 1000, 96, 0, 1, 0), 1553664),
        ((2, 8, 2, 300, 1000, 96, 1, 1, 1), 1058048),
        ((1, 4, 4, 128, 20000, 96, 0, 1, 0), 30808064),
        ((1, 4, 4, 128, 20000, 96, 1, 1, 1), 20588544),
        ((2, 8, 2, 300, 1000, 128, 0, 1, 0), 1553664),
        ((2, 8, 2, 300, 1000, 128, 1, 1, 1), 1058048),
        ((1, 4, 4, 128, 20000, 128, 0, 1, 0), 30808064),
        ((1, 4, 4, 128, 20000, 128, 1, 1, 1), 20588544),
    ],
}


def test_single_fault_messages(lib):
    check_table(lib, SINGLE_FAULT)


def test_workspace_sizes_pinned(lib):
    for fn, rows in WORKSPACE_SIZES.items():
        for args, size in rows:
            assert getattr(lib, fn)(*args) == size, (fn, args)
