"""Keyword-argument callers for the validating C-ABI entry points, shared by the CPU-side ABI tests.

`call(lib, name, **overrides)` makes one call with a small valid problem in which only the overridden arguments differ, and
returns (status, lbfa_last_error()).  Every table entry of the tests changes exactly one thing that the entry point must refuse
BEFORE its first launch, so nothing here needs a GPU - and nothing here may be called with no fault at all.

Argument values: `A(off)` is a pointer `off` bytes past a 256-byte aligned scratch buffer, `None` a null pointer, a tuple of
3 / 2 integers a stride array {batch, head, seq} / {head, token}, everything else is passed as it is.
"""
import ctypes
import os

import pytest

from lowbit_quant_fa2_paddle_amd import _lib


class A:
    def __init__(self, off=0):
        self.off = off

    def __repr__(self):
        return f"A({self.off})"


P = A(0)
S3 = (1024, 512, 64)   # [B, H, S, D] contiguous for H = 2, S = 8, D = 64
S2 = (64, 128)         # [total, H, D] contiguous for H = 2, D = 64
WS = 1 << 15           # more than any default problem's workspace
_F16 = _lib.LBFA_F16

_DENSE = dict(B=1, Hq=2, Hkv=2, Sq=8, Sk=8, D=64)
_PACKED = dict(B=1, Hq=2, Hkv=2, total_q=8, total_k=8, max_q=8, max_k=8, D=64)
_ST4 = dict(sq=S3, sk=S3, sv=S3, so=S3)
_ST4P = dict(sq=S2, sk=S2, sv=S2, so=S2)
_ONE_CALL = dict(sm_scale=0.125, q_qmax=127, k_qmax=127)

# name -> arguments in ABI order with the value of the valid default problem
DEFAULTS = {
    "lbfa_absmax": dict(x=P, dtype=_F16, out=P, B=1, H=2, S=8, D=64, sx=S3, stream=None),
    "lbfa_mean_seq": dict(x=P, dtype=_F16, mean_out=P, workspace=P, workspace_bytes=WS, B=1, H=2, S=8, D=64, sx=S3, stream=None),
    "lbfa_quant_per_block": dict(x=P, dtype=_F16, mean=None, mean_group=1, out=P, scale=P, sm_scale=1.0, qmax=127, blk=128,
                                 B=1, H=2, S=8, D=64, sx=S3, sout=S3, rowdot_vec=None, rowdot_group=1, rowdot_out=None, stream=None),
    "lbfa_quant_per_block_varlen": dict(x=P, dtype=_F16, mean=None, mean_group=1, out=P, scale=P, cu=P, cu_scale=P, sm_scale=1.0,
                                        qmax=127, blk=128, B=1, max_seqlen=8, H=2, D=64, sx=S2, sout=S2, stream=None),
    "lbfa_quant_v_fp8": dict(v=P, dtype=_F16, v_fp8=P, v_scale=P, B=1, H=2, S=8, D=64, sv=S3, stream=None),
    "lbfa_cast_bf16_to_f16": dict(src=P, dst=P, B=1, H=2, S=8, D=64, ssrc=S3, sdst=S3, stream=None),
    "lbfa_attn_fwd": dict(q=P, k=P, v=P, v_dtype=_F16, o=P, o_dtype=_F16, lse=None, q_scale=P, k_scale=P, v_scale=None,
                          **_DENSE, **_ST4, causal=0, stream=None),
    "lbfa_forward": dict(q=P, k=P, v=P, dtype=_F16, o=P, lse=None, workspace=P, workspace_bytes=WS, **_DENSE, **_ST4,
                         **_ONE_CALL, pv_fp8=0, causal=0, smooth_k=1, stream=None),
    "lbfa_sdpa_fwd": dict(q=P, k=P, v=P, dtype=_F16, o=P, lse=None, **_DENSE, **_ST4, sm_scale=0.125, causal=0, stream=None),
    "lbfa_attn_fwd_varlen": dict(q=P, k=P, v=P, v_dtype=_F16, o=P, o_dtype=_F16, q_scale=P, k_scale=P, cu_q=P, cu_k=P,
                                 cu_qscale=P, cu_kscale=P, B=1, Hq=2, Hkv=2, max_q=8, max_k=8, D=64, **_ST4P, causal=0, stream=None),
    "lbfa_forward_varlen": dict(q=P, k=P, v=P, dtype=_F16, o=P, cu_q=P, cu_k=P, workspace=P, workspace_bytes=WS, **_PACKED,
                                **_ST4P, **_ONE_CALL, causal=0, smooth_k=1, stream=None),
    "lbfa_forward_varlen_lse": dict(q=P, k=P, v=P, dtype=_F16, o=P, lse=P, cu_q=P, cu_k=P, workspace=P, workspace_bytes=WS,
                                    **_PACKED, **_ST4P, **_ONE_CALL, causal=0, smooth_k=1, stream=None),
    "lbfa_backward": dict(q=P, k=P, v=P, o=P, dout=P, dtype=_F16, lse=P, dlse=None, dq=P, dk=P, dv=P, workspace=P,
                          workspace_bytes=WS, **_DENSE, **_ST4, sdout=S3, sdq=S3, sdk=S3, sdv=S3, **_ONE_CALL, causal=0,
                          smooth_k=1, stream=None),
    "lbfa_backward_varlen": dict(q=P, k=P, v=P, o=P, dout=P, dtype=_F16, lse=P, dlse=None, dq=P, dk=P, dv=P, cu_q=P, cu_k=P,
                                 workspace=P, workspace_bytes=WS, **_PACKED, **_ST4P, sdout=S2, sdq=S2, sdk=S2, sdv=S2,
                                 **_ONE_CALL, causal=0, smooth_k=1, stream=None),
}


# ---- the KV cache: B 1, Hkv 2, D 64; an append of T 8 rows; a decode of Sq 8 x Hq 4 over 128 keys (4 pages of 64, 2 slots of up
# to 2 pages); a cached prefill of Sq 200 (two Q blocks) over 256 keys (8 pages of 128).  Argument names are the header's.
def _append(table, extent):
    return dict(k_new=P, v_new=P, dtype=_F16, new_lens=None, km=P, k_codes=P, k_scale=P, v_cache=P, k_tail=P, seqlens=P, **table,
                B=1, Hkv=2, T=8, D=64, **extent, sk=S3, sv=S3, k_qmax=127, stream=None)


def _read(lens, table, Sq, extent, max_seqlen_k, workspace_bytes, causal):
    sq = (4 * Sq * 64, Sq * 64, 64)  # [B, Hq 4, Sq, D 64] contiguous
    return dict(q=P, dtype=_F16, k_codes=P, k_scale=P, v_cache=P, km=P, seqlens=P, **lens, **table, o=P, lse=None, workspace=P,
                workspace_bytes=workspace_bytes, B=1, Hq=4, Hkv=2, Sq=Sq, D=64, **extent, max_seqlen_k=max_seqlen_k, num_splits=2,
                sq=sq, so=sq, sm_scale=0.125, q_qmax=127, causal=causal, stream=None)


_TABLE = dict(block_table=P, slots=None)
POOL = dict(num_slots=2, num_pages=4, page_size=64, max_pages_per_seq=2)
PREFILL_POOL = dict(num_slots=2, num_pages=8, page_size=128, max_pages_per_seq=2)
PREFILL_WS = 1 << 20
DEFAULTS.update({
    "lbfa_kvcache_mean": dict(k_new=P, dtype=_F16, new_lens=P, km=P, B=1, Hkv=2, T=8, D=64, sk=S3, stream=None),
    "lbfa_kvcache_append": _append({}, dict(capacity=128)),
    "lbfa_kvcache_paged_append": _append(_TABLE, POOL),
    "lbfa_decode": _read({}, {}, 8, dict(capacity=128), 128, WS, 0),
    "lbfa_decode_paged": _read({}, _TABLE, 8, POOL, 128, WS, 0),
    "lbfa_prefill": _read(dict(q_lens=P), {}, 200, dict(capacity=256), 256, PREFILL_WS, 1),
    "lbfa_prefill_paged": _read(dict(q_lens=None), _TABLE, 200, PREFILL_POOL, 256, PREFILL_WS, 1),
})
# the fp8 V cache: each entry point is its sibling with v_scale behind v_cache (as _lib.SIGNATURES derives them)
V8 = [name for name in DEFAULTS if name + "_v8" in _lib.SIGNATURES]
for _name in V8:
    DEFAULTS[_name + "_v8"] = {k: v for key, val in DEFAULTS[_name].items()
                               for k, v in ((key, val),) + ((("v_scale", P),) if key == "v_cache" else ())}

_buf = ctypes.create_string_buffer(1 << 16)
_BASE = (ctypes.addressof(_buf) + 255) & ~255


def _arg(v):
    if isinstance(v, A):
        return _BASE + v.off
    if isinstance(v, tuple):
        return _lib.strides3(v) if len(v) == 3 else _lib.strides2(v)
    return v


@pytest.fixture(scope="module")
def lib():
    """the built library (built first in a fresh tree); the ABI test files import this fixture"""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def call(lib, name, **overrides):
    """-> (status, message) of `name` on its default problem with `overrides` applied; at least one override is required"""
    args = dict(DEFAULTS[name])
    assert overrides and set(overrides) <= set(args), (name, overrides)
    args.update(overrides)
    st = getattr(lib, name)(*[_arg(v) for v in args.values()])
    return st, lib.lbfa_last_error().decode()


def check_table(lib, table):
    """every (name, overrides, message) of `table`: LBFA_EINVAL and exactly that text"""
    for name, overrides, message in table:
        st, msg = call(lib, name, **overrides)
        assert st == _lib.LBFA_EINVAL, (name, overrides, st, msg)
        assert msg == message, (name, overrides, msg)


# ---- GPU side: the same keyword callers on real device pointers -----------------------------------------------------------
def call_gpu(lib, name, **kwargs):
    """One launching call of `name` with EVERY argument given by keyword (the names of DEFAULTS, any order): device
    pointers as integers or None, stride arrays as tuples.  Nothing is taken from the default problem - its pointers are host
    scratch - so a missing or misspelt argument is an error here, never a launch.  Raises as the front end does on a non-zero
    status."""
    order = tuple(DEFAULTS[name])
    assert set(kwargs) == set(order), (name, sorted(set(order) ^ set(kwargs)))
    assert not any(isinstance(v, A) for v in kwargs.values()), name
    _lib.check(getattr(lib, name)(*[_arg(kwargs[k]) for k in order]), lib)
