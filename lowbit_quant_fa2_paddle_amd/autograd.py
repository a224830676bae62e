"""Autograd for the attention operators (torch only): a `torch.autograd.Function` whose forward is the operator's own forward
(the same `lbfa_forward` / `lbfa_sdpa_fwd` call, with an LSE buffer) and whose backward is one `lbfa_backward` call; for packed
batches (`sageattn_varlen`) the same with `lbfa_forward_varlen_lse` and `lbfa_backward_varlen`.

Straight-through on the quantiser: the backward recomputes the forward's own P from the same codes and scales and from the
returned LSE, and forms dq, dk, dv from the un-quantised 16-bit q, k, v (include/lowbit_fa.h, DESIGN.md "Backward").
The operators route here only when grad mode is on and q, k or v requires grad; every other call takes the unchanged path.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from . import quant_per_block as _qpb


def _kernel_operand(t, D):
    """last-dim contiguous, zero-padded to D channels, 16-byte aligned with strides that are multiples of 8 elements"""
    if t.stride(-1) != 1:
        t = t.contiguous()
    if t.shape[-1] != D:
        t = F.pad(t, (0, D - t.shape[-1]))
    if t.data_ptr() % 16 or any(s % 8 for s in t.stride()[:3]):
        t = t.contiguous()
    return t


def _pad_operands(q, k, v, o, do):
    """-> (D, kernel operands of q, k, v, o, dO): the head dim zero-padded to the D = 64 / 128 the backward kernels run on"""
    if do is None:
        do = torch.zeros_like(o)
    D = 64 if q.shape[-1] <= 64 else 128
    return D, tuple(_kernel_operand(t, D) for t in (q, k, v, o, do.to(o.dtype)))


def _run_backward(fn, workspace_bytes, shape, cu, st, D, operands, lse, dlse, cfg, Dg):
    """What the dense and the packed backward share once the problem is described: gradient buffers, dLSE as contiguous fp32, the
    workspace, the dtype code, the call and the trim back to the caller's head dim Dg.  `fn` / `workspace_bytes`: the entry
    point and its size query; `shape`: their integer arguments before D; `cu`: the offset tables of a packed batch (else empty);
    `st(t)`: the stride array of a tensor.  -> (dq, dk, dv)"""
    is_causal, sm_scale, smooth_k, q_qmax, k_qmax = cfg
    qp, kp, vp = operands[:3]
    # written completely by the kernels (packed batch: tokens outside every sequence get zeros there)
    dq, dk, dv = (torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (qp, kp, vp))
    if dlse is not None:
        dlse = dlse.to(torch.float32).contiguous()
    ws_bytes = workspace_bytes(*shape, D, q_qmax, 1 if smooth_k else 0)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=qp.device)
    code = _lib.LBFA_F16 if qp.dtype == torch.float16 else _lib.LBFA_BF16
    with torch.cuda.device(qp.device):
        _lib.check(fn(*(t.data_ptr() for t in operands), code, lse.data_ptr(), dlse.data_ptr() if dlse is not None else None,
                      dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), *(t.data_ptr() for t in cu), ws.data_ptr(), ws_bytes, *shape, D,
                      *(st(t) for t in operands), st(dq), st(dk), st(dv), float(sm_scale), int(q_qmax), int(k_qmax),
                      1 if is_causal else 0, 1 if smooth_k else 0, torch.cuda.current_stream(qp.device).cuda_stream))
    return (dq[..., :Dg], dk[..., :Dg], dv[..., :Dg]) if D != Dg else (dq, dk, dv)


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, forward, cfg):
        # runs with grad mode off: `forward` takes the operator's plain path
        o, lse = forward(q, k, v)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, o, lse)
        return o, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, do, dlse):
        q, k, v, o, lse = ctx.saved_tensors
        layout, *cfg = ctx.cfg
        if do is None and dlse is None:
            return None, None, None, None, None
        D, operands = _pad_operands(q, k, v, o, do)
        qp, kp = operands[:2]
        (B, Hq, Sq), _ = _qpb._bhs(qp.shape, qp.stride(), layout)
        (_, Hkv, Sk), _ = _qpb._bhs(kp.shape, kp.stride(), layout)
        st = lambda t: _lib.strides3(_qpb._bhs(t.shape, t.stride(), layout)[1])
        lib = _lib.load()
        dq, dk, dv = _run_backward(lib.lbfa_backward, lib.lbfa_backward_workspace_bytes, (B, Hq, Hkv, Sq, Sk), (), st, D, operands,
                                   lse, dlse, cfg, q.shape[-1])
        return dq, dk, dv, None, None


def attention(q, k, v, forward, *, tensor_layout, is_causal, sm_scale, smooth_k, q_qmax, k_qmax):
    """(o, lse) of `forward(q, k, v)` (the operator with return_lse=True) with a backward through `lbfa_backward`.
    q_qmax = k_qmax = 0: un-quantised scores (flash_attn_fp16)."""
    return _AttentionFn.apply(q, k, v, forward, (tensor_layout, is_causal, float(sm_scale), bool(smooth_k), q_qmax, k_qmax))


class _VarlenAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, forward, cfg):
        # runs with grad mode off: `forward` takes the plain packed path with an LSE [Hq, total_q]
        o, lse = forward(q, k, v)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
        return o, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, do, dlse):
        q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, *cfg = ctx.cfg
        if do is None and dlse is None:
            return None, None, None, None, None, None, None
        D, operands = _pad_operands(q, k, v, o, do)
        total_q, Hq, _ = operands[0].shape
        total_k, Hkv, _ = operands[1].shape
        B = cu_q.shape[0] - 1
        st = lambda t: _lib.strides2((t.stride(1), t.stride(0)))  # {head, token}
        lib = _lib.load()
        dq, dk, dv = _run_backward(lib.lbfa_backward_varlen, lib.lbfa_backward_varlen_workspace_bytes,
                                   (B, Hq, Hkv, total_q, total_k, max_q, max_k), (cu_q, cu_k), st, D, operands, lse, dlse, cfg,
                                   q.shape[-1])
        return dq, dk, dv, None, None, None, None


def varlen_attention(q, k, v, cu_q, cu_k, forward, *, max_seqlen_q, max_seqlen_k, is_causal, sm_scale, smooth_k, q_qmax, k_qmax):
    """(o, lse [Hq, total_q]) of `forward(q, k, v)` (the packed operator with an LSE) with a backward through
    `lbfa_backward_varlen`.  cu_q / cu_k: int32 device tensors [B + 1]; no gradient flows to them or to the maxima."""
    return _VarlenAttentionFn.apply(q, k, v, cu_q, cu_k, forward,
                                    (int(max_seqlen_q), int(max_seqlen_k), is_causal, float(sm_scale), bool(smooth_k), q_qmax, k_qmax))
