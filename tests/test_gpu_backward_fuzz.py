"""Seeded fuzz of the dense and packed backward (torch autograd -> lbfa_backward / lbfa_backward_varlen) against the float64
references, under both the per-tensor bound (test_gpu_backward._assert_close) and the per-element one (_grad_close,
bwd_reference.grad_bound).  Random operator, dtype, layout, causal, batch, GQA group, ragged lengths, head dim, smooth-K,
sm_scale, input distribution, operand form (contiguous; views of one fused qkv tensor; every second token; a view of the other
layout's tensor, which the host pads into a copy where the head dim is not 64 / 128), upstream gradient (random; a weight
broadcast over the batch, stride 0; that of o.sum(); every second element of a wider tensor, whose last dim the host copies -
q, k, v with a strided last dim the forward refuses) and loss (o; o and LSE; the LSE alone).

Seeds: LBFA_BWD_FUZZ_N dense (default 40), LBFA_BWD_FUZZ_N_PACKED packed (default 16); LBFA_FUZZ_SEED0 shifts both ranges."""
import math
import os

import numpy as np
import pytest

from bwd_reference import attention_backward
from bwd_varlen_reference import varlen_backward
from test_gpu_backward import _assert_close, _grad_close
from test_gpu_fuzz import _rand_cfg
from test_gpu_parity import TDT, _canon, _np, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_DENSE = int(os.environ.get("LBFA_BWD_FUZZ_N", "40"))
N_PACKED = int(os.environ.get("LBFA_BWD_FUZZ_N_PACKED", "16"))
SEED0 = int(os.environ.get("LBFA_FUZZ_SEED0", "0"))

# operator -> (function name, extra kwargs, q_qmax, k_qmax)
OPS = {
    "int8": ("lowbit_fa_qk_int8_pv_fp16_triton", {}, 127, 127),
    "int4": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 4}, 7, 7),
    "q8k4": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 8}, 127, 7),
    "fp8": ("lowbit_fa_qk_int8_pv_fp8_cuda", {}, 127, 127),
    "fp16": ("flash_attn_fp16", {}, 0, 0),
}


def _inputs(oracle, rng, c, seed):
    dist = str(rng.choice(["normal", "normal", "randint", "peaky"]))
    q, k, v = oracle.make_inputs(c["B"], c["H"], c["Sq"], c["D"], seed=seed, layout=c["layout"], dtype=c["dtype"], Hkv=c["Hkv"],
                                 Sk=c["Sk"], k_bias=c["bias"], dist="randint" if dist == "randint" else "normal")
    if dist == "peaky":
        q = oracle.to_storage(q * np.float32(6.0), c["dtype"])
    return dist, q, k, v


def _seq_dim(layout):
    return 2 if layout == "HND" else 1


def _operands(form, q, k, v, c, dev):
    """leaf tensors q, k, v with the values of the numpy arrays, in operand form `form` (falls back to contiguous where the
    form does not apply)"""
    T = TDT[c["dtype"]]
    t = lambda a: torch.from_numpy(a).to(T).to(dev)
    if form == "fused" and q.shape == k.shape:
        if c["layout"] == "NHD":  # [B, S, 3, H, D]
            qkv = torch.stack([t(q), t(k), t(v)], dim=2).requires_grad_()
            return qkv, (qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
        qkv = torch.cat([t(q), t(k), t(v)], dim=1).requires_grad_()  # [B, 3H, S, D]
        H = q.shape[1]
        return qkv, (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:])
    if form == "every_second":
        sd = _seq_dim(c["layout"])
        leaves = []
        for a in (q, k, v):
            shape = list(a.shape)
            shape[sd] *= 2
            big = torch.zeros(shape, dtype=T, device=dev)
            idx = [slice(None)] * 4
            idx[sd] = slice(None, None, 2)
            big[tuple(idx)] = t(a)
            big.requires_grad_()
            leaves.append((big, tuple(idx)))
        return [b for b, _ in leaves], tuple(b[i] for b, i in leaves)
    if form == "permuted":  # a view of the other layout's tensor: taken as is at D = 64 / 128, padded (copied) by the host else
        ts = [t(np.ascontiguousarray(np.swapaxes(a, 1, 2))).requires_grad_() for a in (q, k, v)]
        return ts, tuple(x.transpose(1, 2) for x in ts)
    ts = [t(a).requires_grad_() for a in (q, k, v)]
    return ts, tuple(ts)


@pytest.mark.parametrize("seed", range(N_DENSE))
def test_fuzz_dense_backward(oracle, dev, seed):
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(5000 + SEED0 + seed)
    c = _rand_cfg(rng)
    if c["B"] * c["H"] * c["Sq"] * c["Sk"] > 2 * 4 * 320 * 320:  # keep the float64 reference and its bound cheap
        c["B"] = 1
        c["H"] = c["Hkv"] * (1 if c["H"] // c["Hkv"] == 1 else 2)
    op = ["int8", "int4", "q8k4", "fp8", "fp16"][seed % 5]
    fn_name, extra, qq, kq = OPS[op]
    fn = getattr(lb, fn_name, None) or getattr(lb.core, fn_name)
    dist, q, k, v = _inputs(oracle, rng, c, seed)
    form = str(rng.choice(["contiguous", "fused", "every_second", "permuted"]))
    upstream = str(rng.choice(["random", "batch_broadcast", "sum", "last_dim_strided"]))
    loss_kind = str(rng.choice(["o", "o_lse", "lse"]))
    leaves, (tq, tk, tv) = _operands(form, q, k, v, c, dev)
    kw = dict(tensor_layout=c["layout"], is_causal=c["causal"], sm_scale=c["sm_scale"], return_lse=True)
    if qq:
        kw["smooth_k"] = c["smooth"]
    o, lse = fn(tq, tk, tv, **extra, **kw)
    g = torch.Generator(device="cpu").manual_seed(seed)
    T = TDT[c["dtype"]]
    if upstream == "random":
        w = torch.randn(o.shape, generator=g).to(T).to(dev)
    elif upstream == "batch_broadcast":
        w = torch.randn((1,) + tuple(o.shape[1:]), generator=g).to(T).to(dev).expand(o.shape)  # batch stride 0
    elif upstream == "sum":
        w = torch.ones((), dtype=T, device=dev).expand(o.shape)  # the gradient of o.sum()
    else:  # stride 2 in the last dim: _kernel_operand copies it
        w = torch.randn(tuple(o.shape[:-1]) + (2 * o.shape[-1],), generator=g).to(T).to(dev)[..., ::2]
        assert w.stride(-1) == 2
    wl = torch.randn(lse.shape, generator=g).to(dev) if loss_kind != "o" else None
    if loss_kind == "o":
        o.backward(w)
    elif loss_kind == "o_lse":
        torch.autograd.backward([o, lse], [w, wl])
    else:
        lse.backward(wl)
    cfg = dict(c, op=op, dist=dist, form=form, upstream=upstream, loss=loss_kind)
    if isinstance(leaves, list):
        grads = [x.grad for x in leaves]
        if form == "every_second":
            sd = _seq_dim(c["layout"])
            idx = [slice(None)] * 4
            idx[sd] = slice(None, None, 2)
            odd = [slice(None)] * 4
            odd[sd] = slice(1, None, 2)
            for x in grads:  # the tokens between the used ones get no gradient
                assert not x[tuple(odd)].any(), cfg
            grads = [x[tuple(idx)] for x in grads]
        elif form == "permuted":
            grads = [x.transpose(1, 2) for x in grads]
    else:  # fused
        G = leaves.grad
        if c["layout"] == "NHD":
            grads = [G[:, :, i] for i in range(3)]
        else:
            H = q.shape[1]
            grads = [G[:, i * H:(i + 1) * H] for i in range(3)]
    do = np.zeros(q.shape, np.float32) if loss_kind == "lse" else _np(w)
    sm = c["sm_scale"] if c["sm_scale"] is not None else 1.0 / math.sqrt(c["D"])
    L = c["layout"]
    ref = attention_backward(_canon(q, L), _canon(k, L), _canon(v, L), _canon(_np(o), L), _np(lse), _canon(do, L), sm_scale=sm,
                             is_causal=c["causal"], dtype=c["dtype"], q_qmax=qq, k_qmax=kq, smooth_k=c["smooth"] and qq != 0,
                             dlse=None if wl is None else wl.cpu().numpy(), return_bound=True)
    for what, got, a, rf, bnd in zip(("dq", "dk", "dv"), grads, (q, k, v), ref[:3], ref[3:]):
        assert got is not None and tuple(got.shape) == a.shape, (what, cfg)
        x = _canon(_np(got), L)
        _assert_close(x, rf, c["dtype"], f"{what} {cfg}")
        _grad_close(x, rf, bnd, what)


@pytest.mark.parametrize("seed", range(N_PACKED))
def test_fuzz_packed_backward(oracle, dev, seed):
    from lowbit_quant_fa2_paddle_amd import core
    rng = np.random.default_rng(6000 + SEED0 + seed)
    c = _rand_cfg(rng)
    qq, kq = [(127, 127), (7, 7), (127, 7)][seed % 3]
    n = int(rng.integers(1, 5))
    lens_q = [int(x) for x in rng.choice([1, 5, 63, 64, 65, 100, 128, 129, 250], size=n)]
    lens_k = lens_q if c["causal"] else [int(x) for x in rng.choice([1, 40, 64, 65, 192, 300], size=n)]
    q, k, v, cu_q, cu_k = oracle.make_varlen_inputs(lens_q, lens_k, c["H"], c["Hkv"], c["D"], seed=seed, dtype=c["dtype"],
                                                    k_bias=c["bias"])
    T = TDT[c["dtype"]]
    tq, tk, tv = (torch.from_numpy(a).to(T).to(dev).requires_grad_() for a in (q, k, v))
    tcq, tck = (torch.from_numpy(x).to(dev) for x in (cu_q, cu_k))
    o, lse = core._varlen_attention(tq, tk, tv, tcq, tck, max(lens_q), max(lens_k), is_causal=c["causal"], sm_scale=c["sm_scale"],
                                    smooth_k=c["smooth"], q_qmax=qq, k_qmax=kq, return_lse=True)
    loss_kind = str(rng.choice(["o", "o_lse", "lse"]))
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(o.shape, generator=g).to(T).to(dev)
    wl = torch.randn(lse.shape, generator=g).to(dev) if loss_kind != "o" else None
    if loss_kind == "o":
        o.backward(w)
    elif loss_kind == "o_lse":
        torch.autograd.backward([o, lse], [w, wl])
    else:
        lse.backward(wl)
    cfg = dict(c, lens_q=lens_q, lens_k=lens_k, qq=qq, kq=kq, loss=loss_kind)
    do = np.zeros(q.shape, np.float32) if loss_kind == "lse" else _np(w)
    ref = varlen_backward(q, k, v, _np(o), _np(lse).astype(np.float64), do, cu_q, cu_k, dtype=c["dtype"], is_causal=c["causal"],
                          sm_scale=c["sm_scale"], smooth_k=c["smooth"], q_qmax=qq, k_qmax=kq,
                          dlse=None if wl is None else wl.cpu().numpy().astype(np.float64), return_bound=True)
    for what, got, rf, bnd in zip(("dq", "dk", "dv"), (tq.grad, tk.grad, tv.grad), ref[:3], ref[3:]):
        x = _np(got)
        _assert_close(x, rf, c["dtype"], f"{what} {cfg}")
        _grad_close(x, rf, bnd, what)
