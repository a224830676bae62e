"""GPU tests of the autograd surface of the dense operators (lowbit_quant_fa2_paddle_amd/autograd.py): strided operand forms,
the dispatchers `sageattn` / `sageattn_multi_precision`, partial requires_grad, and q = k = v as one leaf.  Every comparison is
bit for bit against a plain call: the backward is deterministic and these paths must hand the kernels the same values."""
import numpy as np
import pytest

from test_gpu_parity import dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# family -> (function name, extra kwargs)
FAMILIES = {
    "int8": ("lowbit_fa_qk_int8_pv_fp16_triton", {}),
    "int4": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 4}),
    "q8k4": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 8}),
    "fp8": ("lowbit_fa_qk_int8_pv_fp8_cuda", {}),
    "fp16": ("flash_attn_fp16", {}),
}


def _fn(name):
    import lowbit_quant_fa2_paddle_amd as lb
    fn_name, extra = FAMILIES[name]
    fn = getattr(lb, fn_name, None) or getattr(lb.core, fn_name)
    return lambda *a, **kw: fn(*a, **extra, **kw)


def _grads(fn, q, k, v, w, **kw):
    """o and the gradients of (o * w).sum() with respect to fresh leaves holding the values of q, k, v"""
    leaves = [x.detach().clone().requires_grad_() for x in (q, k, v)]
    o = fn(*leaves, **kw)
    o.backward(w)
    return o.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("name", list(FAMILIES))
@pytest.mark.parametrize("form", ["fused_nhd", "fused_hnd", "every_second_token"])
def test_backward_of_strided_operands_has_the_bits_of_contiguous_ones(dev, oracle, name, form):
    """views of one fused qkv tensor ([B, S, 3, H, D] / [B, 3H, S, D]) and every second token of a longer tensor go to the
    kernels without a copy (_kernel_operand keeps them): their gradients must be the contiguous call's, bit for bit"""
    fn = _fn(name)
    B, H, S, D = 2, 4, 200, 64
    layout = "HND" if form == "fused_hnd" else "NHD"
    q, k, v = (torch.from_numpy(a).to(dev).half() for a in oracle.make_inputs(B, H, S, D, seed=31, layout=layout, k_bias=0.3))
    w = torch.randn(q.shape, generator=torch.Generator(device="cpu").manual_seed(5)).half().to(dev)
    kw = dict(tensor_layout=layout, is_causal=True)
    o_ref, g_ref = _grads(fn, q, k, v, w, **kw)
    if form == "fused_nhd":
        big = torch.stack([q, k, v], dim=2).requires_grad_()  # [B, S, 3, H, D]
        views = [big[:, :, i] for i in range(3)]
    elif form == "fused_hnd":
        big = torch.cat([q, k, v], dim=1).requires_grad_()  # [B, 3H, S, D]
        views = [big[:, i * H:(i + 1) * H] for i in range(3)]
    else:
        big = torch.zeros((3, B, 2 * S, H, D), dtype=q.dtype, device=dev)
        big[:, :, ::2] = torch.stack([q, k, v])
        big.requires_grad_()
        views = [big[i, :, ::2] for i in range(3)]
    assert all(x.stride(-1) == 1 and not x.is_contiguous() for x in views)
    o = fn(*views, **kw)
    o.backward(w)
    assert torch.equal(o.detach(), o_ref)
    if form == "fused_nhd":
        got = [big.grad[:, :, i] for i in range(3)]
    elif form == "fused_hnd":
        got = [big.grad[:, i * H:(i + 1) * H] for i in range(3)]
    else:
        got = [big.grad[i, :, ::2] for i in range(3)]
        assert not big.grad[:, :, 1::2].any()
    for a, b in zip(got, g_ref):
        assert torch.equal(a, b)


def test_sageattn_has_gradients_of_its_operator(dev, oracle):
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = (torch.from_numpy(a).to(dev).half() for a in oracle.make_inputs(1, 4, 190, 128, seed=32, Hkv=2, k_bias=0.5))
    w = torch.randn(q.shape, generator=torch.Generator(device="cpu").manual_seed(6)).half().to(dev)
    o, g = _grads(lb.sageattn, q, k, v, w, is_causal=False)
    o_ref, g_ref = _grads(lb.lowbit_fa_qk_int8_pv_fp16_triton, q, k, v, w, is_causal=False)
    assert torch.equal(o, o_ref)
    for a, b in zip(g, g_ref):
        assert a is not None and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)


@pytest.mark.parametrize("scale,branch", [(10.0, "FP16"), (3.0, "INT8"), (1.0, "INT4")])
def test_multi_precision_branch_gradients(dev, oracle, scale, branch):
    """inputs scaled so that select_quantization picks each branch in turn: the router's gradients are that branch's"""
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import core
    q, k, v = (torch.from_numpy(a * np.float32(scale)).to(dev).half()
               for a in oracle.make_inputs(1, 2, 160, 64, seed=33, layout="NHD"))
    assert core.select_quantization(q, k, v) == branch
    direct = {"FP16": lb.core.flash_attn_fp16, "INT8": lb.lowbit_fa_qk_int8_pv_fp16_triton,
              "INT4": lb.lowbit_fa_qk_int4_pv_fp16_triton}[branch]
    w = torch.randn(q.shape, generator=torch.Generator(device="cpu").manual_seed(7)).half().to(dev)
    kw = dict(tensor_layout="NHD", is_causal=True)
    o, g = _grads(lb.sageattn_multi_precision, q, k, v, w, **kw)
    o_ref, g_ref = _grads(direct, q, k, v, w, **kw)
    assert torch.equal(o, o_ref)
    for a, b in zip(g, g_ref):
        assert a is not None and torch.equal(a, b)


@pytest.mark.parametrize("name", ["int8", "fp16"])
def test_only_q_requires_grad(dev, oracle, name):
    fn = _fn(name)
    q, k, v = (torch.from_numpy(a).to(dev).to(torch.bfloat16)
               for a in oracle.make_inputs(1, 4, 150, 80, seed=34, Hkv=2, dtype="bf16"))
    w = torch.randn(q.shape, generator=torch.Generator(device="cpu").manual_seed(8)).to(torch.bfloat16).to(dev)
    _, (dq_all, _, _) = _grads(fn, q, k, v, w)
    tq = q.clone().requires_grad_()
    o = fn(tq, k, v)
    assert o.grad_fn is not None
    o.backward(w)
    assert torch.equal(tq.grad, dq_all)
    assert k.grad is None and v.grad is None


@pytest.mark.parametrize("name", ["int8", "fp8", "fp16"])
def test_one_leaf_for_q_k_v(dev, oracle, name):
    """q, k and v one tensor: its gradient is dq + dk + dv, accumulated in the dtype in input order"""
    fn = _fn(name)
    x0 = torch.from_numpy(oracle.make_inputs(1, 2, 140, 64, seed=35)[0]).to(dev).half()
    w = torch.randn(x0.shape, generator=torch.Generator(device="cpu").manual_seed(9)).half().to(dev)
    _, (dq, dk, dv) = _grads(fn, x0, x0, x0, w, is_causal=True)
    x = x0.clone().requires_grad_()
    fn(x, x, x, is_causal=True).backward(w)
    assert torch.equal(x.grad, (dq + dk) + dv)
