"""GPU tests of the attention backward (`lbfa_backward` behind torch autograd, lowbit_quant_fa2_paddle_amd/autograd.py).

Against `bwd_reference` (the float64 restatement of the contract, fed the operator's own O and LSE): per gradient tensor
||d||_2 / ||ref||_2 <= 4e-3 (fp16) / 1.6e-2 (bf16) and max|d| <= 1e-2 (fp16) / 4e-2 (bf16) x max|ref| - the kernel rounds P and
dS to the input dtype once each before an fp32-accumulated MFMA.  Both bounds carry a 1e-5 absolute floor: with a single key
dq = dk = 0 exactly, and the kernel's dP - delta (two fp32 sums in different orders) leaves a residue at fp32 level.
Every such check also runs `_grad_close`: each element within the per-element bound of bwd_reference.grad_bound (the largest
deviation a correct kernel can show, derived from attn_bwd.hip's arithmetic and checked sound and sharp on the CPU by
test_bwd_bound_cpu.py); the worst ratio is printed as `BWDBOUND <test> <tensor> worst=<ratio>`.
Against the true gradient of un-quantised attention: cosine similarity (the quantised operators are straight-through, so
only a similarity bound applies)."""
import math
import os

import numpy as np
import pytest

from bwd_reference import attention_backward
from test_gpu_parity import TDT, _canon, _np, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# name -> (operator, extra kwargs, q_qmax, k_qmax)
OPS = {
    "int8_triton": ("lowbit_fa_qk_int8_pv_fp16_triton", {}, 127, 127),
    "int8_cuda": ("lowbit_fa_qk_int8_pv_fp16_cuda", {}, 127, 127),
    "int4": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 4}, 7, 7),
    "int4_q8": ("lowbit_fa_qk_int4_pv_fp16_triton", {"q_bits": 8}, 127, 7),
    "fp8": ("lowbit_fa_qk_int8_pv_fp8_cuda", {}, 127, 127),
    "fp16": ("flash_attn_fp16", {}, 0, 0),
}


def _op(name):
    import lowbit_quant_fa2_paddle_amd as lb
    fn_name, extra, qq, kq = OPS[name]
    fn = getattr(lb, fn_name, None) or getattr(lb.core, fn_name)
    return (lambda *a, **kw: fn(*a, **extra, **kw)), qq, kq


def _run(name, dtype, layout, causal, B, H, Hkv, S, Sk, D, *, smooth_k=True, sm_scale=None, use_dlse=False, seed=0, dev=None,
         oracle=None):
    """inputs, forward with grad, one backward with a random upstream dO (and dLSE); returns numpy copies (canonical)"""
    fn, qq, kq = _op(name)
    q, k, v = oracle.make_inputs(B, H, S, D, seed=seed, layout=layout, dtype=dtype, Hkv=Hkv, Sk=Sk, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev).requires_grad_() for a in (q, k, v))
    kw = dict(tensor_layout=layout, is_causal=causal, sm_scale=sm_scale, return_lse=True)
    if qq:
        kw["smooth_k"] = smooth_k
    o, lse = fn(tq, tk, tv, **kw)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    w = torch.randn(o.shape, generator=g).to(dev)
    loss = (o.float() * w).sum()
    wl = None
    if use_dlse:
        wl = torch.randn(lse.shape, generator=g).to(dev)
        loss = loss + (lse * wl).sum()
    loss.backward()
    do = oracle.to_storage(w.cpu().numpy(), dtype)  # the gradient reaching o is rounded to o's dtype
    res = dict(q=_canon(q, layout), k=_canon(k, layout), v=_canon(v, layout), o=_canon(_np(o), layout), lse=_np(lse),
               do=_canon(do, layout), dlse=None if wl is None else wl.cpu().numpy(),
               dq=tq.grad, dk=tk.grad, dv=tv.grad, qq=qq, kq=kq,
               sm_scale=sm_scale if sm_scale is not None else 1.0 / math.sqrt(D))
    return res, (tq, tk, tv)


def _reference(r, causal, dtype, smooth_k, return_bound=False):
    return attention_backward(r["q"], r["k"], r["v"], r["o"], r["lse"], r["do"], sm_scale=r["sm_scale"], is_causal=causal,
                              dtype=dtype, q_qmax=r["qq"], k_qmax=r["kq"], smooth_k=smooth_k and r["qq"] != 0, dlse=r["dlse"],
                              return_bound=return_bound)


def _assert_close(got, ref, dtype, what):
    rel_l2, rel_max = (4e-3, 1e-2) if dtype == "fp16" else (1.6e-2, 4e-2)
    d = got.astype(np.float64) - ref
    n = np.linalg.norm(ref)
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    assert np.linalg.norm(d) <= rel_l2 * n + 1e-5 * math.sqrt(d.size), f"{what}: rel L2 {np.linalg.norm(d) / max(n, 1e-300):.3e}"
    assert np.abs(d).max() <= rel_max * np.abs(ref).max() + 1e-5, f"{what}: max {np.abs(d).max():.3e} vs {np.abs(ref).max():.3e}"


def _grad_close(got, ref, bound, what):
    """every element finite and |got - ref| <= bound (bwd_reference.grad_bound); prints the worst ratio"""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    d = np.abs(got - ref)
    worst = float(np.max(np.where(d > 0, d / np.maximum(bound, 1e-300), 0.0))) if d.size else 0.0
    if os.environ.get("PYTEST_CURRENT_TEST"):
        print(f"BWDBOUND {os.environ['PYTEST_CURRENT_TEST'].split(' ')[0]} {what} worst={worst:.3f}")
    if worst > 1.0:
        i = np.unravel_index(np.argmax(np.where(d > 0, d / np.maximum(bound, 1e-300), 0.0)), d.shape)
        raise AssertionError(f"{what}: |d| / bound = {worst:.3f} at {i} (got {got[i]:.6e}, ref {ref[i]:.6e}, bound {bound[i]:.3e})")


def test_int8_operator_produces_gradients(dev, oracle):
    """Fails without the feature: the forward result then has no grad_fn and backward() raises."""
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = oracle.make_inputs(1, 2, 128, 64, seed=3)
    tq, tk, tv = (_t(a, "fp16", dev).requires_grad_() for a in (q, k, v))
    o = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv)
    w = torch.randn(o.shape, device=dev)
    (o.float() * w).sum().backward()
    for t in (tq, tk, tv):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype
        assert torch.isfinite(t.grad).all()


CASES = [
    # name, dtype, layout, causal, B, H, Hkv, S, Sk, D, smooth_k, sm_scale, dlse
    ("int8_triton", "fp16", "HND", False, 1, 2, 2, 200, 200, 64, True, None, False),
    ("int8_triton", "bf16", "NHD", True, 1, 8, 2, 333, 333, 128, True, None, True),
    ("int8_triton", "fp16", "NHD", False, 1, 2, 2, 512, 77, 128, True, 0.05, True),
    ("int8_triton", "fp16", "HND", True, 1, 1, 1, 1, 1, 64, True, None, False),
    ("int8_cuda", "fp16", "HND", False, 1, 2, 1, 77, 512, 40, False, None, False),
    ("int4", "fp16", "HND", True, 1, 2, 2, 256, 256, 64, True, None, True),
    ("int4_q8", "bf16", "HND", False, 1, 2, 2, 128, 200, 80, True, None, False),
    ("fp8", "fp16", "NHD", False, 1, 8, 2, 200, 333, 64, True, None, True),
    ("fp8", "bf16", "HND", True, 1, 2, 2, 512, 512, 128, False, None, False),
    ("fp16", "fp16", "HND", True, 1, 8, 2, 333, 333, 64, False, None, True),
    ("fp16", "bf16", "NHD", False, 2, 2, 2, 1, 77, 128, False, None, False),
    ("fp16", "fp16", "HND", False, 1, 2, 1, 200, 512, 80, False, 0.3, False),
]


@pytest.mark.parametrize("name,dtype,layout,causal,B,H,Hkv,S,Sk,D,smooth_k,sm_scale,use_dlse", CASES)
def test_backward_vs_reference(dev, oracle, name, dtype, layout, causal, B, H, Hkv, S, Sk, D, smooth_k, sm_scale, use_dlse):
    r, (tq, tk, tv) = _run(name, dtype, layout, causal, B, H, Hkv, S, Sk, D, smooth_k=smooth_k, sm_scale=sm_scale,
                           use_dlse=use_dlse, dev=dev, oracle=oracle)
    for t in (tq, tk, tv):
        assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
    ref = _reference(r, causal, dtype, smooth_k, return_bound=True)
    for what, got, rf, bnd in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), ref[:3], ref[3:]):
        _assert_close(_canon(_np(got), layout), rf, dtype, what)
        _grad_close(_canon(_np(got), layout), rf, bnd, what)


@pytest.mark.parametrize("name", ["int8_triton", "fp8"])
def test_backward_takes_out_the_forwards_own_correction(dev, oracle, name):
    """The backward must take out of the LSE the very smooth-K correction dtype(q . km) the forward put in: any other fp32
    order can round it one ulp away, and that ulp (times sm_scale log2e) scales a whole row of P.  Observed without a
    reference: with every key's channel 0 equal to c0, a loss on the LSE alone (dO = 0, dLSE = 1) gives dS = P and
    dq[i, 0] = sm_scale c0 sum_t P_it = sm_scale c0 (P normalised by the forward's own LSE).  Peaky q and keys around 16
    make |q . km| ~ 10^3, where one fp16 ulp of it moves P by up to 6 %; about 1 row in 5000 of these inputs rounds apart
    in the two orders the forward and the earlier backward used."""
    fn, _, _ = _op(name)
    D, c0 = 64, 16.0
    q, k, v = oracle.make_inputs(1, 8, 4096, D, seed=1, k_bias=c0)
    q = oracle.to_storage(q * np.float32(6.0), "fp16")
    k[..., 0] = c0
    tq, tk, tv = (_t(a, "fp16", dev).requires_grad_() for a in (q, k, v))
    o, lse = fn(tq, tk, tv, return_lse=True)
    lse.backward(torch.ones_like(lse))
    rowsum = tq.grad[..., 0].double().cpu().numpy() / (D ** -0.5 * c0)
    err = np.abs(rowsum - 1.0)
    print(f"{name}: max |sum_t P - 1| = {err.max():.2e}, rows over 2.5e-3: {int((err > 2.5e-3).sum())}")
    # P rounded to fp16 into the sum (random, 2^-11 each), the fp16 store of dq (2^-11), the forward's fp32 row sum
    assert err.max() <= 2.5e-3


def _sdpa_grads(q, k, v, do, causal, sm_scale):
    """float64 autograd of softmax attention on the un-quantised inputs (CPU)"""
    Hq, Hkv = q.shape[1], k.shape[1]
    tq, tk, tv = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (q, k, v))
    kk, vv = tk.repeat_interleave(Hq // Hkv, 1), tv.repeat_interleave(Hq // Hkv, 1)
    s = tq @ kk.transpose(-1, -2) * sm_scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(), float("-inf"))
    o = torch.softmax(s, -1) @ vv
    return torch.autograd.grad(o, (tq, tk, tv), torch.from_numpy(do.astype(np.float64)))


@pytest.mark.parametrize("name,bound", [("fp16", 0.999), ("int8_triton", 0.995), ("fp8", 0.99), ("int4", None)])
@pytest.mark.parametrize("causal", [False, True])
def test_backward_vs_true_gradient(dev, oracle, name, bound, causal):
    r, _ = _run(name, "fp16", "HND", causal, 1, 4, 2, 256, 256, 64, dev=dev, oracle=oracle, seed=11)
    true = _sdpa_grads(r["q"], r["k"], r["v"], r["do"], causal, r["sm_scale"])
    for what, got, t in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), true):
        a, b = _np(got).astype(np.float64).ravel(), t.numpy().ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        print(f"{name} causal={causal} {what}: cosine {cos:.6f}")
        if bound is not None:
            assert cos >= bound, f"{name} {what}: cosine {cos:.6f} < {bound}"


@pytest.mark.parametrize("name", ["int8_triton", "fp8", "fp16"])
def test_forward_unchanged_under_grad(dev, oracle, name):
    fn, qq, _ = _op(name)
    q, k, v = oracle.make_inputs(1, 4, 300, 64, seed=7, Hkv=2)
    t = [_t(a, "bf16", dev) for a in (q, k, v)]
    with torch.no_grad():
        o0, l0 = fn(*t, is_causal=True, return_lse=True)
        o1 = fn(*t, is_causal=True)
    tg = [x.clone().requires_grad_() for x in t]
    o, lse = fn(*tg, is_causal=True, return_lse=True)
    assert o.grad_fn is not None
    assert torch.equal(o.detach(), o0) and torch.equal(lse.detach(), l0) and torch.equal(o1, o0)


@pytest.mark.parametrize("name", ["int8_triton", "fp16"])
def test_backward_deterministic(dev, oracle, name):
    fn, _, _ = _op(name)
    q, k, v = oracle.make_inputs(2, 8, 600, 128, seed=9, Hkv=2)
    t = [_t(a, "fp16", dev).requires_grad_() for a in (q, k, v)]
    w = torch.randn((2, 8, 600, 128), device=dev)
    grads = []
    for _ in range(2):
        o = fn(*t, is_causal=False)
        grads.append(torch.autograd.grad((o.float() * w).sum(), t))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_full_size_c2_int8(dev, oracle):
    """C2 (B4 H32 S4096 D64, HND, non-causal, int8): one (b, h) checked against bwd_reference."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, S, D = 4, 32, 4096, 64
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, S, D, device=dev).half().requires_grad_() for _ in range(3))
    o, lse = lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, return_lse=True)
    w = torch.randn(o.shape, device=dev)
    (o.float() * w).sum().backward()
    b, h = 1, 17
    sl = lambda t: t.detach()[b:b + 1, h:h + 1].float().cpu().numpy()
    do = w[b:b + 1, h:h + 1].half().float().cpu().numpy()
    ref = attention_backward(sl(q), sl(k), sl(v), sl(o), lse.detach()[b:b + 1, h:h + 1].cpu().numpy(), do, sm_scale=D ** -0.5,
                             dtype="fp16", q_qmax=127, k_qmax=127, smooth_k=True, return_bound=True)
    for what, got, rf, bnd in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), ref[:3], ref[3:]):
        assert torch.isfinite(got).all()
        _assert_close(got[b:b + 1, h:h + 1].float().cpu().numpy(), rf, "fp16", what)
        _grad_close(got[b:b + 1, h:h + 1].float().cpu().numpy(), rf, bnd, what)


def _torch_fwd_corr(q, km):
    """bwd_reference.fwd_corr in torch (fp32 elementwise adds in the kernels' order) for q [S, D], km [1, D] (D in {64, 128})"""
    prod = q.float() * km.float()
    part = []
    for g in range(4):
        acc = torch.zeros(q.shape[0], dtype=torch.float32, device=q.device)
        for s0 in range(0, q.shape[1], 64):
            for c in range(s0 + 16 * g, s0 + 16 * g + 16):
                acc = acc + prod[:, c]
        part.append(acc)
    return ((part[0] + part[1]) + (part[2] + part[3])).half().double()


def _torch_reference_head(q, k, v, o, lse, do, sm_scale, causal, return_bound=False):
    """bwd_reference restated in torch float64 on the GPU for one (b, h) of the int8 operator with smooth-K: [S, D] tensors
    (return_bound: and the bound of bwd_reference.grad_bound, restated by _torch_bound_head)"""
    S = q.shape[0]
    qd, kd = q.double(), k.double()
    km = kd.mean(0, keepdim=True).float().half()  # fp64 mean -> storage dtype
    ks_in = (k.float() - km.float()).half().float()  # k - km in the storage dtype

    def quant(x, scale, qmax, blk):
        x = x * scale
        n = (x.shape[0] + blk - 1) // blk
        xp = torch.zeros(n * blk, x.shape[1], dtype=torch.float32, device=x.device)
        xp[:x.shape[0]] = x
        xb = xp.view(n, -1)
        sc = torch.clamp(xb.abs().amax(1), min=1e-7) / qmax
        y = xb / sc[:, None]
        y = y + 0.5 * torch.where(y >= 0, 1.0, -1.0)
        return torch.trunc(y).view(n * blk, -1)[:x.shape[0]].double(), sc.double().repeat_interleave(blk)[:x.shape[0]]

    q8, qs = quant(q.float(), np.float32(sm_scale * 1.44269504).item(), 127.0, 128)
    k8, ks = quant(ks_in, 1.0, 127.0, 64)
    s2 = (q8 @ k8.T) * qs[:, None] * ks[None, :]
    corr = _torch_fwd_corr(q, km)
    lse2 = (lse.double() - corr * sm_scale) * 1.44269504
    p = torch.exp2(s2 - lse2[:, None])
    if causal:
        p = p.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=p.device).tril(), 0.0)
    dod = do.double()
    dv = p.T @ dod
    dp = dod @ v.double().T
    ds = p * (dp - (dod * o.double()).sum(1, keepdim=True))
    ref = (sm_scale * ds @ kd, sm_scale * ds.T @ qd, dv)
    if not return_bound:
        return ref
    del dp, ds
    from bwd_reference import LOG2E, U32
    c = (corr * sm_scale).abs()[:, None]
    e = U32 * (2 * s2.abs() + (s2 - lse2[:, None]).abs() + 3 * lse2.abs()[:, None] + 3 * LOG2E * c)
    if causal:
        e = e.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=p.device).tril(), 0.0)
    del s2
    return ref, _torch_bound_head(ref, p, e, q, k, v, o, do, sm_scale, "fp16")


def _torch_bound_head(ref, p, arg_err, q, k, v, o, do, sm_scale, dtype):
    """bwd_reference.grad_bound in torch float64 for one (b, h) (no GQA, no dLSE): [S, S] P and argument bound, [S, D] tensors"""
    from bwd_reference import EXP2_REL, HALF_SUB, SAFETY, TINY, U32, U_DT, _gamma
    u, half = U_DT[dtype], HALF_SUB[dtype]

    def rerr(x, e):  # bwd_reference._round_err
        hi = x + e
        return torch.minimum(hi, torch.clamp(u * hi, min=half))

    S, D = q.shape
    aq, ak, av, ao, ado = (t.double().abs() for t in (q, k, v, o, do))
    eP = p * (torch.exp2(arg_err) * (1 + EXP2_REL) - 1)
    eP = eP + torch.clamp(p + eP, max=TINY["bf16"])
    ePr = eP + rerr(p, eP)
    ev = ePr.T @ ado + _gamma(S) * ((p + ePr).T @ ado)
    del ePr
    t = (do.double() @ v.double().T - (do.double() * o.double()).sum(1, keepdim=True)).abs()
    et = (_gamma(D) * (ado @ av.T) + _gamma(D + 1) * (ado * ao).sum(1, keepdim=True)) * (1 + U32) + U32 * t
    ds = p * t
    eds = eP * (t + et) + p * et + U32 * (p + eP) * (t + et)
    del t, et, eP
    edsr = eds + rerr(ds, eds)
    del eds
    dsm = ds + edsr
    ek = sm_scale * (edsr.T @ aq + (_gamma(S) + 2 * U32) * (dsm.T @ aq))
    eq = sm_scale * (edsr @ ak + (_gamma(S) + 2 * U32) * (dsm @ ak))
    return [SAFETY * (e + rerr(x.abs(), e)) for x, e in zip(ref, (eq, ek, ev))]


def test_full_size_c3_causal(dev):
    """C3 shape (B4 H32 S16384 D128, NHD, causal, int8): all gradients finite; one (b, h) against a float64 restatement of
    bwd_reference on the GPU (a 16K x 16K CPU reference is too slow)."""
    import lowbit_quant_fa2_paddle_amd as lb
    B, H, S, D = 4, 32, 16384, 128
    torch.manual_seed(1)
    q, k, v = (torch.randn(B, S, H, D, device=dev).half().requires_grad_() for _ in range(3))
    o, lse = lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, tensor_layout="NHD", is_causal=True, return_lse=True)
    w = torch.randn(o.shape, device=dev)
    (o.float() * w).sum().backward()
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all()
    b, h = 2, 5
    hd = lambda t: t.detach()[b, :, h]
    with torch.no_grad():
        ref, bound = _torch_reference_head(hd(q), hd(k), hd(v), hd(o), lse[b, h], w[b, :, h].half(), D ** -0.5, True,
                                           return_bound=True)
    for what, got, rf, bnd in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), ref, bound):
        _assert_close(got[b, :, h].double().cpu().numpy(), rf.cpu().numpy(), "fp16", what)
        _grad_close(got[b, :, h].double().cpu().numpy(), rf.cpu().numpy(), bnd.cpu().numpy(), what)
