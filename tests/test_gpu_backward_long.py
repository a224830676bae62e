"""GPU tests of the attention backward past 64K keys, at the 2 GiB operand window and beyond it (run with `-m gpu` on an MI355X):
what test_gpu_long.py is for the forward operators.

  * the 16-bit conversion and the MFMA keep fp16 subnormals (a closed-form case: P = 2^-15 .. 2^-17 exactly), which is what lets
    bwd_reference.grad_bound charge half a subnormal step instead of the whole value below 2^-14;
  * long sequences of every operator against the block-sampled float64 reference (bwd_reference.attention_backward_sampled):
    64-row query blocks for dq, 64-key blocks for dk / dv - block 0, a block a third of the way, both halves of the 128-row
    quantiser block that holds row 65536, one block well past it, the last block (ragged at 65537) - of the last (batch, head);
  * the smooth-K mean on both sides of the forward's 64-partial switch (the backward always takes the separate finalize launch);
  * the far end of the forward's 2 GiB windows, an upstream gradient whose window is 4 GiB, q / o / dq windows past 2 GiB
    through the C ABI (the backward has no window), a tensor of more than 2^31 elements;
  * packed batches: one sequence past 64K tokens next to short ones, 4096 sequences, the kv-side window.

Every comparison is test_gpu_backward._assert_close (per sampled block) AND _grad_close (element by element against the sampled
bound; `BWDBOUND <test> <tensor> worst=<ratio>`), all gradients of the full tensors finite.  A bound larger than the values
proves nothing: `BWDSHARP <test> <tensor> <ratio>` is ||bound||_2 / ||ref||_2 over the sampled rows, and the rows marked
`sharp` (peaky queries, q x 6 for fp16 and q x 8 for bf16, whose u is 8 times larger) must keep it at or below 0.1.

Whole file 107 s on an MI355X (the CPU reference dominates); peak device memory 26.4 GiB (torch.cuda.max_memory_allocated:
the tensor of more than 2^31 elements with o, dO, dq and the workspace)."""
import os

import numpy as np
import pytest

from bwd_reference import HALF_SUB, _gamma, _round_err, attention_backward_sampled, p_panel, prepare_p
from bwd_varlen_reference import varlen_backward
from test_gpu_backward import OPS, _assert_close, _grad_close, _op
from test_gpu_long import BLKK, BLKQ, _free, _largest, _randn
from test_gpu_parity import TDT, dev  # noqa: F401
from test_gpu_varlen_backward import _run as _run_packed

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORKERS = 8  # threads of the sampled reference (the machines allow 16 CPUs)
SHARP_CAP = 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _blocks(S):
    """The sampling rule, 64-row blocks of a sequence of S rows: block 0, one a third of the way, both halves of the 128-row
    quantiser block that holds row 65536 (the q_scale index is q0 / 128), one well past it, the last (ragged at 65537)."""
    n = -(-S // 64)
    return sorted({b for b in (0, n // 3, 1024, 1025, 1024 + 517, n - 1) if b < n})


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def _peaky(t, mult):
    """q x mult, rounded to the dtype again (the distribution of the peaky_q6_* fixtures)"""
    return (t.float() * mult).to(t.dtype)


def _head(t, layout, b, hs):
    """[1, heads, S, D] float32 numpy of heads `hs` (a slice) of batch b of a device tensor"""
    x = t.detach()[b:b + 1, hs] if layout == "HND" else t.detach()[b:b + 1, :, hs].transpose(1, 2)
    return x.float().cpu().numpy()


def _compare(tag, what, got, ref, bnd, rows, dtype, sharp, normwise=True):
    """_assert_close per sampled block, _grad_close on every element, and the sharpness of the bound"""
    blk = rows // 64
    print(f"BWDREL {_test_id()} {tag}_{what} rel_l2={np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300):.2e}")
    for b in np.unique(blk) if normwise else ():
        _assert_close(got[:, :, blk == b], ref[:, :, blk == b], dtype, f"{tag} {what}[block {b}]")
    _grad_close(got, ref, bnd, f"{tag}_{what}")
    ratio = float(np.linalg.norm(bnd) / max(np.linalg.norm(ref), 1e-300))
    print(f"BWDSHARP {_test_id()} {tag}_{what} {ratio:.4f}")
    if sharp:
        assert ratio <= SHARP_CAP, f"{tag} {what}: ||bound|| / ||ref|| = {ratio:.3f} > {SHARP_CAP}: the check would hide that much"


def _check_head(tag, tq, tk, tv, o, lse, w, wl, grads, *, layout, causal, dtype, qq, kq, smooth, sm, b, hk, g, q_blocks, k_blocks,
                sharp=False, normwise=("dq", "dk", "dv")):
    """kv head (b, hk) and its g query heads against the sampled reference on the given blocks (the reference is fed the
    operator's o and lse of ALL rows of those heads).  grads = (dq, dk, dv) device tensors; `normwise`: the tensors that also
    get the norm-wise _assert_close."""
    hs, hks = slice(hk * g, (hk + 1) * g), slice(hk, hk + 1)
    r = attention_backward_sampled(
        _head(tq, layout, b, hs), _head(tk, layout, b, hks), _head(tv, layout, b, hks), _head(o, layout, b, hs),
        lse.detach()[b:b + 1, hs].cpu().numpy(), _head(w, layout, b, hs), sm_scale=sm, is_causal=causal, dtype=dtype, q_qmax=qq,
        k_qmax=kq, smooth_k=smooth and qq != 0, dlse=None if wl is None else wl[b:b + 1, hs].cpu().numpy(), q_blocks=q_blocks,
        k_blocks=k_blocks, return_bound=True, workers=WORKERS)
    for what, t, h, rows in (("dq", grads[0], hs, r["rows_q"]), ("dk", grads[1], hks, r["rows_k"]), ("dv", grads[2], hks, r["rows_k"])):
        if len(rows):
            _compare(tag, what, _head(t, layout, b, h)[:, :, rows].astype(np.float64), r[what], r["b" + what[1]], rows, dtype, sharp,
                     what in normwise)
    return r


def _inputs(shape_q, shape_k, dtype, seed, mult=1.0):
    q = _randn(shape_q, dtype, seed)
    if mult != 1.0:
        q = _peaky(q, mult)
    return q.requires_grad_(), _randn(shape_k, dtype, seed + 1, bias=0.5).requires_grad_(), _randn(shape_k, dtype, seed + 2).requires_grad_()


def _shape(layout, B, H, S, D):
    return (B, H, S, D) if layout == "HND" else (B, S, H, D)


def _forward_backward(name, q, k, v, *, layout, causal, use_dlse, seed, smooth_k=True):
    """forward with grad, one backward with an upstream gradient drawn in the dtype (and one into the LSE); -> o, lse, w, wl"""
    fn, qq, _ = _op(name)
    kw = dict(tensor_layout=layout, is_causal=causal, return_lse=True)
    if qq:
        kw["smooth_k"] = smooth_k
    o, lse = fn(q, k, v, **kw)
    w = _randn(tuple(o.shape), "fp16" if o.dtype == torch.float16 else "bf16", seed + 10)
    wl = None
    if use_dlse:
        wl = torch.randn(lse.shape, generator=torch.Generator(device="cuda").manual_seed(seed + 11), device="cuda")
        torch.autograd.backward([o, lse], [w, wl])
    else:
        o.backward(w)
    for t in (q, k, v):
        assert bool(torch.isfinite(t.grad).all()), "non-finite gradient"
    return o, lse, w, wl


# ---------------------------------------------------------------------------------------------------------------------------
# 1. fp16 subnormals in the 16-bit conversion and the MFMA
# ---------------------------------------------------------------------------------------------------------------------------
def _identical_keys_case(name, dtype, n, oracle, packed):
    """All keys of a head identical (quantised operators: smooth-K, so K - km = 0 exactly, every block sits on the 1e-7 floor and
    every code is 0): every score of a row is equal and P = 1 / Sk = 2^-n exactly.  -> (dv [Hkv, Sk or total, D] float64 numpy,
    its closed form [Hkv, sequences, D], the bound, the largest reference P error relative to half a step of the grid)"""
    Hq, Hkv, Sq, D, Sk = 4, 2, 256, 64, 2 ** n
    g = Hq // Hkv
    T = TDT[dtype]
    gen = torch.Generator(device="cuda").manual_seed(100 + n)
    nseq = 2 if packed else 1
    q = (torch.randn((nseq * Sq, Hq, D), generator=gen, device="cuda") / 16).to(T).requires_grad_()   # small: |s2|, |lse2| near n
    kvec = torch.randn((1, Hkv, D), generator=gen, device="cuda").to(T)
    k = kvec.expand(nseq * Sk, Hkv, D).contiguous().requires_grad_()
    v = torch.randn((nseq * Sk, Hkv, D), generator=gen, device="cuda").to(T).requires_grad_()
    w = torch.randn((nseq * Sq, Hq, D), generator=gen, device="cuda").to(T)
    sm = D ** -0.5
    if packed:
        from lowbit_quant_fa2_paddle_amd import core
        cq = torch.tensor([0, Sq, 2 * Sq], dtype=torch.int32, device="cuda")
        ck = torch.tensor([0, Sk, 2 * Sk], dtype=torch.int32, device="cuda")
        o, lse = core._varlen_attention(q, k, v, cq, ck, Sq, Sk, is_causal=False, sm_scale=None, smooth_k=True, q_qmax=127, k_qmax=127,
                                        return_lse=True)
        lse_b = lse.detach().reshape(Hq, nseq, Sq).transpose(0, 1)                # [seq, Hq, Sq]
    else:
        fn, qq, _ = _op(name)
        kw = dict(tensor_layout="NHD", return_lse=True)
        if qq:
            kw["smooth_k"] = True
        o, lse = fn(q[None], k[None], v[None], **kw)
        o, lse_b = o[0], lse.detach()
    o.backward(w)
    assert bool(torch.isfinite(v.grad).all())
    qq, kq = (127, 127) if packed else OPS[name][2:]
    # the reference's own P: within half a step of the 16-bit grid of 2^-n, its argument error included
    qs, ks, wn = (t.detach().float().cpu().numpy().reshape(nseq, -1, t.shape[1], D).transpose(0, 2, 1, 3) for t in (q, k, w))
    half = HALF_SUB[dtype] if 2.0 ** -n < 2.0 ** -14 and dtype == "fp16" else 2.0 ** -n * (2.0 ** -12 if dtype == "fp16" else 2.0 ** -9)
    worst = 0.0
    for s in range(nseq):
        c = prepare_p(qs[s:s + 1], ks[s:s + 1], lse_b[s:s + 1].cpu().numpy(), sm_scale=sm, dtype=dtype, q_qmax=qq, k_qmax=kq,
                      smooth_k=qq != 0)
        for hk in range(Hkv):
            p, e = p_panel(c, 0, hk, np.arange(Sq), np.arange(0, Sk, 257), return_arg_err=True)
            off = np.abs(p - 2.0 ** -n) + p * (np.exp2(e) * (1 + 2.0 ** -23) - 1)
            worst = max(worst, float(off.max() / half))
    # dv[j] = 2^-n sum_i dO[i] over the group's heads, for every key j of the sequence; what remains is the fp32 accumulation
    # (gamma_(g Sq) of sum |dO|, scaled by 2^-n) and the store rounding
    dsum = wn.astype(np.float64).reshape(nseq, Hkv, g * Sq, D).sum(axis=2) * 2.0 ** -n        # [seq, Hkv, D]
    e = _gamma(g * Sq) * np.abs(wn.astype(np.float64)).reshape(nseq, Hkv, g * Sq, D).sum(axis=2) * 2.0 ** -n
    bound = e + _round_err(np.abs(dsum), e, dtype)
    dv = v.grad.detach().double().cpu().numpy().reshape(nseq, Sk, Hkv, D).transpose(0, 2, 1, 3)   # [seq, Hkv, Sk, D]
    res = (q, k, v, o, lse, w) if not packed else None
    return dv, dsum, bound, worst, res


def _assert_closed_form(dv, dsum, bound, worst, n, dtype):
    assert worst < 1.0, f"the reference's P leaves 2^-{n} by {worst:.3f} of half a grid step: the case does not pin P"
    assert np.abs(dsum).max() > 0
    if not dv.any():
        raise AssertionError(f"dV is exactly zero: the hardware flushed the {dtype} P = 2^-{n} (a subnormal for fp16) to zero")
    d = np.abs(dv - dsum[:, :, None, :])
    ratio = float((d / bound[:, :, None, :]).max())
    print(f"BWDSUBNORMAL {_test_id()} P=2^-{n} worst |dv - 2^-n sum dO| / bound = {ratio:.3f}, reference P off by {worst:.2e} of half a step")
    assert ratio <= 1.0, f"dV differs from 2^-{n} sum_i dO by {ratio:.3f} of the bound (fp32 accumulation + store rounding)"


@pytest.mark.parametrize("n", [15, 16, 17])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["int8_triton", "fp8", "fp16"])
def test_mfma_keeps_fp16_subnormals(dev, oracle, name, dtype, n):
    """P = 2^-15, 2^-16, 2^-17: exactly representable fp16 subnormals (bf16: normal numbers, the control).  If the conversion
    or the MFMA's A operand flushed them, dV would be exactly zero; kept, dV = 2^-n sum_i dO up to fp32 accumulation and the
    store.  dq, dk and dv also meet the general bound, whose round-only model of subnormals (bwd_reference._round_err) rests on
    this test: dS = P (dP - delta) is a subnormal times an O(1) number.  (dq has no norm-wise check here: with identical keys
    dq_i = sm_scale k sum_j dS_ij, and that sum is zero in exact arithmetic - what the kernel returns is the rounding of dS, which
    only the element-wise bound describes.)"""
    dv, dsum, bound, worst, (q, k, v, o, lse, w) = _identical_keys_case(name, dtype, n, oracle, packed=False)
    _assert_closed_form(dv, dsum, bound, worst, n, dtype)
    qq, kq = OPS[name][2:]
    for hk in range(2):
        _check_head(f"h{hk}", q[None], k[None], v[None], o[None], lse, w[None], None, (q.grad[None], k.grad[None], v.grad[None]),
                    layout="NHD", causal=False, dtype=dtype, qq=qq, kq=kq, smooth=True, sm=64 ** -0.5, b=0, hk=hk, g=2, q_blocks=None,
                    k_blocks=_blocks(2 ** n)[-2:], normwise=("dk", "dv"))
    _free()


@pytest.mark.parametrize("n", [15, 17])
def test_mfma_keeps_fp16_subnormals_packed(dev, oracle, n):
    """the same in one packed batch of two sequences (ONE mean over all packed keys, all of them identical)"""
    dv, dsum, bound, worst, _ = _identical_keys_case("int8_triton", "fp16", n, oracle, packed=True)
    _assert_closed_form(dv, dsum, bound, worst, n, "fp16")
    _free()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. long sequences, every operator
# ---------------------------------------------------------------------------------------------------------------------------
LONG = [
    # op, Sq, Sk, D, H, Hkv, layout, causal, dtype, dlse, sharp
    ("int8_triton", 131072, 131072, 64, 2, 2, "HND", False, "fp16", True, True),
    ("int8_triton", 65537, 65537, 128, 4, 1, "NHD", True, "bf16", False, False),
    ("int8_triton", 131072, 131072, 128, 1, 1, "HND", True, "fp16", False, False),
    ("int8_triton", 131072, 256, 64, 2, 1, "HND", False, "bf16", False, False),   # every key sums 2 x 131072 rows: not sharp
    ("int4", 65537, 65537, 64, 1, 1, "HND", False, "fp16", False, True),
    ("int4", 131072, 131072, 128, 2, 1, "NHD", False, "bf16", False, False),
    ("int4_q8", 65537, 65537, 64, 1, 1, "NHD", True, "fp16", True, True),
    ("fp8", 131072, 131072, 64, 1, 1, "HND", False, "fp16", False, False),
    ("fp8", 65537, 65537, 128, 1, 1, "NHD", True, "bf16", False, True),
    ("fp16", 131072, 131072, 64, 2, 2, "HND", False, "fp16", False, True),
    ("fp16", 65537, 65537, 128, 2, 2, "NHD", True, "bf16", True, True),
    ("fp16", 256, 131072, 128, 2, 1, "NHD", False, "fp16", False, False),
]


@pytest.mark.parametrize("name,Sq,Sk,D,H,Hkv,layout,causal,dtype,use_dlse,sharp", LONG)
def test_long_sequence_vs_sampled_reference(dev, oracle, name, Sq, Sk, D, H, Hkv, layout, causal, dtype, use_dlse, sharp):
    """Smooth-K on for every quantised row, k_bias = 0.5 so that the mean matters.  `sharp` rows draw peaky queries and must
    keep ||bound|| / ||ref|| <= 0.1; the others are N(0,1), where a worst-case bound over 10^5 random-sign terms cannot be sharp
    and the norm-wise _assert_close carries the check.  The sharp rows have one query head per kv head: dk of a causal GQA group
    sums g x Sq rows, and with peaky queries (q x 6 fp16 / q x 8 bf16) its bound measured 0.13 (g = 2, bf16) to 0.27 (g = 4, fp16)
    of the tensor at 65537 - over the cap, so the GQA rows draw N(0,1) and rest on the norm-wise check."""
    mult = (6.0 if dtype == "fp16" else 8.0) if sharp else 1.0
    q, k, v = _inputs(_shape(layout, 1, H, Sq, D), _shape(layout, 1, Hkv, Sk, D), dtype, Sq % 1000 + D + H, mult)
    o, lse, w, wl = _forward_backward(name, q, k, v, layout=layout, causal=causal, use_dlse=use_dlse, seed=Sk % 1000 + D)
    qq, kq = OPS[name][2:]
    _check_head("last", q, k, v, o, lse, w, wl, (q.grad, k.grad, v.grad), layout=layout, causal=causal, dtype=dtype, qq=qq, kq=kq,
                smooth=True, sm=D ** -0.5, b=0, hk=Hkv - 1, g=H // Hkv, q_blocks=_blocks(Sq), k_blocks=_blocks(Sk), sharp=sharp)
    del q, k, v, o, lse, w, wl
    _free()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the smooth-K mean on both sides of the forward's 64-partial switch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk", [65536, 65537, 131072])   # forward: 64 partial sums (fused) / 65 / 128 (separate finalize launch)
@pytest.mark.parametrize("dtype,layout,name", [("fp16", "HND", "int8_triton"), ("bf16", "NHD", "fp8"), ("fp16", "NHD", "fp8"),
                                               ("bf16", "HND", "int8_triton")])
def test_backward_across_the_mean_switch(dev, oracle, Sk, dtype, layout, name):
    """The backward always forms km with the separate finalize launch, the forward fuses it into the K quantiser up to 65536
    keys: the shapes of test_gpu_long.test_smooth_k_mean_past_64_partials_is_exact.  A km that differed by one storage ulp
    between the two would change K - km, the codes and q . km, and so move whole rows of P: the check that fires is
    _grad_close on dq (all query rows are compared), then on dk / dv of the sampled key blocks."""
    B, H, Hkv, Sq, D = 1, 4, 2, 256, 128
    q, k, v = _inputs(_shape(layout, B, H, Sq, D), _shape(layout, B, Hkv, Sk, D), dtype, Sk + 7 * len(dtype + layout + name))
    o, lse, w, wl = _forward_backward(name, q, k, v, layout=layout, causal=False, use_dlse=False, seed=Sk % 977)
    qq, kq = OPS[name][2:]
    for hk in range(Hkv):
        _check_head(f"h{hk}", q, k, v, o, lse, w, wl, (q.grad, k.grad, v.grad), layout=layout, causal=False, dtype=dtype, qq=qq, kq=kq,
                    smooth=True, sm=D ** -0.5, b=0, hk=hk, g=H // Hkv, q_blocks=None, k_blocks=_blocks(Sk))
    del q, k, v, o, lse, w
    _free()


@pytest.mark.parametrize("Sk", [65536, 65537, 131072])
@pytest.mark.parametrize("name", ["int8_triton", "fp8"])
def test_forwards_own_correction_across_the_mean_switch(dev, oracle, name, Sk):
    """test_gpu_backward.test_backward_takes_out_the_forwards_own_correction at these key counts: channel 0 of every key equal
    to c0 and a loss on the LSE alone make dq[i, 0] / (sm_scale c0) the kernel's own row sum of P, which is 1 when the backward
    takes out the very correction (and so the very km) the forward put in.  Peaky inputs, the bound of that test."""
    fn, _, _ = _op(name)
    D, c0, H, Sq = 64, 16.0, 4, 256
    q = _peaky(_randn((1, H, Sq, D), "fp16", Sk % 1000 + 1), 6.0).requires_grad_()
    k = _randn((1, H, Sk, D), "fp16", Sk % 1000 + 2, bias=c0)
    k[..., 0] = c0
    k.requires_grad_()
    v = _randn((1, H, Sk, D), "fp16", Sk % 1000 + 3).requires_grad_()
    o, lse = fn(q, k, v, return_lse=True)
    lse.backward(torch.ones_like(lse))
    rowsum = q.grad[..., 0].double().cpu().numpy() / (D ** -0.5 * c0)
    err = np.abs(rowsum - 1.0)
    print(f"BWDROWSUM {_test_id()} max |sum_t P - 1| = {err.max():.2e}, rows over 2.5e-3: {int((err > 2.5e-3).sum())}")
    assert err.max() <= 2.5e-3
    del q, k, v, o, lse
    _free()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the far end of the forward's 2 GiB windows, and beyond them where the backward has none
# ---------------------------------------------------------------------------------------------------------------------------
H_WIN, D_WIN = 46, 128   # test_gpu_long: with 46 heads of 128 channels the largest accepted window ends within 2 D bytes of 2^31 - 1


def _window_shape(side):
    if side == "q":
        return _largest(lambda s: 2 * ((s + BLKQ) * H_WIN * D_WIN + D_WIN)), 256, 2
    return 200, _largest(lambda s: max(2 * ((s + 2 * BLKK) * H_WIN * D_WIN + D_WIN), (s + 2 * BLKK) * D_WIN + D_WIN)), H_WIN


@pytest.mark.parametrize("name", ["int8_triton", "fp16"])
@pytest.mark.parametrize("side", ["q", "kv"])
def test_backward_at_the_far_end_of_the_forward_window(dev, oracle, side, name):
    """The largest lengths the forward accepts (NHD, H = 46, D = 128): the last query block (q side) / the last key block (kv
    side) of the last head against the sampled reference."""
    Sq, Sk, Hkv = _window_shape(side)
    q, k, v = _inputs((1, Sq, H_WIN, D_WIN), (1, Sk, Hkv, D_WIN), "fp16", 40 + len(side + name))
    o, lse, w, _ = _forward_backward(name, q, k, v, layout="NHD", causal=False, use_dlse=False, seed=50)
    qq, kq = OPS[name][2:]
    far = dict(q_blocks=[(Sq - 1) // 64], k_blocks=[]) if side == "q" else dict(q_blocks=[], k_blocks=[(Sk - 1) // 64])
    if side == "q":  # dq of the last head alone: one query head against its kv head
        cut = lambda t: t[:, :, H_WIN - 1:]
        _check_head("far", cut(q), k[:, :, Hkv - 1:], v[:, :, Hkv - 1:], cut(o), lse[:, H_WIN - 1:], cut(w), None,
                    (cut(q.grad), k.grad[:, :, Hkv - 1:], v.grad[:, :, Hkv - 1:]), layout="NHD", causal=False, dtype="fp16", qq=qq, kq=kq,
                    smooth=True, sm=D_WIN ** -0.5, b=0, hk=0, g=1, **far)
    else:
        _check_head("far", q, k, v, o, lse, w, None, (q.grad, k.grad, v.grad), layout="NHD", causal=False, dtype="fp16", qq=qq, kq=kq,
                    smooth=True, sm=D_WIN ** -0.5, b=0, hk=Hkv - 1, g=1, **far)
    del q, k, v, o, lse, w
    _free()


def test_upstream_gradient_with_a_4_gib_window(dev, oracle, monkeypatch):
    """o.backward(w) with w = buf[:, :, :H] of a [1, Sq, 2 H, D] buffer: dO reaches lbfa_backward as that view (checked on the
    call's own arguments - _kernel_operand must not copy it), its (batch, head) window about 4 GiB while q, k, v, o sit at the
    end of the forward's.  The gradients equal those of the same call with a contiguous copy of dO bit for bit (the kernels are
    deterministic and see the same values), and the far block is within the bound."""
    from lowbit_quant_fa2_paddle_amd import _lib
    Sq, Sk, Hkv = _window_shape("q")
    q, k, v = _inputs((1, Sq, H_WIN, D_WIN), (1, Sk, Hkv, D_WIN), "fp16", 60)
    fn, qq, kq = _op("int8_triton")
    o, lse = fn(q, k, v, tensor_layout="NHD", return_lse=True)
    buf = _randn((1, Sq, 2 * H_WIN, D_WIN), "fp16", 61)
    w = buf[:, :, :H_WIN]
    assert 2 * ((Sq - 1) * w.stride(1) + D_WIN) > 4 * 10 ** 9 and w.stride(1) == 2 * H_WIN * D_WIN
    lib = _lib.load()
    real, seen = lib.lbfa_backward, []

    def spy(*a):
        seen.append((a[4], list(a[23])))  # dout, strides_dout {batch, head, seq}
        return real(*a)
    monkeypatch.setattr(lib, "lbfa_backward", spy, raising=True)
    g_view = torch.autograd.grad(o, (q, k, v), w, retain_graph=True)
    monkeypatch.undo()
    assert len(seen) == 1 and seen[0][0] == w.data_ptr() and seen[0][1][1:] == [D_WIN, 2 * H_WIN * D_WIN], seen
    wc = w.contiguous()
    g_copy = torch.autograd.grad(o, (q, k, v), wc)
    for a, b, what in zip(g_view, g_copy, ("dq", "dk", "dv")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{what} differs between the strided and the contiguous dO"
    cut = lambda t: t[:, :, H_WIN - 1:]
    _check_head("far", cut(q), k[:, :, Hkv - 1:], v[:, :, Hkv - 1:], cut(o), lse[:, H_WIN - 1:], cut(wc), None,
                (cut(g_view[0]), g_view[1][:, :, Hkv - 1:], g_view[2][:, :, Hkv - 1:]), layout="NHD", causal=False, dtype="fp16", qq=qq,
                kq=kq, smooth=True, sm=D_WIN ** -0.5, b=0, hk=0, g=1, q_blocks=[(Sq - 1) // 64], k_blocks=[])
    del q, k, v, o, lse, buf, w, wc, g_view, g_copy
    _free()


def _call_backward(lib, q, k, v, o, do, lse, dq, dk, dv, *, sm_scale, q_qmax, k_qmax, smooth_k):
    """lbfa_backward on NHD tensors [B, S, H, D] as they are (no copies), as autograd._run_backward calls it"""
    from lowbit_quant_fa2_paddle_amd import _lib
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    st = lambda t: _lib.strides3((t.stride(0), t.stride(2), t.stride(1)))  # {batch, head, seq}
    ws_bytes = lib.lbfa_backward_workspace_bytes(B, Hq, Hkv, Sq, Sk, D, q_qmax, 1 if smooth_k else 0)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q.device)
    ops = (q, k, v, o, do)
    _lib.check(lib.lbfa_backward(*(t.data_ptr() for t in ops), _lib.LBFA_F16, lse.data_ptr(), None, dq.data_ptr(), dk.data_ptr(),
                                 dv.data_ptr(), ws.data_ptr(), ws_bytes, B, Hq, Hkv, Sq, Sk, D, *(st(t) for t in ops), st(dq), st(dk),
                                 st(dv), float(sm_scale), q_qmax, k_qmax, 0, 1 if smooth_k else 0,
                                 torch.cuda.current_stream(q.device).cuda_stream))
    torch.cuda.synchronize()


def test_backward_has_no_operand_window(dev, oracle):
    """lbfa_backward itself (ctypes) on q, o, dq views whose token stride is doubled, so that their (batch, head) windows pass
    2 GiB (about 4 GiB), with the LSE of the forward on compact copies: accepted, and dq / dk / dv bitwise equal to the compact
    call.  include/lowbit_fa.h states it: the backward has no per-(batch, head) window."""
    from lowbit_quant_fa2_paddle_amd import _lib
    Sq, Sk, Hkv = _window_shape("q")
    H, D = H_WIN, D_WIN
    fn, qq, kq = _op("int8_triton")
    with torch.no_grad():
        q, k, v = (t.detach() for t in _inputs((1, Sq, H, D), (1, Sk, Hkv, D), "fp16", 70))
        o, lse = fn(q, k, v, tensor_layout="NHD", return_lse=True)
        do = _randn((1, Sq, H, D), "fp16", 71)
        wide = lambda t: torch.zeros((1, Sq, 2 * H, D), dtype=t.dtype, device=t.device)[:, :, :H].copy_(t)
        lib = _lib.load()
        kw = dict(sm_scale=D ** -0.5, q_qmax=qq, k_qmax=kq, smooth_k=True)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _call_backward(lib, q, k, v, o, do, lse, dq, dk, dv, **kw)
        qw, ow = wide(q), wide(o)
        dqw = torch.full((1, Sq, 2 * H, D), 7.0, dtype=q.dtype, device=q.device)
        assert 2 * ((Sq - 1) * qw.stride(1) + D) > 4 * 10 ** 9 and torch.equal(qw, q)
        dk2, dv2 = torch.empty_like(k), torch.empty_like(v)
        _call_backward(lib, qw, k, v, ow, do, lse, dqw[:, :, :H], dk2, dv2, **kw)
        assert bool(torch.isfinite(dq).all()) and bool(dq.any())
        assert torch.equal(dqw[:, :, :H], dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)
        assert bool((dqw[:, :, H:] == 7.0).all()), "the call wrote between the heads of the strided dq"
    del q, k, v, o, lse, do, qw, ow, dqw, dq, dk, dv, dk2, dv2
    _free()


def test_more_than_2_31_elements_hnd(dev, oracle):
    """The shape of test_gpu_long.test_more_than_2_31_elements_hnd with a gradient into o and into the LSE (lse2 / delta / dlse
    rows beyond 2^24): first and last query block of the last (batch, head) for dq, dk / dv of that head entirely."""
    B, H, Sq, Sk, D, dtype = 2, 64, 131136, 256, 128, "fp16"
    assert B * H * Sq * D >= 2 ** 31 + 2 ** 20 and B * H * Sq > 2 ** 24
    q, k, v = _inputs((B, H, Sq, D), (B, H, Sk, D), dtype, 80)
    o, lse, w, wl = _forward_backward("int8_triton", q, k, v, layout="HND", causal=False, use_dlse=True, seed=81)
    _check_head("last", q, k, v, o, lse, w, wl, (q.grad, k.grad, v.grad), layout="HND", causal=False, dtype=dtype, qq=127, kq=127,
                smooth=True, sm=D ** -0.5, b=B - 1, hk=H - 1, g=1, q_blocks=[0, (Sq - 1) // 64], k_blocks=None)
    del q, k, v, o, lse, w, wl
    _free()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. packed batches
# ---------------------------------------------------------------------------------------------------------------------------
def _compare_packed(r, ref, dtype, cu_q, cu_k, seqs):
    """r: test_gpu_varlen_backward._run; ref: varlen_backward(..., return_bound=True, blocks=...) -> per sequence _assert_close on
    its computed tokens, _grad_close and the sharpness over all computed tokens"""
    mq, mk = ref[6:]
    for name, got, want, bnd, m, cu in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), ref[:3], ref[3:6], (mq, mk, mk),
                                           (cu_q, cu_k, cu_k)):
        assert np.all(np.isfinite(got)), name
        for b in seqs:
            sl = slice(int(cu[b]), int(cu[b + 1]))
            if m[sl].any():
                _assert_close(got[sl][m[sl]], want[sl][m[sl]], dtype, f"{name} seq {b}")
        _grad_close(got[m], want[m], bnd[m], name)
        print(f"BWDSHARP {_test_id()} {name} {np.linalg.norm(bnd[m]) / max(np.linalg.norm(want[m]), 1e-300):.4f}")


@pytest.mark.parametrize("dtype,D,causal,qmax", [("fp16", 64, False, 127), ("bf16", 128, True, 127), ("fp16", 64, True, 7)])
def test_packed_long_sequence_next_to_short_ones(dev, oracle, dtype, D, causal, qmax):
    """One sequence of 65537 tokens next to short ones (300, 1 and an empty one), smooth-K: the single mean runs over more than
    65536 packed keys.  Sampled blocks of the long sequence and all of the short ones against bwd_varlen_reference."""
    lens_q = [65537, 300, 1, 0]
    lens_k = lens_q if causal else [65537, 200, 5, 7]
    r = _run_packed(oracle, dev, lens_q, lens_k, 2, 1, D, dtype=dtype, causal=causal, smooth_k=True, seed=D + qmax, q_qmax=qmax,
                    k_qmax=qmax, use_dlse=not causal)
    ref = varlen_backward(r["q"], r["k"], r["v"], r["o"], r["lse"], r["do"], r["cu_q"], r["cu_k"], dtype=dtype, is_causal=causal,
                          smooth_k=True, q_qmax=qmax, k_qmax=qmax, dlse=r["dlse"], return_bound=True,
                          blocks={0: (_blocks(65537), _blocks(65537))}, workers=WORKERS)
    _compare_packed(r, ref, dtype, r["cu_q"], r["cu_k"], range(4))
    ck = r["cu_k"]
    assert not r["dk"][ck[3]:ck[4]].any() and not r["dv"][ck[3]:ck[4]].any()  # keys of the sequence without queries
    _free()


@pytest.mark.parametrize("causal", [False, True])
def test_packed_long_sequence_equals_dense_without_smooth_k(dev, oracle, causal):
    """without the shared mean the long sequence's gradients are the dense operator's bit for bit
    (test_mixed_batch_equals_dense_per_sequence_without_smooth_k at 65537 tokens)"""
    import lowbit_quant_fa2_paddle_amd as lb
    lens = [65537, 300, 1]
    r = _run_packed(oracle, dev, lens, lens, 2, 1, 64, causal=causal, smooth_k=False, seed=91)
    w = torch.from_numpy(r["do"]).to(dev)
    tq, tk, tv = (torch.from_numpy(a[:lens[0]][None]).to(torch.float16).to(dev).requires_grad_() for a in (r["q"], r["k"], r["v"]))
    o = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, tensor_layout="NHD", is_causal=causal, smooth_k=False)
    (o.float() * w[:lens[0]][None].float()).sum().backward()
    assert torch.equal(o[0].detach(), r["o_t"][:lens[0]])
    for got, t in zip(r["grads"], (tq, tk, tv)):
        assert torch.equal(got[:lens[0]], t.grad[0])
    _free()


def test_packed_4096_sequences(dev, oracle):
    """4096 sequences of seeded lengths 0 .. 96 (some empty on either side), H 4 / 2, padding tokens after the last sequence and
    max_seqlen = 90 cutting the longest: every uncut sequence against the reference, zeros where the header promises zeros
    (the bisection of `covered` and grids of nkb Hkv B workgroups had only seen B <= 15)."""
    rng = np.random.default_rng(4096)
    lens_q = rng.integers(0, 97, 4096).tolist()
    lens_k = rng.integers(0, 97, 4096).tolist()
    cap = 90
    r = _run_packed(oracle, dev, lens_q, lens_k, 4, 2, 64, seed=92, max_q=cap, max_k=cap, pad_q=24, pad_k=40, use_dlse=False)
    cq, ck = r["cu_q"], r["cu_k"]
    uncut = [b for b in range(4096) if lens_q[b] <= cap and lens_k[b] <= cap]
    assert 0 < len(uncut) < 4096 and 0 in lens_q and 0 in lens_k
    for x in ("dq", "dk", "dv"):
        assert np.all(np.isfinite(r[x])), x
    assert not r["dq"][cq[-1]:].any() and not r["dk"][ck[-1]:].any() and not r["dv"][ck[-1]:].any()  # padding tokens
    for b in range(4096):
        if lens_q[b] > cap:
            assert not r["dq"][cq[b] + cap:cq[b + 1]].any(), b
        if lens_k[b] > cap:
            assert not r["dk"][ck[b] + cap:ck[b + 1]].any() and not r["dv"][ck[b] + cap:ck[b + 1]].any(), b
        if lens_q[b] == 0:
            assert not r["dk"][ck[b]:ck[b + 1]].any() and not r["dv"][ck[b]:ck[b + 1]].any(), b
        if lens_k[b] == 0:
            assert not r["dq"][cq[b]:cq[b + 1]].any(), b
    ref = varlen_backward(r["q"], r["k"], r["v"], r["o"], r["lse"], r["do"], cq, ck, dtype="fp16", smooth_k=True, only=set(uncut),
                          return_bound=True)
    mq, mk = np.zeros(r["q"].shape[0], bool), np.zeros(r["k"].shape[0], bool)
    for b in uncut:
        mq[cq[b]:cq[b + 1]] = True
        mk[ck[b]:ck[b + 1]] = True
    for name, got, want, bnd, m in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), ref[:3], ref[3:], (mq, mk, mk)):
        _assert_close(got[m], want[m], "fp16", name)
        _grad_close(got[m], want[m], bnd[m], name)
    _free()


def test_packed_backward_at_the_far_end_of_the_kv_window(dev, oracle):
    """the kv-side shape of test_gpu_long.test_varlen_window_limit through the backward: the last key block of the long sequence,
    last head (the reference is given that head alone: the mean, the codes and the gradients of a head do not see the others)"""
    from lowbit_quant_fa2_paddle_amd import core
    H, D, dtype = H_WIN, D_WIN, "fp16"
    n = _largest(lambda s: max((s + 2 * BLKK) * H * D + D, 2 * ((s + 2 * BLKK) * H * D + D)))
    lq, lk = [200, 77], [n, 77]
    q = _randn((sum(lq), H, D), dtype, 95).requires_grad_()
    k = _randn((sum(lk), H, D), dtype, 96, bias=0.5).requires_grad_()
    v = _randn((sum(lk), H, D), dtype, 97).requires_grad_()
    cu = lambda lens: torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    o, lse = core._varlen_attention(q, k, v, cu(lq), cu(lk), max(lq), max(lk), is_causal=False, sm_scale=None, smooth_k=True, q_qmax=127,
                                    k_qmax=127, return_lse=True)
    w = _randn(tuple(o.shape), dtype, 98)
    o.backward(w)
    for t in (q, k, v):
        assert bool(torch.isfinite(t.grad).all())
    h = H - 1
    f = lambda t: t.detach()[:, h:h + 1].float().cpu().numpy()
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    ref = varlen_backward(f(q), f(k), f(v), f(o), lse.detach()[h:h + 1].double().cpu().numpy(), f(w), cq, ck, dtype=dtype, smooth_k=True,
                          return_bound=True, blocks={0: ([], [(n - 1) // 64])}, only={0}, workers=WORKERS)
    mk = ref[7]
    mk[ck[1]:] = False
    assert mk.sum() == n - 64 * ((n - 1) // 64)
    for name, got, want, bnd in zip(("dk", "dv"), (f(k.grad), f(v.grad)), ref[1:3], ref[4:6]):
        _assert_close(got[mk], want[mk], dtype, name)
        _grad_close(got[mk], want[mk], bnd[mk], name)
    del q, k, v, o, lse, w
    _free()
