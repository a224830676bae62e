"""GPU tests of the packed-batch backward (`lbfa_forward_varlen_lse` + `lbfa_backward_varlen` behind torch autograd,
lowbit_quant_fa2_paddle_amd/autograd.py `_VarlenAttentionFn`).

Against `bwd_varlen_reference` (the float64 restatement, fed the operator's own O and LSE) under the bounds of
test_gpu_backward._assert_close and, element by element, of test_gpu_backward._grad_close (bwd_varlen_reference's per-element
bound, sequence by sequence); bit for bit against the dense operator on single sequences; zero gradients outside every
sequence; cosine against the true gradient of un-quantised attention.  Whole file 4 s on an MI355X; peak device memory 6.0 GiB
(torch.cuda.max_memory_allocated: the 64K-token full-size case, q, k, v, o, their gradients and the workspaces at H = 32,
D = 128)."""
import numpy as np
import pytest

from bwd_varlen_reference import varlen_backward, varlen_lse
from test_gpu_backward import _assert_close, _grad_close
from test_gpu_parity import TDT, _np, _t, dev  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _covered(cu, total, cap):
    m = np.zeros(total, bool)
    for b in range(len(cu) - 1):
        m[cu[b]:cu[b] + min(cu[b + 1] - cu[b], cap)] = True
    return m


def _run(oracle, dev, lens_q, lens_k, Hq, Hkv, D, *, dtype="fp16", causal=False, smooth_k=True, seed=0, max_q=None, max_k=None,
         q_qmax=127, k_qmax=127, use_dlse=False, cu_dtype=torch.int32, pad_q=0, pad_k=0):
    """packed inputs (pad_q / pad_k tokens after the last sequence), forward with grad through the private helper, one backward
    with a random dO (and a loss on the LSE rows the forward wrote); numpy copies of everything the reference needs"""
    from lowbit_quant_fa2_paddle_amd import core
    pad = [pad_q] if pad_q or pad_k else []
    q, k, v, cu_q, cu_k = oracle.make_varlen_inputs(list(lens_q) + pad, list(lens_k) + ([pad_k] if pad else []), Hq, Hkv, D,
                                                    seed=seed, dtype=dtype, k_bias=0.5)
    if pad:  # the padding tokens lie in no sequence
        cu_q, cu_k = cu_q[:-1], cu_k[:-1]
    max_q = max(lens_q) if max_q is None else max_q
    max_k = max(lens_k) if max_k is None else max_k
    tq, tk, tv = (_t(a, dtype, dev).requires_grad_() for a in (q, k, v))
    tcq, tck = (torch.from_numpy(c).to(cu_dtype).to(dev) for c in (cu_q, cu_k))
    o, lse = core._varlen_attention(tq, tk, tv, tcq, tck, max_q, max_k, is_causal=causal, sm_scale=None, smooth_k=smooth_k,
                                    q_qmax=q_qmax, k_qmax=k_qmax, return_lse=True)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    w = torch.randn(o.shape, generator=g).to(dev)
    loss = (o.float() * w).sum()
    cov = _covered(cu_q, q.shape[0], max_q) & _covered_keys_nonempty(cu_q, cu_k, q.shape[0])
    dl = None
    if use_dlse:
        wl = torch.randn(lse.shape, generator=g)
        wl[:, ~cov] = 0
        idx = torch.from_numpy(cov).to(dev)
        loss = loss + (lse[:, idx] * wl[:, cov].to(dev)).sum()
        dl = wl.numpy().astype(np.float64)
    loss.backward()
    return dict(q=q, k=k, v=v, cu_q=cu_q, cu_k=cu_k, o=_np(o), lse=_np(lse).astype(np.float64), lse_t=lse.detach(), o_t=o.detach(),
                do=oracle.to_storage(w.cpu().numpy(), dtype), dlse=dl, dq=_np(tq.grad), dk=_np(tk.grad), dv=_np(tv.grad),
                grads=(tq.grad, tk.grad, tv.grad), tensors=(tq, tk, tv, tcq, tck), max_q=max_q, max_k=max_k, cov=cov)


def _covered_keys_nonempty(cu_q, cu_k, total):
    """query rows of sequences with at least one key (rows of key-less sequences hold -inf LSE)"""
    m = np.zeros(total, bool)
    for b in range(len(cu_q) - 1):
        if cu_k[b + 1] > cu_k[b]:
            m[cu_q[b]:cu_q[b + 1]] = True
    return m


def _reference(r, dtype, causal, smooth_k, q_qmax=127, k_qmax=127, only=None):
    """(dq, dk, dv, bq, bk, bv): the reference gradients and their per-element bounds"""
    return varlen_backward(r["q"], r["k"], r["v"], r["o"], r["lse"], r["do"], r["cu_q"], r["cu_k"], dtype=dtype, is_causal=causal,
                           smooth_k=smooth_k, q_qmax=q_qmax, k_qmax=k_qmax, dlse=r["dlse"], only=only, return_bound=True)


def test_varlen_operator_produces_gradients(dev, oracle):
    """Fails without the feature: the packed result then has no grad_fn and backward() raises."""
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v, cu_q, cu_k = oracle.make_varlen_inputs([100, 37], [100, 37], 2, 2, 64, seed=1)
    tq, tk, tv = (_t(a, "fp16", dev).requires_grad_() for a in (q, k, v))
    cu = torch.from_numpy(cu_q).to(dev)
    o = lb.sageattn_varlen(tq, tk, tv, cu, cu, 100, 100, is_causal=True)
    assert o.grad_fn is not None
    o.float().sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() for t in (tq, tk, tv))
    o2 = lb.lowbit_fa_varlen(tq, tk, tv, cu.long(), cu.long(), 100, 100, is_causal=True)  # int64 cu_seqlens
    assert o2.grad_fn is not None and torch.equal(o2, o)


# ---------------------------------------------------------------------------------------------------------------------------
# LSE for packed batches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal,smooth_k", [("fp16", 64, False, True), ("bf16", 128, True, True), ("fp16", 80, False, False)])
def test_varlen_lse_vs_reference(dev, oracle, dtype, D, causal, smooth_k):
    from lowbit_quant_fa2_paddle_amd import core
    lens_q = [1, 65, 0, 129, 40]
    lens_k = [7, 65, 12, 129, 0] if not causal else [1, 65, 0, 129, 0]
    q, k, v, cu_q, cu_k = oracle.make_varlen_inputs(lens_q, lens_k, 6, 2, D, seed=4, dtype=dtype, k_bias=0.5)
    tq, tk, tv = (_t(a, dtype, dev) for a in (q, k, v))
    tcq, tck = (torch.from_numpy(c).to(dev) for c in (cu_q, cu_k))
    kw = dict(is_causal=causal, sm_scale=None, smooth_k=smooth_k, q_qmax=127, k_qmax=127)
    o, lse = core._varlen_attention(tq, tk, tv, tcq, tck, max(lens_q), max(lens_k), return_lse=True, **kw)
    o0 = core._varlen_attention(tq, tk, tv, tcq, tck, max(lens_q), max(lens_k), return_lse=False, **kw)
    assert torch.equal(o, o0)  # the LSE changes nothing in o
    ref, corr = varlen_lse(q, k, v, cu_q, cu_k, return_corr=True, dtype=dtype, is_causal=causal, smooth_k=smooth_k)
    got = _np(lse).astype(np.float64)
    fin = np.isfinite(ref)
    assert np.all(got[~fin & ~np.isnan(ref)] == -np.inf)  # sequences without keys
    assert np.any(~fin & ~np.isnan(ref))
    # 2^-21 relative plus the absolute term of the dense parity bound (test_gpu_parity: the kernel sums the fp16-rounded P of
    # its PV product into l), and one storage-dtype ulp of the rounded q . km, which the kernel forms in its own order
    ulp = (2.0 ** -10 if dtype == "fp16" else 2.0 ** -7) * np.abs(corr[fin])
    d = np.abs(got[fin] - ref[fin])
    assert np.all(d <= 2.0 ** -21 * np.abs(ref[fin]) + 1e-3 + ulp), f"LSE max err {d.max():.3e}"
    print(f"LSE max abs err {d.max():.3e}")


def test_varlen_lse_one_sequence_equals_dense(dev, oracle):
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import core
    q, k, v = oracle.make_inputs(1, 4, 300, 64, seed=9, layout="NHD", k_bias=0.3)
    tq, tk, tv = (_t(a, "fp16", dev) for a in (q, k, v))
    cu = torch.tensor([0, 300], dtype=torch.int32, device=dev)
    for causal in (False, True):
        o_d, lse_d = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, tensor_layout="NHD", is_causal=causal, return_lse=True)
        o_v, lse_v = core._varlen_attention(tq[0], tk[0], tv[0], cu, cu, 300, 300, is_causal=causal, sm_scale=None, smooth_k=True,
                                            q_qmax=127, k_qmax=127, return_lse=True)
        assert torch.equal(o_d[0], o_v) and torch.equal(lse_d[0], lse_v)


# ---------------------------------------------------------------------------------------------------------------------------
# gradients against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
GRID = [
    # dtype, D, Hq, Hkv, causal, smooth_k, lens_q, lens_k, extra
    ("fp16", 64, 2, 2, False, True, [1, 63, 64, 65, 127], [1, 63, 64, 65, 127], {}),
    ("fp16", 64, 6, 2, True, True, [128, 129, 1, 513], [128, 129, 1, 513], {}),
    ("bf16", 128, 6, 2, False, True, [65, 0, 129, 40], [30, 77, 129, 0], {}),         # empty query / key ranges, len_q != len_k
    ("bf16", 64, 2, 2, True, False, [63, 200, 1], [63, 200, 1], {}),
    ("fp16", 128, 2, 2, True, False, [129, 64], [129, 64], {"max_q": 300, "max_k": 300}),  # max_seqlen above the true maximum
    ("fp16", 80, 6, 2, False, True, [70, 140, 1], [90, 60, 33], {}),                   # padded head dim
    ("bf16", 40, 2, 2, True, True, [65, 127], [65, 127], {}),
    ("fp16", 64, 6, 2, True, True, [130, 64, 1], [130, 64, 1], {"use_dlse": True}),    # loss on the LSE
    ("fp16", 64, 2, 2, False, True, [100, 257], [150, 90], {"q_qmax": 7, "k_qmax": 7, "use_dlse": True}),
    ("bf16", 128, 2, 2, False, True, [129, 65], [63, 200], {"q_qmax": 127, "k_qmax": 7}),
]


@pytest.mark.parametrize("dtype,D,Hq,Hkv,causal,smooth_k,lens_q,lens_k,extra", GRID)
def test_varlen_backward_vs_reference(dev, oracle, dtype, D, Hq, Hkv, causal, smooth_k, lens_q, lens_k, extra):
    qq, kq = extra.get("q_qmax", 127), extra.get("k_qmax", 127)
    r = _run(oracle, dev, lens_q, lens_k, Hq, Hkv, D, dtype=dtype, causal=causal, smooth_k=smooth_k, seed=D + Hq, q_qmax=qq,
             k_qmax=kq, use_dlse=extra.get("use_dlse", False), max_q=extra.get("max_q"), max_k=extra.get("max_k"))
    ref = _reference(r, dtype, causal, smooth_k, qq, kq)
    for name, got, want, bnd in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), ref[:3], ref[3:]):
        _assert_close(got, want, dtype, name)
        _grad_close(got, want, bnd, name)
    # empty ranges: no queries -> dk = dv = 0 for its keys; no keys -> dq = 0 for its queries
    cq, ck = r["cu_q"], r["cu_k"]
    for b in range(len(lens_q)):
        if lens_q[b] == 0:
            assert not r["dk"][ck[b]:ck[b + 1]].any() and not r["dv"][ck[b]:ck[b + 1]].any()
        if lens_k[b] == 0:
            assert not r["dq"][cq[b]:cq[b + 1]].any()


# ---------------------------------------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", [("fp16", 64, False), ("bf16", 128, True), ("fp16", 80, True)])
def test_one_packed_sequence_equals_dense_gradients(dev, oracle, dtype, D, causal):
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v = oracle.make_inputs(1, 6, 333, D, seed=5, layout="NHD", dtype=dtype, Hkv=2, k_bias=0.4)
    g = torch.Generator(device="cpu").manual_seed(3)
    w = torch.randn((1, 333, 6, D), generator=g).to(dev)
    grads = []
    for packed in (False, True):
        tq, tk, tv = (_t(a, dtype, dev).requires_grad_() for a in (q, k, v))
        if packed:
            cu = torch.tensor([0, 333], dtype=torch.int32, device=dev)
            o = lb.sageattn_varlen(tq[0], tk[0], tv[0], cu, cu, 333, 333, is_causal=causal)[None]
        else:
            o = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, tensor_layout="NHD", is_causal=causal)
        (o.float() * w).sum().backward()
        grads.append((o.detach(), tq.grad, tk.grad, tv.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_mixed_batch_equals_dense_per_sequence_without_smooth_k(dev, oracle):
    """Each sequence of a packed batch (no shared mean) is the dense backward of that sequence alone, bit for bit: nothing leaks
    between sequences."""
    import lowbit_quant_fa2_paddle_amd as lb
    lens = [1, 63, 64, 65, 200, 129, 7]
    for causal in (False, True):
        r = _run(oracle, dev, lens, lens, 6, 2, 64, causal=causal, smooth_k=False, seed=12)
        w = torch.from_numpy(r["do"]).to(dev)
        cu = r["cu_q"]
        for b in range(len(lens)):
            tq, tk, tv = (_t(a[cu[b]:cu[b + 1]][None], "fp16", dev).requires_grad_() for a in (r["q"], r["k"], r["v"]))
            o = lb.lowbit_fa_qk_int8_pv_fp16_triton(tq, tk, tv, tensor_layout="NHD", is_causal=causal, smooth_k=False)
            (o.float() * w[cu[b]:cu[b + 1]][None].float()).sum().backward()
            assert torch.equal(o[0].detach(), r["o_t"][cu[b]:cu[b + 1]]), b
            for got, t in zip(r["grads"], (tq, tk, tv)):
                assert torch.equal(got[cu[b]:cu[b + 1]], t.grad[0]), (causal, b)


def test_backward_deterministic_and_forward_unchanged(dev, oracle):
    import lowbit_quant_fa2_paddle_amd as lb
    runs = [_run(oracle, dev, [300, 1, 129], [300, 1, 129], 6, 2, 128, causal=True, seed=21) for _ in range(2)]
    for a, b in zip(runs[0]["grads"], runs[1]["grads"]):
        assert torch.equal(a, b)
    tq, tk, tv, tcq, tck = runs[0]["tensors"]
    with torch.no_grad():
        o = lb.sageattn_varlen(tq, tk, tv, tcq, tck, 300, 300, is_causal=True)
    assert torch.equal(o, runs[0]["o_t"])


# ---------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_tokens_outside_sequences_and_past_the_cut_get_zero_gradient(dev, oracle):
    """Tokens after the last sequence and tokens past max_seqlen (sequence 1 is cut at 100 of 150) get exactly zero gradient;
    the uncut sequences match the reference (the cut one has no reference: its K scales include the cut keys, as the
    forward's do)."""
    lens_q, lens_k = [80, 150, 33], [90, 150, 20]
    r = _run(oracle, dev, lens_q, lens_k, 2, 2, 64, seed=30, max_q=100, max_k=100, pad_q=24, pad_k=40)
    cq, ck = r["cu_q"], r["cu_k"]
    assert not r["dq"][cq[-1]:].any() and not r["dk"][ck[-1]:].any() and not r["dv"][ck[-1]:].any()
    assert not r["dq"][cq[1] + 100:cq[2]].any() and not r["dk"][ck[1] + 100:ck[2]].any() and not r["dv"][ck[1] + 100:ck[2]].any()
    assert r["dq"][cq[1]:cq[1] + 100].any() and r["dk"][ck[1]:ck[1] + 100].any()
    for x in ("dq", "dk", "dv"):
        assert np.all(np.isfinite(r[x]))
    ref = _reference(r, "fp16", False, True, only=(0, 2))
    for name, got, want, bnd, c in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), ref[:3], ref[3:], (cq, ck, ck)):
        for b in (0, 2):
            _assert_close(got[c[b]:c[b + 1]], want[c[b]:c[b + 1]], "fp16", f"{name} seq {b}")
            _grad_close(got[c[b]:c[b + 1]], want[c[b]:c[b + 1]], bnd[c[b]:c[b + 1]], f"{name}_seq{b}")


@pytest.mark.parametrize("causal", [False, True])
def test_cosine_against_true_gradient(dev, oracle, causal):
    lens = [200, 64, 333, 1]
    r = _run(oracle, dev, lens, lens if causal else [150, 90, 333, 5], 6, 2, 64, causal=causal, seed=40)
    tq, tk, tv = (torch.from_numpy(a).to(dev).double().requires_grad_() for a in (r["q"], r["k"], r["v"]))
    w = torch.from_numpy(r["do"]).to(dev).double()
    cq, ck = r["cu_q"], r["cu_k"]
    loss = 0
    for b in range(len(lens)):
        qb, kb, vb = tq[cq[b]:cq[b + 1]].transpose(0, 1), tk[ck[b]:ck[b + 1]].transpose(0, 1), tv[ck[b]:ck[b + 1]].transpose(0, 1)
        kb, vb = kb.repeat_interleave(3, 0), vb.repeat_interleave(3, 0)
        ob = torch.nn.functional.scaled_dot_product_attention(qb, kb, vb, is_causal=causal)
        loss = loss + (ob.transpose(0, 1) * w[cq[b]:cq[b + 1]]).sum()
    loss.backward()
    for name, got, t in zip(("dq", "dk", "dv"), (r["dq"], r["dk"], r["dv"]), (tq, tk, tv)):
        a, b = got.ravel().astype(np.float64), t.grad.cpu().numpy().ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos >= 0.995, f"{name}: cosine {cos:.6f}"


# ---------------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_size_mixed_batch_causal_d128(dev):
    """About 64K packed tokens (seeded lengths 256..8192), H = 32, D = 128, causal, no shared mean: sampled sequences equal the
    per-sequence dense backward bit for bit."""
    import lowbit_quant_fa2_paddle_amd as lb
    rng = np.random.default_rng(7)
    lens = []
    while sum(lens) < 60000:
        lens.append(int(rng.integers(256, 8193)))
    H, D = 32, 128
    tot = sum(lens)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v = (torch.randn((tot, H, D), generator=g, device=dev, dtype=torch.float16).requires_grad_() for _ in range(3))
    w = torch.randn((tot, H, D), generator=g, device=dev, dtype=torch.float16)
    o = lb.sageattn_varlen(q, k, v, cu, cu, max(lens), max(lens), is_causal=True, smooth_k=False)
    (o.float() * w.float()).sum().backward()
    c = cu.tolist()
    for b in sorted({0, len(lens) - 1, int(np.argmax(lens)), int(np.argmin(lens))}):
        sq, sk, sv = (t.detach()[c[b]:c[b + 1]][None].clone().requires_grad_() for t in (q, k, v))
        ob = lb.lowbit_fa_qk_int8_pv_fp16_triton(sq, sk, sv, tensor_layout="NHD", is_causal=True, smooth_k=False)
        (ob.float() * w[c[b]:c[b + 1]][None].float()).sum().backward()
        assert torch.equal(ob[0].detach(), o.detach()[c[b]:c[b + 1]]), b
        for t, s in zip((q, k, v), (sq, sk, sv)):
            assert torch.equal(t.grad[c[b]:c[b + 1]], s.grad[0]), b
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all()
