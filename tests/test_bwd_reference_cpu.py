"""CPU checks of `bwd_reference` (the float64 restatement of the backward contract) against torch autograd."""
import numpy as np
import pytest

from bwd_reference import attention_backward, attention_backward_sampled, grads_from_p, recompute_p

torch = pytest.importorskip("torch")


def _inputs(B, Hq, Hkv, Sq, Sk, D, seed):
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((B, h, s, D)) for h, s in ((Hq, Sq), (Hkv, Sk), (Hkv, Sk)))
    return q, k, v


def _autograd(q, k, v, do, dlse, causal, sm_scale):
    """o, lse and the float64 autograd gradients of softmax attention (GQA by repetition)"""
    g = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.from_numpy(a).requires_grad_() for a in (q, k, v))
    s = tq @ tk.repeat_interleave(g, 1).transpose(-1, -2) * sm_scale
    if causal:
        s = s.masked_fill(~torch.ones(s.shape[-2:], dtype=torch.bool).tril(), float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse[..., None]) @ tv.repeat_interleave(g, 1)
    loss = (o * torch.from_numpy(do)).sum()
    if dlse is not None:
        loss = loss + (lse * torch.from_numpy(dlse)).sum()
    grads = torch.autograd.grad(loss, (tq, tk, tv))
    return o.detach().numpy(), lse.detach().numpy(), [x.numpy() for x in grads]


@pytest.mark.parametrize("with_dlse", [False, True])
@pytest.mark.parametrize("causal,Hq,Hkv,Sq,Sk", [(False, 2, 2, 37, 50), (True, 4, 2, 45, 45), (False, 6, 2, 1, 9)])
def test_exact_inputs_match_autograd(with_dlse, causal, Hq, Hkv, Sq, Sk):
    q, k, v = _inputs(2, Hq, Hkv, Sq, Sk, 16, seed=Sq + Hq)
    rng = np.random.default_rng(1)
    do = rng.standard_normal(q.shape)
    dlse = rng.standard_normal(q.shape[:3]) if with_dlse else None
    sm = 0.3
    o, lse, want = _autograd(q, k, v, do, dlse, causal, sm)
    got = attention_backward(q, k, v, o, lse, do, sm_scale=sm, is_causal=causal, dlse=dlse)
    for a, b in zip(got, want):
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max())


def test_gqa_sum_and_causal_mask_match_per_head_loop():
    q, k, v = _inputs(1, 4, 2, 33, 33, 8, seed=4)
    rng = np.random.default_rng(2)
    do = rng.standard_normal(q.shape)
    sm = 0.5
    o, lse, _ = _autograd(q, k, v, do, None, True, sm)
    dq, dk, dv = attention_backward(q, k, v, o, lse, do, sm_scale=sm, is_causal=True)
    dk_loop, dv_loop = np.zeros_like(k), np.zeros_like(v)
    for h in range(4):
        hk = h // 2
        s = q[0, h] @ k[0, hk].T * sm
        s[np.triu_indices(33, 1)] = -np.inf
        p = np.exp(s - lse[0, h][:, None])
        dp = do[0, h] @ v[0, hk].T
        ds = p * (dp - (do[0, h] * o[0, h]).sum(-1)[:, None])
        assert np.allclose(dq[0, h], sm * ds @ k[0, hk], rtol=0, atol=1e-12)
        dk_loop[0, hk] += sm * ds.T @ q[0, h]
        dv_loop[0, hk] += p.T @ do[0, h]
    assert np.allclose(dk, dk_loop, rtol=0, atol=1e-12) and np.allclose(dv, dv_loop, rtol=0, atol=1e-12)


def test_smooth_k_invariance():
    """Smoothing shifts the keys by km and the LSE by q.km sm_scale: P is unchanged, and so are the gradients, which use the
    ORIGINAL K (with a dLSE flowing in as well)."""
    q, k, v = _inputs(1, 2, 2, 40, 40, 16, seed=8)
    rng = np.random.default_rng(3)
    do, dlse = rng.standard_normal(q.shape), rng.standard_normal(q.shape[:3])
    sm = 0.25
    o, lse, want = _autograd(q, k, v, do, dlse, False, sm)
    km = k.mean(axis=2, keepdims=True) + 0.7  # any shift
    p0 = recompute_p(q, k, lse, sm_scale=sm)
    p1 = recompute_p(q, k, lse, sm_scale=sm, km=km)  # scores of k - km, the correction q.km sm_scale taken out of lse
    assert np.abs(p1 - p0).max() <= 1e-12
    g0 = grads_from_p(p0, q, k, v, o, do, sm_scale=sm, dlse=dlse)
    g1 = attention_backward(q, k, v, o, lse, do, sm_scale=sm, dlse=dlse, km=km)
    for a, b, c in zip(g0, g1, want):
        assert np.abs(a - b).max() <= 1e-10 and np.abs(b - c).max() <= 1e-10 * max(1.0, np.abs(c).max())


def test_quantised_p_is_normalised_by_its_own_lse(oracle):
    """int8 codes: P recomputed from the oracle's codes and the oracle's LSE sums to 1 per row (the scores and the LSE
    correction are the forward's).  The oracle rounds its smooth-K correction dtype(q . km) from a numpy fp32 sum; the kernels,
    and so the reference, from their own order (bwd_reference.fwd_corr): the LSE is given the kernels' correction."""
    from bwd_reference import fwd_corr
    q, k, v = oracle.make_inputs(1, 2, 200, 64, seed=2, Hkv=1, k_bias=0.5)
    for smooth in (False, True):
        o, lse = oracle.lowbit_fa_forward(q, k, v, is_causal=True, smooth_k=smooth, return_lse=True, amax_floor=1e-7)
        if smooth:
            km = np.repeat(oracle.mean_seq(k, "fp16"), 2, axis=1)
            c_orc = oracle.to_storage(np.einsum("bhsd,bhtd->bhs", q.astype(np.float32), km.astype(np.float32)), "fp16")
            lse = (lse.astype(np.float64) + (fwd_corr(q, km, "fp16") - c_orc) * 64 ** -0.5).astype(np.float32)
        p = recompute_p(q, k, lse, sm_scale=64 ** -0.5, is_causal=True, q_qmax=127, k_qmax=127, smooth_k=smooth)
        assert np.abs(p.sum(-1) - 1).max() <= 1e-5


@pytest.mark.parametrize("causal,Hq,Hkv,Sq,Sk", [(False, 2, 2, 137, 150), (True, 4, 2, 145, 145), (False, 6, 2, 1, 129)])
def test_sampled_blocks_equal_the_full_gradients(causal, Hq, Hkv, Sq, Sk):
    """attention_backward_sampled on some 64-row blocks gives the rows of attention_backward bit for bit (the full form is the
    sampled form with all blocks), and the causal mask of a sampled block uses its absolute rows: it matches autograd."""
    q, k, v = _inputs(2, Hq, Hkv, Sq, Sk, 16, seed=Sq + Hq)
    rng = np.random.default_rng(5)
    do, dlse = rng.standard_normal(q.shape), rng.standard_normal(q.shape[:3])
    sm = 0.3
    o, lse, want = _autograd(q, k, v, do, dlse, causal, sm)
    full = attention_backward(q, k, v, o, lse, do, sm_scale=sm, is_causal=causal, dlse=dlse)
    qb, kb = [(Sq - 1) // 64], sorted({0, (Sk - 1) // 64})
    r = attention_backward_sampled(q, k, v, o, lse, do, sm_scale=sm, is_causal=causal, dlse=dlse, q_blocks=qb, k_blocks=kb)
    assert r["rows_q"][0] == 64 * qb[0] and r["rows_q"][-1] == Sq - 1 and r["rows_k"][0] == 0 and r["rows_k"][-1] == Sk - 1
    for name, f, w, rows in zip(("dq", "dk", "dv"), full, want, (r["rows_q"], r["rows_k"], r["rows_k"])):
        assert np.array_equal(r[name], f[:, :, rows]), name
        assert np.abs(r[name] - w[:, :, rows]).max() <= 1e-10 * max(1.0, np.abs(w).max())
