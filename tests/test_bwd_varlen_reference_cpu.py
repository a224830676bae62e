"""The float64 restatement of the packed-batch backward (bwd_varlen_reference.py) against the dense one and against torch
autograd: it is the dense contract sequence by sequence, and its packing and slicing carry the right rows."""
import numpy as np
import pytest

from bwd_reference import attention_backward
from bwd_varlen_reference import packed_codes, varlen_backward, varlen_lse
from oracle import lowbit_fa_oracle as orc

torch = pytest.importorskip("torch")


def _dense(x, c, b):
    return np.transpose(x[c[b]:c[b + 1]], (1, 0, 2))[None]


def _packed(x):
    return np.transpose(x[0], (1, 0, 2))


def _inputs(lens_q, lens_k, Hq, Hkv, D, seed, causal, smooth_k=True, q_qmax=127):
    q, k, v, cu_q, cu_k = orc.make_varlen_inputs(lens_q, lens_k, Hq, Hkv, D, seed=seed, k_bias=0.4)
    o = orc.lowbit_fa_varlen(q, k, v, cu_q, cu_k, is_causal=causal, smooth_k=smooth_k, q_qmax=float(q_qmax), tail="neg_inf",
                             amax_floor=1e-7)
    lse = varlen_lse(q, k, v, cu_q, cu_k, is_causal=causal, smooth_k=smooth_k, q_qmax=q_qmax)
    do = orc.to_storage(np.random.default_rng(seed + 1).standard_normal(q.shape).astype(np.float32), "fp16")
    return q, k, v, o, lse, do, cu_q, cu_k


@pytest.mark.parametrize("causal", [False, True])
def test_one_sequence_is_the_dense_restatement(causal):
    q, k, v, o, lse, do, cu_q, cu_k = _inputs([200], [200], 4, 2, 64, 3, causal)
    dlse = np.random.default_rng(5).standard_normal(lse.shape)
    got = varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, is_causal=causal, dlse=dlse)
    ref = attention_backward(_dense(q, cu_q, 0), _dense(k, cu_k, 0), _dense(v, cu_k, 0), _dense(o, cu_q, 0), lse[None], _dense(do, cu_q, 0),
                             sm_scale=64 ** -0.5, is_causal=causal, q_qmax=127, k_qmax=127, smooth_k=True, dlse=dlse[None])
    for g, r in zip(got, ref):
        np.testing.assert_allclose(g, _packed(r), rtol=1e-12, atol=1e-14)


def test_sequences_without_smooth_k_are_independent_dense_problems():
    lens = [1, 63, 129, 70]
    q, k, v, o, lse, do, cu_q, cu_k = _inputs(lens, lens, 2, 2, 64, 7, False, smooth_k=False)
    got = varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, smooth_k=False)
    for b in range(len(lens)):
        ref = attention_backward(_dense(q, cu_q, b), _dense(k, cu_k, b), _dense(v, cu_k, b), _dense(o, cu_q, b),
                                 lse[:, cu_q[b]:cu_q[b + 1]][None], _dense(do, cu_q, b), sm_scale=64 ** -0.5, q_qmax=127,
                                 k_qmax=127, smooth_k=False)
        for g, r, c in zip(got, ref, (cu_q, cu_k, cu_k)):
            np.testing.assert_allclose(g[c[b]:c[b + 1]], _packed(r), rtol=1e-12, atol=1e-14)


def test_lse_rows_of_keyless_and_queryless_sequences():
    q, k, v, cu_q, cu_k = orc.make_varlen_inputs([5, 0, 9], [7, 3, 0], 2, 1, 64, seed=1)
    lse = varlen_lse(q, k, v, cu_q, cu_k)
    assert np.all(np.isfinite(lse[:, :5])) and np.all(lse[:, 5:] == -np.inf)


@pytest.mark.parametrize("causal", [False, True])
def test_packing_matches_torch_autograd_of_float64_attention(causal):
    """P from float64 un-quantised scores: packed gradients equal torch autograd of float64 attention per sequence, with a
    loss on o and on the LSE.  Empty query / key ranges get zero gradients."""
    lens_q = [3, 0, 17, 40, 9] if not causal else [3, 0, 17, 40, 0]
    lens_k = [5, 6, 17, 33, 0] if not causal else [3, 0, 17, 40, 0]
    Hq, Hkv, D = 4, 2, 16
    q, k, v, cu_q, cu_k = orc.make_varlen_inputs(lens_q, lens_k, Hq, Hkv, D, seed=11)
    sm = D ** -0.5
    rng = np.random.default_rng(2)
    do = rng.standard_normal(q.shape)
    dlse = rng.standard_normal((Hq, q.shape[0]))
    o = np.zeros(q.shape)
    lse = np.full((Hq, q.shape[0]), -np.inf)
    want = [np.zeros(x.shape) for x in (q, k, v)]
    for b in range(len(lens_q)):
        if lens_q[b] == 0 or lens_k[b] == 0:
            continue
        tq, tk, tv = (torch.tensor(_dense(x, c, b)[0], dtype=torch.float64, requires_grad=True)
                      for x, c in ((q, cu_q), (k, cu_k), (v, cu_k)))
        s = torch.einsum("hsd,htd->hst", tq, tk.repeat_interleave(Hq // Hkv, 0)) * sm
        if causal:
            s = s.masked_fill(~torch.ones(s.shape[1:], dtype=torch.bool).tril(), float("-inf"))
        ls = torch.logsumexp(s, -1)
        ob = torch.einsum("hst,htd->hsd", torch.softmax(s, -1), tv.repeat_interleave(Hq // Hkv, 0))
        (ob * torch.tensor(_dense(do, cu_q, b)[0])).sum().add((ls * torch.tensor(dlse[:, cu_q[b]:cu_q[b + 1]])).sum()).backward()
        o[cu_q[b]:cu_q[b + 1]] = _packed(ob.detach().numpy()[None])
        lse[:, cu_q[b]:cu_q[b + 1]] = ls.detach().numpy()
        for w, t, c in zip(want, (tq, tk, tv), (cu_q, cu_k, cu_k)):
            w[c[b]:c[b + 1]] = _packed(t.grad.numpy()[None])

    def p_fn(b, qb, kb, lb, sm_scale):
        g = qb.shape[1] // kb.shape[1]
        s = np.einsum("bhsd,bhtd->bhst", qb.astype(np.float64), np.repeat(kb, g, axis=1).astype(np.float64)) * sm_scale
        p = np.exp(s - lb[None, ..., None])
        return np.where(np.tril(np.ones(s.shape[2:], bool)), p, 0.0) if causal else p

    got = varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, is_causal=causal, dlse=dlse, p_fn=p_fn)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("D,smooth_k,qmax", [(64, True, 127), (80, True, 7), (128, False, 127)])
def test_packed_codes_are_the_oracles(D, smooth_k, qmax):
    """packed_codes (no attention, linear in the lengths) gives the intermediates of oracle.lowbit_fa_varlen bit for bit"""
    lens_q, lens_k = [70, 0, 129, 5, 1], [3, 40, 129, 0, 200]
    q, k, v, cu_q, cu_k = orc.make_varlen_inputs(lens_q, lens_k, 4, 2, D, seed=D, k_bias=0.4)
    _, want = orc.lowbit_fa_varlen(q, k, v, cu_q, cu_k, smooth_k=smooth_k, q_qmax=float(qmax), k_qmax=float(qmax), tail="neg_inf",
                                   amax_floor=1e-7, return_intermediates=True)
    got = packed_codes(q, k, cu_q, cu_k, dtype="fp16", sm_scale=D ** -0.5, smooth_k=smooth_k, q_qmax=qmax, k_qmax=qmax)
    for name in ("q_i8", "k_i8", "q_scale", "k_scale"):
        assert np.array_equal(got[name], want[name]), name
    assert (got["km"] is None and want["km"] is None) if not smooth_k else np.array_equal(got["km"], want["km"])


@pytest.mark.parametrize("causal", [False, True])
def test_sampled_blocks_of_a_sequence_equal_the_full_packed_result(causal):
    """`blocks` samples 64-row blocks of the named sequences: values and bounds equal the full result bit for bit on the tokens
    the returned masks name, the other tokens of those sequences stay zero, the other sequences are computed completely."""
    lens = [70, 300, 0, 131]
    q, k, v, o, lse, do, cu_q, cu_k = _inputs(lens, lens, 4, 2, 64, 9, causal)
    dlse = np.random.default_rng(6).standard_normal(lse.shape)
    full = varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, is_causal=causal, dlse=dlse, return_bound=True)
    got = varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, is_causal=causal, dlse=dlse, return_bound=True,
                          blocks={1: ([1, 4], [0, 4]), 3: ([], None)})
    mq, mk = got[6:]
    want_q = np.ones(q.shape[0], bool)
    want_q[cu_q[1]:cu_q[2]] = False
    want_q[cu_q[1] + 64:cu_q[1] + 128] = want_q[cu_q[1] + 256:cu_q[2]] = True
    want_q[cu_q[3]:cu_q[4]] = False
    want_k = np.ones(k.shape[0], bool)
    want_k[cu_k[1] + 64:cu_k[1] + 256] = False
    assert np.array_equal(mq, want_q) and np.array_equal(mk, want_k)
    for i, m in enumerate((mq, mk, mk, mq, mk, mk)):
        assert np.array_equal(got[i][m], full[i][m]) and not got[i][~m].any(), i
