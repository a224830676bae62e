"""CPU float64 restatement of the attention backward contract (include/lowbit_fa.h `lbfa_backward`, DESIGN.md "Backward").

Straight-through on the quantiser: P is the forward's own P, recomputed from the scores the forward used and the LSE it
returned, P = exp2(s2 - lse2); the gradient products use the un-quantised q, k, v:
    dV = P^T dO,  dP = dO V^T,  delta = rowsum(dO o O) - dLSE,  dS = P o (dP - delta),  dQ = sm_scale dS K,  dK = sm_scale dS^T Q.
Arrays are canonical [B, H, S, D] (fp32 values already rounded to the storage dtype); Hq % Hkv == 0 (GQA: dk / dv of a kv head
sum over its query heads).  The codes and scales come from `oracle.per_block_int8`, so the scores are the forward's.
"""
from __future__ import annotations

import numpy as np

from oracle import lowbit_fa_oracle as orc

LOG2E = 1.44269504


def _rep(x, g):
    return np.repeat(x, g, axis=1) if g > 1 else x


def _mask(Sq, Sk, is_causal):
    if not is_causal:
        return np.ones((Sq, Sk), bool)
    return np.arange(Sk)[None, :] <= np.arange(Sq)[:, None]


def recompute_p(q, k, lse, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False, km=None):
    """P [B, Hq, Sq, Sk] float64 from the forward's scores and its natural-log LSE [B, Hq, Sq].

    q_qmax = k_qmax = 0: un-quantised scores q.k * sm_scale (lbfa_sdpa_fwd), P = exp(s - lse).  `km` ([B, Hkv, 1, D]) then shifts the keys as
    smooth-K does, with the exact correction q.km taken out of the LSE (to check the invariance in float64).
    q_qmax in {127, 7}: the int8 / int4-range codes of `oracle.per_block_int8` (km = the oracle's mean when smooth_k) and the
    storage-dtype-rounded correction q.km of src/core.py:294-304, as the forward adds it to the LSE."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    qd = q.astype(np.float64)
    if q_qmax == 0:
        # natural-log domain: the forward multiplies by and divides by the same log2(e) literal, which cancels
        kk = k.astype(np.float64) if km is None else k.astype(np.float64) - km.astype(np.float64)
        s = np.einsum("bhsd,bhtd->bhst", qd, _rep(kk, g), optimize=True) * sm_scale
        corr = np.zeros((B, Hq, Sq)) if km is None else np.einsum("bhsd,bhtd->bhs", qd, _rep(km.astype(np.float64), g), optimize=True)
        p = np.exp(s - (lse.astype(np.float64) - corr * sm_scale)[..., None])
        return np.where(_mask(Sq, Sk, is_causal), p, 0.0)
    else:
        kmq = orc.mean_seq(k, dtype) if smooth_k else None
        q8, qs, k8, ks = orc.per_block_int8(q, k, kmq, sm_scale, dtype, q_qmax=float(q_qmax), k_qmax=float(k_qmax),
                                            amax_floor=1e-7)
        si = np.einsum("bhsd,bhtd->bhst", q8.astype(np.float64), _rep(k8.astype(np.float64), g), optimize=True)
        qsr = np.repeat(qs.astype(np.float64), 128, axis=2)[:, :, :Sq]
        ksr = np.repeat(ks.astype(np.float64), 64, axis=2)[:, :, :Sk]
        s2 = si * qsr[..., :, None] * _rep(ksr, g)[..., None, :]
        if smooth_k:
            corr = orc.to_storage(np.einsum("bhsd,bhtd->bhs", q.astype(np.float32), _rep(kmq, g).astype(np.float32)),
                                  dtype).astype(np.float64)
        else:
            corr = np.zeros((B, Hq, Sq))
    lse2 = (lse.astype(np.float64) - corr * sm_scale) * LOG2E
    p = np.exp2(s2 - lse2[..., None])
    return np.where(_mask(Sq, Sk, is_causal), p, 0.0)


def grads_from_p(p, q, k, v, o, do, *, sm_scale, dlse=None):
    """(dq, dk, dv) float64 for a given P [B, Hq, Sq, Sk]"""
    Hq, Hkv = q.shape[1], k.shape[1]
    g = Hq // Hkv
    qd, kd, vd, od, dod = (x.astype(np.float64) for x in (q, k, v, o, do))
    dv_h = np.einsum("bhst,bhsd->bhtd", p, dod, optimize=True)
    dp = np.einsum("bhsd,bhtd->bhst", dod, _rep(vd, g), optimize=True)
    delta = np.sum(dod * od, axis=-1)
    if dlse is not None:
        delta = delta - dlse.astype(np.float64)
    ds = p * (dp - delta[..., None])
    dq = sm_scale * np.einsum("bhst,bhtd->bhsd", ds, _rep(kd, g), optimize=True)
    dk_h = sm_scale * np.einsum("bhst,bhsd->bhtd", ds, qd, optimize=True)
    B, _, Sk, D = k.shape
    dk = dk_h.reshape(B, Hkv, g, Sk, D).sum(axis=2)
    dv = dv_h.reshape(B, Hkv, g, Sk, v.shape[-1]).sum(axis=2)
    return dq, dk, dv


def attention_backward(q, k, v, o, lse, do, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False,
                       dlse=None, km=None):
    """(dq, dk, dv) float64 of the contract: P recomputed (recompute_p), then grads_from_p.  o and lse are the operator's."""
    p = recompute_p(q, k, lse, sm_scale=sm_scale, is_causal=is_causal, dtype=dtype, q_qmax=q_qmax, k_qmax=k_qmax,
                    smooth_k=smooth_k, km=km)
    return grads_from_p(p, q, k, v, o, do, sm_scale=sm_scale, dlse=dlse)
