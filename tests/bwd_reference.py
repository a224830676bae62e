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

# ---- per-element error bound of a correct kernel (attention_backward(..., return_bound=True)); derivation in grad_bound ----
U32 = 2.0 ** -24                                  # fp32 unit roundoff (round to nearest even)
U_DT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}    # unit roundoff of the input dtype
TINY = {"fp16": 2.0 ** -14, "bf16": 2.0 ** -126}  # smallest normal number of the input dtype
EXP2_REL = 2.0 ** -23                             # __builtin_amdgcn_exp2f = v_exp_f32: 1 ulp (see grad_bound)
LOG2E_LIT = abs(LOG2E - 1.0 / np.log(2.0)) / (1.0 / np.log(2.0))  # the literal 1.44269504 against log2(e)
SAFETY = 2.0                                      # see grad_bound


def _rep(x, g):
    return np.repeat(x, g, axis=1) if g > 1 else x


def _mask(Sq, Sk, is_causal):
    if not is_causal:
        return np.ones((Sq, Sk), bool)
    return np.arange(Sk)[None, :] <= np.arange(Sq)[:, None]


def recompute_p(q, k, lse, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False, km=None,
                return_arg_err=False):
    """P [B, Hq, Sq, Sk] float64 from the forward's scores and its natural-log LSE [B, Hq, Sq].

    q_qmax = k_qmax = 0: un-quantised scores q.k * sm_scale (lbfa_sdpa_fwd), P = exp(s - lse).  `km` ([B, Hkv, 1, D]) then shifts the keys as
    smooth-K does, with the exact correction q.km taken out of the LSE (to check the invariance in float64).
    q_qmax in {127, 7}: the int8 / int4-range codes of `oracle.per_block_int8` (km = the oracle's mean when smooth_k) and the
    storage-dtype-rounded correction q.km of src/core.py:294-304, as the forward adds it to the LSE.
    return_arg_err: also the bound on the kernel's error in the exponent argument s2 - lse2 (binades, see grad_bound)."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    qd = q.astype(np.float64)
    mask = _mask(Sq, Sk, is_causal)
    if q_qmax == 0:
        # natural-log domain: the forward multiplies by and divides by the same log2(e) literal, which cancels
        kk = k.astype(np.float64) if km is None else k.astype(np.float64) - km.astype(np.float64)
        s = np.einsum("bhsd,bhtd->bhst", qd, _rep(kk, g), optimize=True) * sm_scale
        corr = np.zeros((B, Hq, Sq)) if km is None else np.einsum("bhsd,bhtd->bhs", qd, _rep(km.astype(np.float64), g), optimize=True)
        lsec = lse.astype(np.float64) - corr * sm_scale
        with np.errstate(invalid="ignore"):
            p = np.where(mask, np.exp(s - lsec[..., None]), 0.0)
        if not return_arg_err:
            return p
        # the kernel: a = fp32 MFMA sum of the D exact 16-bit products, fl(a * fl(sm_scale log2e)) - fl(lse * fl(log2e))
        sabs = np.einsum("bhsd,bhtd->bhst", np.abs(qd), _rep(np.abs(k.astype(np.float64)), g), optimize=True)
        s2, lse2 = s * LOG2E, lse.astype(np.float64) * LOG2E
        e = (U32 * (2 * np.abs(s2) + np.abs(s2 - lse2[..., None]) + 3 * np.abs(lse2)[..., None])
             + LOG2E_LIT * (np.abs(s2) + np.abs(lse2)[..., None]) + _gamma(D) * sabs * sm_scale * LOG2E * (1 + 3 * U32))
        return p, np.where(mask, e, 0.0)
    else:
        kmq = orc.mean_seq(k, dtype) if smooth_k else None
        q8, qs, k8, ks = orc.per_block_int8(q, k, kmq, sm_scale, dtype, q_qmax=float(q_qmax), k_qmax=float(k_qmax),
                                            amax_floor=1e-7)
        si = np.einsum("bhsd,bhtd->bhst", q8.astype(np.float64), _rep(k8.astype(np.float64), g), optimize=True)
        qsr = np.repeat(qs.astype(np.float64), 128, axis=2)[:, :, :Sq]
        ksr = np.repeat(ks.astype(np.float64), 64, axis=2)[:, :, :Sk]
        s2 = si * qsr[..., :, None] * _rep(ksr, g)[..., None, :]
        corr = fwd_corr(q, _rep(kmq, g), dtype) if smooth_k else np.zeros((B, Hq, Sq))
    lse2 = (lse.astype(np.float64) - corr * sm_scale) * LOG2E
    with np.errstate(over="ignore"):  # masked scores may lie far above the LSE
        p = np.where(mask, np.exp2(s2 - lse2[..., None]), 0.0)
    if not return_arg_err:
        return p
    return p, np.where(mask, quantised_arg_err(s2, lse2, corr * sm_scale), 0.0)


def fwd_corr(q, km, dtype):
    """the smooth-K correction dtype(q . km) [.., Sq] bit for bit as the kernels form it (q [.., Sq, D], km [.., 1, D], values of the
    dtype): the forward's in-kernel Q quantiser (attn_fwd16.hip, attn_fwd.hip) and the backward's pre-pass (attn_bwd.hip
    fwd_corr) sum the exact fp32 products of columns 64 s + 16 g + 0..15 (s ascending, D zero-padded to 64 / 128) in sequence
    for each g = 0..3, add (S0 + S1) + (S2 + S3) and round to the dtype.  Another order can round one dtype ulp away, which
    moves a whole row of P by that ulp times sm_scale log2(e)."""
    D = q.shape[-1]
    Dp = 64 if D <= 64 else 128
    prod = (q.astype(np.float32) * km.astype(np.float32)).astype(np.float32)
    if Dp != D:
        prod = np.concatenate([prod, np.zeros(prod.shape[:-1] + (Dp - D,), np.float32)], axis=-1)
    part = []
    for g in range(4):
        acc = np.zeros(prod.shape[:-1], np.float32)
        for s0 in range(0, Dp, 64):
            for c in range(s0 + 16 * g, s0 + 16 * g + 16):
                acc = (acc + prod[..., c]).astype(np.float32)
        part.append(acc)
    tot = ((part[0] + part[1]).astype(np.float32) + (part[2] + part[3]).astype(np.float32)).astype(np.float32)
    return orc.to_storage(tot, dtype).astype(np.float64)


def quantised_arg_err(s2, lse2, c):
    """bound (binades) on |(kernel's s2 - lse2) - (s2 - lse2)| for the quantised operators: s2 [.., Sq, Sk] = codes x q_scale x
    k_scale, lse2 [.., Sq] = (lse - c) log2e, c = the correction fwd_corr * sm_scale [.., Sq]  (derivation: grad_bound)"""
    s2, lse2, c = np.abs(s2), np.abs(lse2)[..., None], np.abs(c)[..., None]
    return U32 * (2 * s2 + np.abs(s2 - lse2) + 3 * lse2 + 3 * LOG2E * c)


def _gamma(n):
    """gamma_n = n u / (1 - n u): bound on the relative error of any fp32 sum of n terms, in any order"""
    return n * U32 / (1 - n * U32)


def _round_err(x, e, dtype):
    """bound on the rounding to `dtype` of a kernel value within e of the exact |x|: relative u, and the whole value where it
    may be subnormal (a round to the subnormal grid, a flush to zero: either is at most the value itself)"""
    hi = x + e
    return U_DT[dtype] * hi + np.where(x - e < TINY[dtype], np.minimum(hi, TINY[dtype]), 0.0)


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


def grad_bound(p, arg_err, q, k, v, o, do, *, sm_scale, dtype="fp16", dlse=None):
    """(bq, bk, bv) float64, shaped like dq / dk / dv: the largest |kernel - reference| a correct attn_bwd.hip can show, element
    by element, for P [B, Hq, Sq, Sk] (recompute_p) and the bound `arg_err` on its exponent argument.

    The kernel's arithmetic, as written (attn_bwd.hip, lbfa_backward; built with -ffp-contract=off, so every product and
    sum rounds on its own; u32 = 2^-24):
      argument  quantised: a = the integer code dot product (exact), sc = fl(q_scale k_scale), x = fl(fl(a sc) - lse2);
                un-quantised: a = fp32 MFMA sum of the D exact 16-bit products, sc = fl(sm_scale 1.44269504).
                lse2 = fl(fl(lse - fl(corr fl(sm_scale))) fl(1.44269504)) in the pre-pass.  Each rounding is relative to a
                quantity of size |s2| or |lse2|, so the argument error is
                  u32 (2|s2| + |s2 - lse2| + 3|lse2| + 3 log2e |corr sm_scale|)          (recompute_p / quantised_arg_err)
                corr = dtype(q . km) is restated bit for bit in the kernels' order (fwd_corr): the one the forward added.
                plus, un-quantised, gamma_D sum_d |q||k| sm_scale log2e (the fp32 dot product) and the relative difference
                of the literal 1.44269504 from log2(e) times |s2| + |lse2| (the reference is natural-log there).
                This grows with the scores: at |s2| ~ |lse2| ~ 2^14 binades (randint inputs, D = 128) it is ~2^-8 binades,
                more than the fp16 rounding of P.
      P         fl(exp2(x)): v_exp_f32 is accurate to 1 ulp (AMD Instinct CDNA3 ISA reference guide, V_EXP_F32; the HIP math
                library's exp2f, built on it, documents the same 1 ulp), so P_k = P 2^(+-arg_err) (1 +- 2^-23); a subnormal
                result may be flushed (at most P itself).
      P, dS     rounded once each to the input dtype (pack_pair: store_cvt) - relative u = 2^-11 (fp16) / 2^-8 (bf16).  Whether
                the f16 / bf16 A / B inputs of v_mfma_f32_16x16x32_{f16,bf16} flush subnormals on gfx950 is not settled by
                the ISA text at hand (it covers C / D and f32 A / B), so the flush is modelled: below the smallest normal the
                error is the whole value (_round_err).
      dP, delta dP = fp32 MFMA sum over D: gamma_D sum_d |dO||V|; delta = fp32 fma chain over D, then - dLSE:
                gamma_(D+1) (sum_d |dO||O| + |dLSE|).
      dS        fl(P_k fl(dP - delta)): the errors of P_k, dP and delta propagated, plus two fp32 roundings.
      outputs   fp32 MFMA sums over the keys (dq: Sk terms) or over the group's query rows (dk / dv: group x Sq terms):
                sum |error of each term| + gamma_N sum |term|; dq / dk times fl(sm_scale) (two more fp32 roundings); each
                stored in the dtype (_round_err).
    The MFMA sums are k-ordered fp32 fma chains with one round-to-nearest rounding per step, which gamma_N covers in any
    order.  SAFETY = 2 is margin, not a missing term: on a correct kernel the worst element is one output's own rounding to
    the dtype, which reaches about 0.95 of the un-scaled bound (worst 0.48 of the scaled one in the GPU tests), so the bound
    is tight there; and two inputs of the derivation are documented facts rather than derived from this code (the 1-ulp
    accuracy of v_exp_f32; that no unit on the path flushes or rounds other than as modelled).  The factor keeps an error
    in either from failing a correct kernel; test_bwd_bound_cpu.py shows every listed bug is still rejected with it."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    u = U_DT[dtype]
    aq, ak, av, ao, ado = (np.abs(x.astype(np.float64)) for x in (q, k, v, o, do))
    ak, av = _rep(ak, g), _rep(av, g)
    # P before (eP) and after (ePr) its rounding to the dtype
    with np.errstate(over="ignore"):
        rho = np.exp2(arg_err) * (1 + EXP2_REL) - 1
    eP = p * rho + np.minimum(p * (1 + rho), TINY["bf16"])
    ePr = eP + _round_err(p, eP, dtype)
    # dP - delta and dS
    dp = np.einsum("bhsd,bhtd->bhst", do.astype(np.float64), _rep(v.astype(np.float64), g), optimize=True)
    delta = np.sum(do.astype(np.float64) * o.astype(np.float64), axis=-1)
    adl = np.zeros((B, Hq, Sq)) if dlse is None else np.abs(dlse.astype(np.float64))
    if dlse is not None:
        delta = delta - dlse.astype(np.float64)
    t = np.abs(dp - delta[..., None])
    et = (_gamma(D) * np.einsum("bhsd,bhtd->bhst", ado, av, optimize=True)
          + (_gamma(D + 1) * (np.sum(ado * ao, axis=-1) + adl))[..., None])
    et = et * (1 + U32) + U32 * t
    ds = p * t
    eds = eP * (t + et) + p * et + U32 * (p + eP) * (t + et)
    edsr = eds + _round_err(ds, eds, dtype)

    # outputs: sum |term error| + gamma_N sum |term|; dq / dk times fl(sm_scale)
    pr_mag = p + ePr
    ev = np.einsum("bhst,bhsd->bhtd", ePr, ado, optimize=True) + _gamma(g * Sq) * np.einsum("bhst,bhsd->bhtd", pr_mag, ado, optimize=True)
    ds_mag = ds + edsr
    ek = sm_scale * (np.einsum("bhst,bhsd->bhtd", edsr, aq, optimize=True)
                     + (_gamma(g * Sq) + 2 * U32) * np.einsum("bhst,bhsd->bhtd", ds_mag, aq, optimize=True))
    eq = sm_scale * (np.einsum("bhst,bhtd->bhsd", edsr, ak, optimize=True)
                     + (_gamma(Sk) + 2 * U32) * np.einsum("bhst,bhtd->bhsd", ds_mag, ak, optimize=True))
    ev = ev.reshape(B, Hkv, g, Sk, D).sum(axis=2)
    ek = ek.reshape(B, Hkv, g, Sk, D).sum(axis=2)
    dq, dk, dv = grads_from_p(p, q, k, v, o, do, sm_scale=sm_scale, dlse=dlse)
    return tuple(SAFETY * (e + _round_err(np.abs(x), e, dtype)) for x, e in ((dq, eq), (dk, ek), (dv, ev)))


def attention_backward(q, k, v, o, lse, do, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False,
                       dlse=None, km=None, return_bound=False):
    """(dq, dk, dv) float64 of the contract: P recomputed (recompute_p), then grads_from_p.  o and lse are the operator's.
    return_bound: (dq, dk, dv, bq, bk, bv), the b* the per-element bound of grad_bound (the largest deviation of a correct
    kernel from dq / dk / dv)."""
    p = recompute_p(q, k, lse, sm_scale=sm_scale, is_causal=is_causal, dtype=dtype, q_qmax=q_qmax, k_qmax=k_qmax,
                    smooth_k=smooth_k, km=km, return_arg_err=return_bound)
    if not return_bound:
        return grads_from_p(p, q, k, v, o, do, sm_scale=sm_scale, dlse=dlse)
    p, e = p
    return (grads_from_p(p, q, k, v, o, do, sm_scale=sm_scale, dlse=dlse)
            + grad_bound(p, e, q, k, v, o, do, sm_scale=sm_scale, dtype=dtype, dlse=dlse))
