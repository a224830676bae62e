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
HALF_SUB = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134}  # half a step of its subnormal grid
BLK = 64                                          # rows of a dQ workgroup / keys of a dK / dV workgroup
EXP2_REL = 2.0 ** -23                             # __builtin_amdgcn_exp2f = v_exp_f32: 1 ulp (see grad_bound)
LOG2E_LIT = abs(LOG2E - 1.0 / np.log(2.0)) / (1.0 / np.log(2.0))  # the literal 1.44269504 against log2(e)
SAFETY = 2.0                                      # see grad_bound


def _rep(x, g):
    return np.repeat(x, g, axis=1) if g > 1 else x


def _block_rows(blocks, S):
    """absolute rows of the 64-row blocks `blocks` (ascending; None: every row) of a sequence of S rows - the dQ workgroup's query
    rows or the dK / dV workgroup's keys (oracle.block_rows with 64-row blocks)"""
    if blocks is None:
        return np.arange(S)
    return orc.block_rows(blocks, S, BLK) if len(blocks) else np.zeros(0, np.int64)


def _all_blocks(S):
    return [[b] for b in range(-(-S // BLK))]


def prepare_p(q, k, lse, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False, km=None):
    """What P needs of the whole tensors, O(S D): the codes and scales of `oracle.per_block_int8` over the whole tensor, the
    correction fwd_corr and lse2 of every row (q_qmax = k_qmax = 0: the float64 q, shifted k and corrected natural-log LSE).
    -> the context `p_panel` takes."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    c = dict(g=g, causal=is_causal, quant=q_qmax != 0, sm=sm_scale, D=D, Sq=Sq, Sk=Sk)
    if q_qmax == 0:
        qd = q.astype(np.float64)
        c["qd"] = qd
        c["kk"] = k.astype(np.float64) if km is None else k.astype(np.float64) - km.astype(np.float64)
        corr = np.zeros((B, Hq, Sq)) if km is None else np.einsum("bhsd,bhtd->bhs", qd, _rep(km.astype(np.float64), g), optimize=True)
        c["lsec"] = lse.astype(np.float64) - corr * sm_scale
        c["lse2"] = lse.astype(np.float64) * LOG2E
        c["aq"], c["ak"] = np.abs(qd), np.abs(k.astype(np.float64))
        return c
    kmq = orc.mean_seq(k, dtype) if smooth_k else None
    q8, qs, k8, ks = orc.per_block_int8(q, k, kmq, sm_scale, dtype, q_qmax=float(q_qmax), k_qmax=float(k_qmax), amax_floor=1e-7)
    corr = fwd_corr(q, _rep(kmq, g), dtype) if smooth_k else np.zeros((B, Hq, Sq))
    return quantised_context(q8, qs, k8, ks, corr, lse, sm_scale, is_causal)


def quantised_context(q8, qs, k8, ks, corr, lse, sm_scale, is_causal):
    """the context of `p_panel` from codes [B, H, S, D], scales [B, H, blocks], the correction dtype(q . km) [B, Hq, Sq] and the
    operator's natural-log LSE [B, Hq, Sq]"""
    Sq, Sk = q8.shape[2], k8.shape[2]
    c = dict(g=q8.shape[1] // k8.shape[1], causal=is_causal, quant=True, sm=sm_scale, D=q8.shape[3], Sq=Sq, Sk=Sk, q8=q8, k8=k8)
    c["qsr"] = np.repeat(qs.astype(np.float64), 128, axis=2)[:, :, :Sq]
    c["ksr"] = np.repeat(ks.astype(np.float64), 64, axis=2)[:, :, :Sk]
    c["corrsm"] = corr.astype(np.float64) * sm_scale
    c["lse2"] = (lse.astype(np.float64) - c["corrsm"]) * LOG2E
    return c


def p_panel(c, b, hk, rows, cols, return_arg_err=False):
    """P [g, rows, cols] float64 of the g query heads of kv head (b, hk) at the absolute query rows `rows` and keys `cols`
    (causal: key <= row, absolute), and on request the bound on the kernel's exponent-argument error (grad_bound)"""
    g = c["g"]
    hs = slice(hk * g, (hk + 1) * g)
    mask = (cols[None, :] <= rows[:, None]) if c["causal"] else np.ones((len(rows), len(cols)), bool)
    if not c["quant"]:
        # natural-log domain: the forward multiplies by and divides by the same log2(e) literal, which cancels
        qd, kk = c["qd"][b, hs][:, rows], c["kk"][b, hk][cols]
        s = np.matmul(qd, kk.T) * c["sm"]
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.where(mask, np.exp(s - c["lsec"][b, hs][:, rows][..., None]), 0.0)
        if not return_arg_err:
            return p
        # the kernel: a = fp32 MFMA sum of the D exact 16-bit products, fl(a * fl(sm_scale log2e)) - fl(lse * fl(log2e))
        sabs = np.matmul(c["aq"][b, hs][:, rows], c["ak"][b, hk][cols].T)
        s2, lse2 = s * LOG2E, c["lse2"][b, hs][:, rows][..., None]
        e = (U32 * (2 * np.abs(s2) + np.abs(s2 - lse2) + 3 * np.abs(lse2))
             + LOG2E_LIT * (np.abs(s2) + np.abs(lse2)) + _gamma(c["D"]) * sabs * c["sm"] * LOG2E * (1 + 3 * U32))
        return p, np.where(mask, e, 0.0)
    si = np.matmul(c["q8"][b, hs][:, rows].astype(np.float64), c["k8"][b, hk][cols].astype(np.float64).T)
    s2 = si * c["qsr"][b, hs][:, rows][..., None] * c["ksr"][b, hk][cols][None, None, :]
    lse2 = c["lse2"][b, hs][:, rows]
    with np.errstate(over="ignore"):  # masked scores may lie far above the LSE
        p = np.where(mask, np.exp2(s2 - lse2[..., None]), 0.0)
    if not return_arg_err:
        return p
    return p, np.where(mask, quantised_arg_err(s2, lse2, c["corrsm"][b, hs][:, rows]), 0.0)


def recompute_p(q, k, lse, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False, km=None,
                return_arg_err=False):
    """P [B, Hq, Sq, Sk] float64 from the forward's scores and its natural-log LSE [B, Hq, Sq] (p_panel over all rows and keys).

    q_qmax = k_qmax = 0: un-quantised scores q.k * sm_scale (lbfa_sdpa_fwd), P = exp(s - lse).  `km` ([B, Hkv, 1, D]) then shifts the keys as
    smooth-K does, with the exact correction q.km taken out of the LSE (to check the invariance in float64).
    q_qmax in {127, 7}: the int8 / int4-range codes of `oracle.per_block_int8` (km = the oracle's mean when smooth_k) and the
    storage-dtype-rounded correction q.km of src/core.py:294-304, as the forward adds it to the LSE.
    return_arg_err: also the bound on the kernel's error in the exponent argument s2 - lse2 (binades, see grad_bound)."""
    B, Hq, Sq, _ = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    c = prepare_p(q, k, lse, sm_scale=sm_scale, is_causal=is_causal, dtype=dtype, q_qmax=q_qmax, k_qmax=k_qmax, smooth_k=smooth_k, km=km)
    p, e = np.zeros((B, Hq, Sq, Sk)), (np.zeros((B, Hq, Sq, Sk)) if return_arg_err else None)
    rows, cols = np.arange(Sq), np.arange(Sk)
    for b in range(B):
        for hk in range(Hkv):
            r = p_panel(c, b, hk, rows, cols, return_arg_err)
            if return_arg_err:
                p[b, hk * g:(hk + 1) * g], e[b, hk * g:(hk + 1) * g] = r
            else:
                p[b, hk * g:(hk + 1) * g] = r
    return (p, e) if return_arg_err else p


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
    """bound on the rounding to `dtype` of a kernel value within e of the exact |x|: relative u, and below the smallest normal
    half a step of the subnormal grid (the 16-bit conversion and the MFMA keep subnormals: grad_bound), and never more than
    the value itself (below half a step it rounds to zero; an exact zero, a masked P, stays zero)"""
    hi = x + e
    return np.minimum(hi, np.maximum(U_DT[dtype] * hi, HALF_SUB[dtype]))


def sampled_from_p(p_fn, q, k, v, o, do, *, sm_scale, dtype="fp16", dlse=None, q_blocks=None, k_blocks=None, return_bound=False,
                   workers=1):
    """The gradients on sampled 64-row blocks, in O(S D) + O(64 S) memory per head: dq (and its bound) on the rows of the query
    blocks `q_blocks` - P rows against all keys - and dk, dv (and their bounds) on the rows of the key blocks `k_blocks` - P
    columns against all queries of the kv head's whole group.  None: every block (the full gradients), [] : none.
    `p_fn(b, hk, rows, cols)` gives P [g, rows, cols] (return_bound: and the argument bound) - p_panel.  delta is formed for
    all rows from o and do.  One 64-row block at a time, so a block's result does not depend on which others are asked for
    (`workers`: that many blocks at a time, on threads).
    -> dict(dq, dk, dv [B, H, sampled rows, D], rows_q, rows_k) and, with return_bound, bq, bk, bv (derivation: grad_bound)."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    qd, kd, vd, od, dod = (x.astype(np.float64) for x in (q, k, v, o, do))
    delta = np.sum(dod * od, axis=-1)
    adl = np.zeros((B, Hq, Sq)) if dlse is None else np.abs(dlse.astype(np.float64))
    if dlse is not None:
        delta = delta - dlse.astype(np.float64)
    if return_bound:
        aq, ak, av, ado = (np.abs(x) for x in (qd, kd, vd, dod))
        edelta = _gamma(D + 1) * (np.sum(ado * np.abs(od), axis=-1) + adl)
    qbl = _all_blocks(Sq) if q_blocks is None else [[int(x)] for x in q_blocks]
    kbl = _all_blocks(Sk) if k_blocks is None else [[int(x)] for x in k_blocks]
    rows_q = np.concatenate([_block_rows(x, Sq) for x in qbl]) if qbl else np.zeros(0, np.int64)
    rows_k = np.concatenate([_block_rows(x, Sk) for x in kbl]) if kbl else np.zeros(0, np.int64)
    res = dict(rows_q=rows_q, rows_k=rows_k, dq=np.zeros((B, Hq, len(rows_q), D)), dk=np.zeros((B, Hkv, len(rows_k), D)),
               dv=np.zeros((B, Hkv, len(rows_k), v.shape[-1])))
    if return_bound:
        res.update(bq=np.zeros_like(res["dq"]), bk=np.zeros_like(res["dk"]), bv=np.zeros_like(res["dv"]))
    all_q, all_k = np.arange(Sq), np.arange(Sk)

    def panel(b, hk, rows, cols):
        """P, dS [g, rows, cols] and, for the bound, the errors of P and dS after their rounding to the dtype and the magnitudes
        the fp32 sums run over"""
        hs = slice(hk * g, (hk + 1) * g)
        p = p_fn(b, hk, rows, cols)
        if return_bound:
            p, arg_err = p
        dor = dod[b, hs][:, rows]
        dp = np.matmul(dor, vd[b, hk][cols].T)
        tt = dp - delta[b, hs][:, rows][..., None]
        ds = p * tt
        if not return_bound:
            return p, ds, None
        # P before (eP) and after (ePr) its rounding to the dtype
        with np.errstate(over="ignore"):
            rho = np.exp2(arg_err) * (1 + EXP2_REL) - 1
        eP = p * rho + np.minimum(p * (1 + rho), TINY["bf16"])
        ePr = eP + _round_err(p, eP, dtype)
        t = np.abs(tt)
        et = (_gamma(D) * np.matmul(ado[b, hs][:, rows], av[b, hk][cols].T)
              + edelta[b, hs][:, rows][..., None])
        et = et * (1 + U32) + U32 * t
        ads = p * t
        eds = eP * (t + et) + p * et + U32 * (p + eP) * (t + et)
        edsr = eds + _round_err(ads, eds, dtype)
        return p, ds, (ePr, p + ePr, edsr, ads + edsr)

    def store(x, e):
        return SAFETY * (e + _round_err(np.abs(x), e, dtype))

    def dq_block(b, hk, rows, sl):  # dq: sum over the keys (Sk terms), times fl(sm_scale)
        hs = slice(hk * g, (hk + 1) * g)
        p, ds, eb = panel(b, hk, rows, all_k)
        dq = sm_scale * np.matmul(ds, kd[b, hk])
        res["dq"][b, hs, sl] = dq
        if return_bound:
            _, _, edsr, ds_mag = eb
            eq = sm_scale * (np.matmul(edsr, ak[b, hk])
                             + (_gamma(Sk) + 2 * U32) * np.matmul(ds_mag, ak[b, hk]))
            res["bq"][b, hs, sl] = store(dq, eq)

    def dkv_block(b, hk, cols, sl):  # dk / dv: sum over the group's query rows (g Sq terms); dk times fl(sm_scale)
        hs = slice(hk * g, (hk + 1) * g)
        p, ds, eb = panel(b, hk, all_q, cols)
        dk = sm_scale * np.matmul(ds.transpose(0, 2, 1), qd[b, hs]).sum(axis=0)
        dv = np.matmul(p.transpose(0, 2, 1), dod[b, hs]).sum(axis=0)
        res["dk"][b, hk, sl], res["dv"][b, hk, sl] = dk, dv
        if return_bound:
            ePr, pr_mag, edsr, ds_mag = eb
            ev = (np.matmul(ePr.transpose(0, 2, 1), ado[b, hs])
                  + _gamma(g * Sq) * np.matmul(pr_mag.transpose(0, 2, 1), ado[b, hs])).sum(axis=0)
            ek = sm_scale * (np.matmul(edsr.transpose(0, 2, 1), aq[b, hs])
                             + (_gamma(g * Sq) + 2 * U32) * np.matmul(ds_mag.transpose(0, 2, 1), aq[b, hs])).sum(axis=0)
            res["bk"][b, hk, sl], res["bv"][b, hk, sl] = store(dk, ek), store(dv, ev)

    tasks = []
    for b in range(B):
        for hk in range(Hkv):
            for fn, bl, S in ((dq_block, qbl, Sq), (dkv_block, kbl, Sk)):
                at = 0
                for blk in bl:
                    rows = _block_rows(blk, S)
                    tasks.append((fn, b, hk, rows, slice(at, at + len(rows))))
                    at += len(rows)
    limits = None
    if workers > 1:  # each thread's BLAS must then stay single-threaded, or the threads fight over the cores
        try:
            from threadpoolctl import threadpool_limits as limits
        except ImportError:
            workers = 1
    if workers > 1:  # blocks are independent and write disjoint rows
        from concurrent.futures import ThreadPoolExecutor
        with limits(limits=1, user_api="blas"), ThreadPoolExecutor(workers) as ex:
            list(ex.map(lambda t: t[0](*t[1:]), tasks))
    else:
        for t in tasks:
            t[0](*t[1:])
    return res


def _slicer(p, arg_err, g):
    """p_fn of sampled_from_p for a given full P [B, Hq, Sq, Sk] (and argument bound)"""
    def p_fn(b, hk, rows, cols):
        cut = lambda x: x[b, hk * g:(hk + 1) * g][:, rows[:, None], cols[None, :]]
        return cut(p) if arg_err is None else (cut(p), cut(arg_err))
    return p_fn


def grads_from_p(p, q, k, v, o, do, *, sm_scale, dlse=None):
    """(dq, dk, dv) float64 for a given P [B, Hq, Sq, Sk]: sampled_from_p with every block"""
    r = sampled_from_p(_slicer(p, None, q.shape[1] // k.shape[1]), q, k, v, o, do, sm_scale=sm_scale, dlse=dlse)
    return r["dq"], r["dk"], r["dv"]


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
                library's exp2f, built on it, documents the same 1 ulp), so P_k = P 2^(+-arg_err) (1 +- 2^-23); an fp32
                subnormal result may be flushed (at most 2^-126).
      P, dS     rounded once each to the input dtype (pack_pair: store_cvt) - relative u = 2^-11 (fp16) / 2^-8 (bf16), and
                below the smallest normal half a step of the subnormal grid (2^-25 for fp16): neither the conversion nor the
                f16 / bf16 A / B inputs of v_mfma_f32_16x16x32_{f16,bf16} flush subnormals on gfx950, which
                test_gpu_backward_long.py::test_mfma_keeps_fp16_subnormals settles with P = 2^-15 .. 2^-17 exactly
                (_round_err).
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
    r = sampled_from_p(_slicer(p, arg_err, q.shape[1] // k.shape[1]), q, k, v, o, do, sm_scale=sm_scale, dtype=dtype, dlse=dlse,
                       return_bound=True)
    return r["bq"], r["bk"], r["bv"]


def attention_backward_sampled(q, k, v, o, lse, do, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False,
                               dlse=None, km=None, q_blocks=None, k_blocks=None, return_bound=False, workers=1):
    """sampled_from_p with the contract's P (prepare_p / p_panel): dq on the 64-row query blocks `q_blocks`, dk / dv on the 64-key
    blocks `k_blocks` (None: all), o and lse the operator's for ALL rows; memory O(S D) + O(64 S) per head."""
    c = prepare_p(q, k, lse, sm_scale=sm_scale, is_causal=is_causal, dtype=dtype, q_qmax=q_qmax, k_qmax=k_qmax, smooth_k=smooth_k, km=km)
    return sampled_from_p(lambda b, hk, rows, cols: p_panel(c, b, hk, rows, cols, return_bound), q, k, v, o, do, sm_scale=sm_scale,
                          dtype=dtype, dlse=dlse, q_blocks=q_blocks, k_blocks=k_blocks, return_bound=return_bound, workers=workers)


def attention_backward(q, k, v, o, lse, do, *, sm_scale, is_causal=False, dtype="fp16", q_qmax=0, k_qmax=0, smooth_k=False,
                       dlse=None, km=None, return_bound=False):
    """(dq, dk, dv) float64 of the contract: attention_backward_sampled with every block.  o and lse are the operator's.
    return_bound: (dq, dk, dv, bq, bk, bv), the b* the per-element bound of grad_bound (the largest deviation of a correct
    kernel from dq / dk / dv)."""
    r = attention_backward_sampled(q, k, v, o, lse, do, sm_scale=sm_scale, is_causal=is_causal, dtype=dtype, q_qmax=q_qmax,
                                   k_qmax=k_qmax, smooth_k=smooth_k, dlse=dlse, km=km, return_bound=return_bound)
    return tuple(r[x] for x in (("dq", "dk", "dv", "bq", "bk", "bv") if return_bound else ("dq", "dk", "dv")))
