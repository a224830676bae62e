"""CPU float64 restatement of the packed-batch backward contract (include/lowbit_fa.h `lbfa_backward_varlen`): the dense
contract of bwd_reference.py applied sequence by sequence.

Sequence b owns query tokens [cu_q[b], cu_q[b+1]) and key tokens [cu_k[b], cu_k[b+1]); no gradient crosses a boundary.  The
forward's km (ONE mean over all packed keys), codes and scales come from `oracle.lowbit_fa_varlen(..., return_intermediates=True)`
(quantisation blocks restart at every sequence).  Per sequence:
    lse  = lse2 / log2(e) + dtype(q . km) * sm_scale   (lse2 of oracle.attn_fwd_int8_fp16; -inf for a sequence without keys)
    P    = exp2(s2 - (lse - dtype(q . km) * sm_scale) * log2(e)),  s2 = codes x scales
and the gradients of bwd_reference.grads_from_p.  Arrays are packed [total, H, D] (fp32 values already rounded to the storage
dtype); lse / dlse are [Hq, total_q].  Tokens in no sequence get zero gradients.
"""
from __future__ import annotations

import numpy as np

from bwd_reference import LOG2E, _slicer, fwd_corr, p_panel, quantised_context, sampled_from_p
from oracle import lowbit_fa_oracle as orc


def _seq(x, c, b):
    """[1, H, len, D] panel of sequence b of a packed [total, H, D] array"""
    return np.transpose(x[c[b]:c[b + 1]], (1, 0, 2))[None]


def packed_codes(q, k, cu_q, cu_k, *, dtype, sm_scale, smooth_k, q_qmax, k_qmax):
    """the `return_intermediates` dict of oracle.lowbit_fa_varlen (q_i8, k_i8, km, q_scale, k_scale) without its attention, which
    is quadratic in the sequence length: ONE mean over all packed keys, k - km in the storage dtype, then oracle.quant_per_block
    sequence by sequence with the 1e-7 floor (test_bwd_varlen_reference_cpu.py holds the two equal)"""
    q, k = orc._pad_head_dim(q), orc._pad_head_dim(k)
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    km = None
    if smooth_k:
        km = orc.to_storage(np.mean(k.astype(np.float64), axis=0, keepdims=True).astype(np.float32), dtype)
        k = orc.to_storage(k.astype(np.float32) - km.astype(np.float32), dtype)
    q_i8, k_i8, qsc, ksc = np.zeros(q.shape, np.int8), np.zeros(k.shape, np.int8), [], []
    for b in range(len(cq) - 1):
        if cq[b + 1] == cq[b]:
            continue
        qi, qs = orc.quant_per_block(_seq(q, cq, b), np.float32(float(sm_scale) * LOG2E), float(q_qmax), 128, 1e-7)
        q_i8[cq[b]:cq[b + 1]] = np.transpose(qi[0], (1, 0, 2))
        qsc.append(np.transpose(qs[0], (1, 0)))
        if ck[b + 1] == ck[b]:
            continue
        ki, ks = orc.quant_per_block(_seq(k, ck, b), 1.0, float(k_qmax), 64, 1e-7)
        k_i8[ck[b]:ck[b + 1]] = np.transpose(ki[0], (1, 0, 2))
        ksc.append(np.transpose(ks[0], (1, 0)))
    return dict(q_i8=q_i8, k_i8=k_i8, km=km, q_scale=np.concatenate(qsc, axis=0) if qsc else np.zeros((0, q.shape[1]), np.float32),
                k_scale=np.concatenate(ksc, axis=0) if ksc else np.zeros((0, k.shape[1]), np.float32))


def intermediates(q, k, v, cu_q, cu_k, *, dtype="fp16", is_causal=False, sm_scale=None, smooth_k=True, q_qmax=127, k_qmax=127):
    """per sequence (None for an empty query range): dict(qi, qs, ki, ks, corr) - the forward's codes [1, H, len, D], scales
    [1, H, blocks] and the storage-rounded q . km [1, Hq, len_q] (zeros without smooth-K) - and sm_scale"""
    D = q.shape[-1]
    sm_scale = 1.0 / D ** 0.5 if sm_scale is None else sm_scale
    it = packed_codes(q, k, cu_q, cu_k, dtype=dtype, sm_scale=sm_scale, smooth_k=smooth_k, q_qmax=q_qmax, k_qmax=k_qmax)
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    g = q.shape[1] // k.shape[1]
    seqs, qb0, kb0 = [], 0, 0
    for b in range(len(cq) - 1):
        lq, lk = cq[b + 1] - cq[b], ck[b + 1] - ck[b]
        if lq == 0:
            seqs.append(None)
            continue
        nq, nk = -(-lq // 128), (-(-lk // 64) if lk else 0)
        s = dict(qi=_seq(it["q_i8"], cq, b), ki=_seq(it["k_i8"], ck, b),
                 qs=np.transpose(it["q_scale"][qb0:qb0 + nq], (1, 0))[None],
                 ks=np.transpose(it["k_scale"][kb0:kb0 + nk], (1, 0))[None])
        qb0, kb0 = qb0 + nq, kb0 + nk
        qf = _seq(q, cq, b).astype(np.float32)
        if smooth_k:
            km = np.repeat(np.transpose(it["km"][..., :D], (1, 0, 2))[None], g, axis=1).astype(np.float32)  # [1, Hq, 1, D]
            s["corr"] = fwd_corr(qf, km, dtype)
        else:
            s["corr"] = np.zeros(qf.shape[:3])
        seqs.append(s)
    return seqs, sm_scale


def varlen_lse(q, k, v, cu_q, cu_k, return_corr=False, **kw):
    """natural-log LSE [Hq, total_q] float64 of the packed forward; rows in no sequence NaN, key-less sequences -inf.
    return_corr: also the correction term dtype(q . km) * sm_scale of every row (0 in rows of no sequence)"""
    seqs, sm_scale = intermediates(q, k, v, cu_q, cu_k, **kw)
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    out = np.full((q.shape[1], q.shape[0]), np.nan)
    corr = np.zeros(out.shape)
    for b, s in enumerate(seqs):
        if s is None:
            continue
        corr[:, cq[b]:cq[b + 1]] = s["corr"][0] * sm_scale
        if ck[b + 1] == ck[b]:
            out[:, cq[b]:cq[b + 1]] = -np.inf
            continue
        vb = _seq(orc._pad_head_dim(v), ck, b).astype(np.float16).astype(np.float32)  # the codes' padded head dim
        _, lse2 = orc.attn_fwd_int8_fp16(s["qi"], s["ki"], vb, s["qs"], s["ks"], causal=kw.get("is_causal", False),
                                         return_lse=True, tail="neg_inf")
        out[:, cq[b]:cq[b + 1]] = (lse2[0].astype(np.float64) / LOG2E + s["corr"][0] * sm_scale)
    return (out, corr) if return_corr else out


def _context(s, lse, sm_scale, is_causal):
    """bwd_reference's P context of one sequence from its codes, scales and the operator's LSE rows [Hq, len_q]"""
    return quantised_context(s["qi"], s["qs"], s["ki"], s["ks"], s["corr"], lse[None], sm_scale, is_causal)


def p_quantised(s, lse, sm_scale, is_causal, return_arg_err=False):
    """P [1, Hq, len_q, len_k] of one sequence from its codes, scales and the operator's LSE rows [Hq, len_q]
    (return_arg_err: and the bound on the kernel's exponent-argument error, bwd_reference.quantised_arg_err)"""
    c = _context(s, lse, sm_scale, is_causal)
    g, Hkv = c["g"], s["ki"].shape[1]
    rows, cols = np.arange(c["Sq"]), np.arange(c["Sk"])
    r = [p_panel(c, 0, hk, rows, cols, return_arg_err) for hk in range(Hkv)]
    if not return_arg_err:
        return np.concatenate(r, axis=0)[None]
    return np.concatenate([x[0] for x in r], axis=0)[None], np.concatenate([x[1] for x in r], axis=0)[None]


def varlen_backward(q, k, v, o, lse, do, cu_q, cu_k, *, dtype="fp16", is_causal=False, sm_scale=None, smooth_k=True,
                    q_qmax=127, k_qmax=127, dlse=None, p_fn=None, only=None, return_bound=False, blocks=None, workers=1):
    """(dq, dk, dv) float64, packed like q / k / v.  `p_fn(b, q_b, k_b, lse_b, sm_scale)` replaces the quantised P of sequence b
    (q_b / k_b [1, H, len, D]); `only`: the sequences to compute (others stay zero).
    return_bound: (dq, dk, dv, bq, bk, bv) with the per-element bound of bwd_reference.grad_bound, sequence by sequence
    (0 where the kernel writes exact zeros: tokens in no sequence, sequences without queries or keys); not with p_fn.
    `blocks`: {sequence: (query blocks, key blocks)} - those sequences are computed on these 64-row blocks only
    (bwd_reference.sampled_from_p; None in the pair: all blocks), and two boolean token masks are appended to the result: the
    query tokens and the key tokens that were computed (every token of a sequence not named in `blocks`)."""
    if return_bound and p_fn is not None:
        raise ValueError("return_bound needs the quantised P (p_fn given)")
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    if p_fn is None:
        seqs, sm_scale = intermediates(q, k, v, cu_q, cu_k, dtype=dtype, is_causal=is_causal, sm_scale=sm_scale,
                                       smooth_k=smooth_k, q_qmax=q_qmax, k_qmax=k_qmax)
    else:
        seqs, sm_scale = None, (1.0 / q.shape[-1] ** 0.5 if sm_scale is None else sm_scale)
    dq, dk, dv = (np.zeros(x.shape) for x in (q, k, v))
    bq, bk, bv = (np.zeros(x.shape) for x in (q, k, v))
    mq, mk = np.ones(q.shape[0], bool), np.ones(k.shape[0], bool)
    g = q.shape[1] // k.shape[1]
    for b in range(len(cq) - 1):
        if (only is not None and b not in only) or cq[b + 1] == cq[b] or ck[b + 1] == ck[b]:
            continue  # no queries or no keys: every gradient of the sequence is zero
        qb, kb, vb, ob, dob = (_seq(x, c, b) for x, c in ((q, cq), (k, ck), (v, ck), (o, cq), (do, cq)))
        lb = lse[:, cq[b]:cq[b + 1]]
        dlb = None if dlse is None else dlse[:, cq[b]:cq[b + 1]][None]
        if p_fn is None:
            c = _context(seqs[b], lb, sm_scale, is_causal)
            fn = lambda _, hk, rows, cols: p_panel(c, 0, hk, rows, cols, return_bound)
        else:
            fn = _slicer(p_fn(b, qb, kb, lb, sm_scale), None, g)
        qbl, kbl = (blocks or {}).get(b, (None, None))
        r = sampled_from_p(fn, qb, kb, vb, ob, dob, sm_scale=sm_scale, dtype=dtype, dlse=dlb, q_blocks=qbl, k_blocks=kbl,
                           return_bound=return_bound, workers=workers)
        for c0, m, bl, rows in ((cq[b], mq, qbl, r["rows_q"]), (ck[b], mk, kbl, r["rows_k"])):
            if bl is not None:
                m[c0:c0 + (cq[b + 1] - cq[b] if m is mq else ck[b + 1] - ck[b])] = False
                m[c0 + rows] = True
        for outs, names, c0, rows in (((dq, bq), ("dq", "bq"), cq[b], r["rows_q"]), ((dk, bk), ("dk", "bk"), ck[b], r["rows_k"]),
                                      ((dv, bv), ("dv", "bv"), ck[b], r["rows_k"])):
            for out, name in zip(outs, names):
                if name in r:
                    out[c0 + rows] = np.transpose(r[name][0], (1, 0, 2))
    res = (dq, dk, dv, bq, bk, bv) if return_bound else (dq, dk, dv)
    return res if blocks is None else res + (mq, mk)
