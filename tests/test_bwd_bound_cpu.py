"""The per-element backward bound (`bwd_reference.grad_bound`, attention_backward(..., return_bound=True)) is SOUND and SHARP -
CPU only, no GPU.

`_kernel` restates the arithmetic of the two gradient kernels of attn_bwd.hip in numpy: fp32 throughout (np.float32), the pre-pass
(delta as an fma chain over d ascending, then - dLSE; lse2 = fl(fl(lse - fl(corr fl(sm_scale))) fl(log2e))), the argument
fl(fl(a sc) - lse2) with sc = fl(q_scale k_scale) (or fl(sm_scale log2e) un-quantised, a an fp32 dot product), P = fl(exp2),
P and dS rounded to the dtype (orc.to_storage) before fp32 products summed over 64-row (dk / dv) or 64-key (dq) tiles,
dq / dk times fl(sm_scale), stores in the dtype.  Switches give what a correct kernel may do differently (sound: every one
must pass the bound against the float64 reference) and plain bugs (sharp: each must be rejected on at least one case).
For every bug the old per-tensor check (test_gpu_backward._assert_close) is run as well and its verdict printed:
`BWDMUTANT <name> new: rejected on i/n cases, old: accepted on j/n`.
The block-sampled form of the reference (attention_backward_sampled, what the long-sequence GPU tests use) gives the full
form's gradients and bounds bit for bit on the sampled rows, and still rejects every listed bug on a sampling that holds the
block the bug touches."""
import numpy as np
import pytest

from bwd_reference import LOG2E, attention_backward, attention_backward_sampled, fwd_corr
from oracle import lowbit_fa_oracle as orc

F32 = np.float32
VARIANTS = [None, "tiles_reversed", "pairwise", "sc_unrounded", "exp2_ulp"]
MUTANTS = ["drop_last_key", "drop_last_row", "causal_lt", "q_scale_neighbour", "k_scale_off_by_one", "dlse_dropped",
           "dlse_sign", "corr_kept", "gqa_head_missing", "dk_no_sm_scale", "delta_d_minus_8", "p_tile_x_1+2^-7"]


def _inputs(dist, dtype, B, Hq, Hkv, Sq, Sk, D, seed, k_bias=0.0):
    q, k, v = orc.make_inputs(B, Hq, Sq, D, seed=seed, dtype=dtype, Hkv=Hkv, Sk=Sk, k_bias=k_bias,
                              dist="randint" if dist == "randint" else "normal")
    if dist == "peaky":
        q = orc.to_storage(q * F32(6.0), dtype)
    elif dist == "x100":
        q, k, v = (orc.to_storage(x * F32(100.0), dtype) for x in (q, k, v))
    return q, k, v


def _mask(Sq, Sk, causal):
    return np.arange(Sk)[None, :] <= np.arange(Sq)[:, None] if causal else np.ones((Sq, Sk), bool)


def _quant(q, k, c):
    """codes, scales (oracle) and the correction dtype(q . km) [B, Hq, Sq] in the kernels' order (fwd_corr): bit-exact to the kernels"""
    g = q.shape[1] // k.shape[1]
    kmq = orc.mean_seq(k, c["dtype"]) if c["smooth"] else None
    q8, qs, k8, ks = orc.per_block_int8(q, k, kmq, c["sm"], c["dtype"], q_qmax=float(c["qmax"]), k_qmax=float(c["kmax"]),
                                        amax_floor=1e-7)
    if c["smooth"]:
        corr = fwd_corr(q, np.repeat(kmq, g, axis=1), c["dtype"])
    else:
        corr = np.zeros(q.shape[:3], F32)
    return q8.astype(F32), qs, k8.astype(F32), ks, corr.astype(F32)


def _forward(q, k, v, c):
    """the operator's O (rounded to the dtype) and natural-log LSE (fp32), exact softmax of the forward's scores"""
    g = q.shape[1] // k.shape[1]
    if c["qmax"]:
        q8, qs, k8, ks, corr = _quant(q, k, c)
        Sq, Sk = q.shape[2], k.shape[2]
        s2 = (np.einsum("bhsd,bhtd->bhst", q8.astype(np.float64), np.repeat(k8, g, axis=1).astype(np.float64))
              * np.repeat(qs, 128, axis=2)[:, :, :Sq, None] * np.repeat(np.repeat(ks, 64, axis=2)[:, :, :Sk], g, axis=1)[:, :, None, :])
    else:
        corr = np.zeros(q.shape[:3], F32)
        s2 = np.einsum("bhsd,bhtd->bhst", q.astype(np.float64), np.repeat(k, g, axis=1).astype(np.float64)) * c["sm"] * LOG2E
    s2 = np.where(_mask(q.shape[2], k.shape[2], c["causal"]), s2, -np.inf)
    m = s2.max(-1, keepdims=True)
    p = np.exp2(s2 - m)
    lse2 = m[..., 0] + np.log2(p.sum(-1))
    o = np.einsum("bhst,bhtd->bhsd", p / p.sum(-1, keepdims=True), np.repeat(v, g, axis=1).astype(np.float64))
    lse = lse2 / LOG2E + corr.astype(np.float64) * c["sm"]
    return orc.to_storage(o.astype(F32), c["dtype"]), lse.astype(F32)


def _fma_chain(a, b, acc):
    """acc = fma(a_d, b_d, acc) for d ascending, fp32 (the 16-bit products and one fp32 add are exact in float64)"""
    for d in range(a.shape[-1]):
        acc = (a[..., d].astype(np.float64) * b[..., d].astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return acc


def _kernel(q, k, v, o, lse, do, dlse, c, var=None, seed=0):
    """(dq, dk, dv) of attn_bwd.hip restated; `var` one of VARIANTS / MUTANTS"""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = Hq // Hkv
    dt, sm32 = c["dtype"], F32(c["sm"])
    rnd = lambda x: orc.to_storage(np.asarray(x, F32), dt)
    rng = np.random.default_rng(seed)
    # pre-pass: delta and lse2 per query row
    Dd = D - 8 if var == "delta_d_minus_8" else D
    delta = _fma_chain(do[..., :Dd], o[..., :Dd], np.zeros((B, Hq, Sq), F32))
    if var == "pairwise":
        delta = (do * o).astype(F32).sum(-1, dtype=F32)
    if dlse is not None and var != "dlse_dropped":
        delta = (delta + dlse if var == "dlse_sign" else delta - dlse).astype(F32)
    if c["qmax"]:
        q8, qs, k8, ks, corr = _quant(q, k, c)
    l = lse.astype(F32)
    if c["qmax"] and c["smooth"] and var != "corr_kept":
        l = (l - (corr * sm32).astype(F32)).astype(F32)
    lse2 = (l * F32(LOG2E)).astype(F32)
    mask = _mask(Sq, Sk, c["causal"]) & (np.arange(Sk)[None, :] < Sk - (var == "drop_last_key")) \
        & (np.arange(Sq)[:, None] < Sq - (var == "drop_last_row"))
    if var == "causal_lt":
        mask = mask & (np.arange(Sk)[None, :] < np.arange(Sq)[:, None])
    dq = np.zeros((B, Hq, Sq, D), F32)
    dk, dv = np.zeros((B, Hkv, Sk, D), F32), np.zeros((B, Hkv, Sk, D), F32)
    qtiles, ktiles = list(range(0, Sq, 64)), list(range(0, Sk, 64))
    if var == "tiles_reversed":
        qtiles, ktiles = qtiles[::-1], ktiles[::-1]
    for b in range(B):
        for h in range(Hq):
            hk = h // g
            if c["qmax"]:
                a = q8[b, h] @ k8[b, hk].T  # integer dot products: exact in fp32
                qblk = np.arange(Sq) // 128
                kblk = np.arange(Sk) // 64
                if var == "k_scale_off_by_one":
                    kblk = np.minimum(kblk + 1, ks.shape[2] - 1)
                qsr = qs[b, h][qblk].astype(F32)
                if var == "q_scale_neighbour":  # rows 64..127 (a 64-row tile) take the next 128-row block's scale
                    qsr[64:128] = qs[b, h][min(1, qs.shape[2] - 1)]
                ksr = ks[b, hk][kblk].astype(F32)
                if var == "sc_unrounded":
                    sc = qsr[:, None].astype(np.float64) * ksr[None, :].astype(np.float64)
                else:
                    sc = (qsr[:, None] * ksr[None, :]).astype(F32)
            else:
                a = (q[b, h] @ k[b, hk].T).astype(F32)
                sc = F32(c["sm"] * 1.44269504)
                if var == "pairwise":
                    a = (q[b, h][:, None, :] * k[b, hk][None, :, :]).astype(F32).sum(-1, dtype=F32)
            x = ((a * sc).astype(F32) - lse2[b, h][:, None]).astype(F32)
            with np.errstate(over="ignore"):
                p = np.exp2(x.astype(np.float64)).astype(F32)
            if var == "exp2_ulp":  # one ulp up or down at random
                p = np.where(rng.integers(0, 2, p.shape) == 1, np.nextafter(p, F32(np.inf)), np.nextafter(p, F32(0)))
            p = np.where(mask, p, F32(0))
            if var == "p_tile_x_1+2^-7":
                p[:64] = (p[:64] * F32(1 + 2.0 ** -7)).astype(F32)
            if var == "pairwise":
                dp = (do[b, h][:, None, :] * v[b, hk][None, :, :]).astype(F32).sum(-1, dtype=F32)
            else:
                dp = (do[b, h] @ v[b, hk].T).astype(F32)
            ds = (p * (dp - delta[b, h][:, None]).astype(F32)).astype(F32)
            pr, dsr = rnd(p), rnd(ds)
            for k0 in ktiles:
                dq[b, h] = (dq[b, h] + (dsr[:, k0:k0 + 64] @ k[b, hk][k0:k0 + 64]).astype(F32)).astype(F32)
            if var == "gqa_head_missing" and g > 1 and h % g == g - 1:
                continue
            for q0 in qtiles:
                dv[b, hk] = (dv[b, hk] + (pr[q0:q0 + 64].T @ do[b, h][q0:q0 + 64]).astype(F32)).astype(F32)
                dk[b, hk] = (dk[b, hk] + (dsr[q0:q0 + 64].T @ q[b, h][q0:q0 + 64]).astype(F32)).astype(F32)
    dq = rnd(dq * sm32)
    dk = rnd(dk if var == "dk_no_sm_scale" else dk * sm32)
    return dq, dk, rnd(dv)


def _case(c):
    """inputs, the operator's O / LSE, upstream gradients, the reference and its bound"""
    q, k, v = _inputs(c["dist"], c["dtype"], c["B"], c["Hq"], c["Hkv"], c["Sq"], c["Sk"], c["D"], c["seed"], c.get("k_bias", 0.0))
    c = dict(c, sm=c.get("sm") or c["D"] ** -0.5)
    o, lse = _forward(q, k, v, c)
    rng = np.random.default_rng(c["seed"] + 7)
    do = orc.to_storage(rng.standard_normal(o.shape).astype(F32), c["dtype"])
    dlse = rng.standard_normal(lse.shape).astype(F32) if c["dlse"] else None
    ref = attention_backward(q, k, v, o, lse, do, sm_scale=c["sm"], is_causal=c["causal"], dtype=c["dtype"], q_qmax=c["qmax"],
                             k_qmax=c["kmax"], smooth_k=c["smooth"] and c["qmax"] != 0, dlse=dlse, return_bound=True)
    return c, (q, k, v, o, lse, do, dlse), ref


def _worst(got, ref):
    """max over the three gradients of |got - ref| / bound (inf where a gradient is non-finite)"""
    w = 0.0
    for x, r, bnd in zip(got, ref[:3], ref[3:]):
        if not np.all(np.isfinite(x)):
            return np.inf
        d = np.abs(x.astype(np.float64) - r)
        w = max(w, float(np.max(np.where(d > 0, d / np.maximum(bnd, 1e-300), 0.0))))
    return w


def _cfg(dtype, causal, Hq, Hkv, Sq, Sk, D, qmax, kmax, smooth, dlse, dist, k_bias=0.0, seed=0, sm=None):
    return dict(dtype=dtype, causal=causal, B=1, Hq=Hq, Hkv=Hkv, Sq=Sq, Sk=Sk, D=D, qmax=qmax, kmax=kmax, smooth=smooth, dlse=dlse,
                dist=dist, k_bias=k_bias, seed=seed, sm=sm)


SOUND = [
    _cfg("fp16", False, 2, 2, 200, 150, 64, 127, 127, True, False, "normal", 0.0, 1),
    _cfg("fp16", True, 4, 2, 192, 192, 64, 127, 127, True, True, "normal", 0.5, 2),
    _cfg("bf16", False, 2, 1, 130, 200, 128, 127, 127, True, True, "normal", 0.5, 3),
    _cfg("bf16", True, 2, 2, 200, 200, 128, 127, 127, False, False, "randint", 0.0, 4),
    _cfg("fp16", False, 2, 2, 150, 129, 128, 127, 127, False, True, "randint", 0.0, 5),
    _cfg("fp16", True, 2, 1, 150, 150, 64, 7, 7, True, False, "peaky", 0.5, 6),
    _cfg("bf16", False, 2, 2, 129, 100, 64, 127, 7, True, True, "peaky", 0.0, 7),
    _cfg("fp16", False, 2, 2, 100, 140, 64, 127, 127, True, False, "x100", 0.0, 8),
    _cfg("fp16", True, 4, 2, 140, 140, 64, 0, 0, False, True, "normal", 0.5, 9),
    _cfg("bf16", False, 2, 2, 129, 70, 128, 0, 0, False, False, "randint", 0.0, 10, 0.05),
    _cfg("fp16", False, 2, 1, 100, 100, 128, 0, 0, False, True, "x100", 0.0, 11),
    _cfg("bf16", True, 2, 2, 140, 140, 64, 0, 0, False, False, "peaky", 0.0, 12),
]


@pytest.mark.parametrize("ci", range(len(SOUND)))
def test_bound_is_sound(ci):
    """the restatement and every variant a correct kernel may be stay within the bound, and the restatement comes within a
    factor 32 of it somewhere (the bound is not vacuous: its worst element is set by the roundings to the dtype)"""
    c, (q, k, v, o, lse, do, dlse), ref = _case(SOUND[ci])
    worst = {}
    for var in VARIANTS:
        got = _kernel(q, k, v, o, lse, do, dlse, c, var=var, seed=ci)
        worst[var] = _worst(got, ref)
        assert worst[var] <= 1.0, (SOUND[ci], var, worst[var])
    assert worst[None] >= 1.0 / 32, (SOUND[ci], worst[None])
    print(f"BWDBOUND sound case {ci} {c['dtype']} {c['dist']} qmax={c['qmax']}: " +
          " ".join(f"{v}={w:.3f}" for v, w in worst.items()))


# each mutant against the cases that can show it (all run: the bound must reject it on at least one)
SHARP = [
    _cfg("fp16", True, 4, 2, 200, 200, 64, 127, 127, True, True, "normal", 0.5, 21),
    _cfg("bf16", True, 4, 2, 200, 200, 128, 127, 127, True, True, "normal", 0.5, 22),
    _cfg("fp16", False, 2, 2, 192, 150, 64, 127, 127, True, True, "peaky", 0.5, 23),
    _cfg("bf16", False, 4, 2, 200, 140, 128, 127, 127, True, True, "normal", 0.5, 24),
]


@pytest.fixture(scope="module")
def sharp_cases():
    return [_case(c) for c in SHARP]


def _old_accepts(got, ref, dtype):
    from test_gpu_backward import _assert_close
    try:
        for what, x, r in zip(("dq", "dk", "dv"), got, ref[:3]):
            _assert_close(x, r, dtype, what)
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_is_sharp(sharp_cases, mutant):
    rejected, old = [], []
    for c, (q, k, v, o, lse, do, dlse), ref in sharp_cases:
        got = _kernel(q, k, v, o, lse, do, dlse, c, var=mutant)
        rejected.append(_worst(got, ref) > 1.0)
        old.append(_old_accepts(got, ref, c["dtype"]))
    print(f"BWDMUTANT {mutant} new: rejected on {sum(rejected)}/{len(rejected)} cases, old: accepted on {sum(old)}/{len(old)} "
          "(per case new/old, R rejected, a accepted: " +
          ", ".join(f"{'R' if r else 'a'}/{'a' if a else 'R'}" for r, a in zip(rejected, old)) + ")")
    assert any(rejected), f"{mutant}: no case rejects it"


# ---- the block-sampled form ----
def _sampled(c, data, q_blocks, k_blocks):
    q, k, v, o, lse, do, dlse = data
    return attention_backward_sampled(q, k, v, o, lse, do, sm_scale=c["sm"], is_causal=c["causal"], dtype=c["dtype"], q_qmax=c["qmax"],
                                      k_qmax=c["kmax"], smooth_k=c["smooth"] and c["qmax"] != 0, dlse=dlse, q_blocks=q_blocks,
                                      k_blocks=k_blocks, return_bound=True)


def _sampling(c):
    """query blocks 0, 1 (rows 64..127: the second half of the first quantiser block) and the last; key blocks 0 and the last"""
    nq, nk = -(-c["Sq"] // 64), -(-c["Sk"] // 64)
    return sorted({0, min(1, nq - 1), nq - 1}), sorted({0, nk - 1})


@pytest.mark.parametrize("ci", range(len(SOUND)))
def test_sampled_equals_full_on_the_sampled_rows(ci):
    """EQUAL, not close: the full form is the sampled form with every block, one 64-row block at a time, so a block sees the
    same float64 operations on the same shapes whichever other blocks are asked for."""
    c, data, ref = _case(SOUND[ci])
    nq, nk = -(-c["Sq"] // 64), -(-c["Sk"] // 64)
    qb, kb = [nq - 1], ([0, nk - 1] if nk > 2 else [nk - 1])  # the ragged last blocks among them
    r = _sampled(c, data, qb, kb)
    assert len(r["rows_q"]) < c["Sq"] and len(r["rows_k"]) < c["Sk"] and r["rows_q"][-1] == c["Sq"] - 1 and r["rows_k"][-1] == c["Sk"] - 1
    for i, (name, rows) in enumerate((("dq", "rows_q"), ("dk", "rows_k"), ("dv", "rows_k"))):
        assert np.array_equal(r[name], ref[i][:, :, r[rows]]), name
        assert np.array_equal(r["b" + name[1]], ref[3 + i][:, :, r[rows]]), "bound of " + name
    assert _sampled(c, data, [], kb)["dq"].shape[2] == 0 and np.array_equal(_sampled(c, data, [], kb)["dk"], r["dk"])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_sampled_bound_is_sharp(sharp_cases, mutant):
    """every listed bug is still rejected when only the sampled blocks are compared (each bug touches query block 0, 1 or the
    last, or key block 0 or the last, or every block)"""
    rejected = []
    for c, data, _ in sharp_cases:
        qb, kb = _sampling(c)
        r = _sampled(c, data, qb, kb)
        got = _kernel(*data, c, var=mutant)
        cut = (got[0][:, :, r["rows_q"]], got[1][:, :, r["rows_k"]], got[2][:, :, r["rows_k"]])
        rejected.append(_worst(cut, (r["dq"], r["dk"], r["dv"], r["bq"], r["bk"], r["bv"])) > 1.0)
    print(f"BWDMUTANT {mutant} sampled: rejected on {sum(rejected)}/{len(rejected)} cases")
    assert any(rejected), f"{mutant}: no case rejects it on the sampled blocks"
