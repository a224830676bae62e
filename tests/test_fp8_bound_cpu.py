"""The fp8-PV bound (`_fp8_flip_close` + the oracle's flip slack) is SOUND and SHARP - CPU only, no GPU.

A small restatement of the oracle's fp8 tile loop (`_model`) with switches for what a correct kernel may do differently
(sound: must pass against the plain oracle) and for plain bugs (sharp: each must be rejected on at least one case).  The
restatement without switches is checked bit for bit against `attn_fwd_int8_fp8` first, so the switches are the only change."""
import numpy as np
import pytest

from test_gpu_parity import _fp8_close, _fp8_flip_close

FP8_OFF = np.float32(8.807)
KMAGIC = np.float32(12582912.0)


def _inputs(orc, dist, B, H, Hkv, Sq, Sk, D, seed):
    q, k, v = orc.make_inputs(B, H, Sq, D, seed=seed, Hkv=Hkv, Sk=Sk, dist="randint" if dist == "randint" else "normal")
    if dist == "peaky":
        q = orc.to_storage(q * np.float32(6.0), "fp16")
    elif dist == "x1000":
        q, k = orc.to_storage(q * np.float32(1000.0), "fp16"), orc.to_storage(k * np.float32(1000.0), "fp16")
    return q, k, v


def _e4m3_nan_beyond(x):
    """e4m3fn conversion WITHOUT satfinite: |x| >= 464 (half-way to the next binade) gives the NaN code."""
    from oracle.lowbit_fa_oracle import e4m3fn_round
    return np.where(np.abs(x) >= 464.0, np.float32(np.nan), e4m3fn_round(x))


def _model(orc, mid, v8, v_scale, causal, var=None, seed=0):
    """attn_fwd_int8_fp8 restated, with `var` one of the variants / mutants below (None: bit-identical to the oracle)."""
    q_i8, k_i8, qsc, ksc = mid["q_i8"], mid["k_i8"], mid["q_scale"], mid["k_scale"]
    v8 = v8.copy()
    v_scale = v_scale.copy()
    if var == "drop_last_key":
        k_i8, v8 = k_i8[:, :, :-1], v8[:, :, :-1]
    if var == "zero_v_row":
        v8[:, :, min(3, v8.shape[2] - 1)] = 0
    if var == "v_scale_x1.01":
        v_scale = (v_scale * np.float32(1.01)).astype(np.float32)
    rng = np.random.default_rng(seed)
    B, Hq, Sq, D = q_i8.shape
    _, Hkv, Sk, _ = k_i8.shape
    g = Hq // Hkv
    nblk = qsc.shape[2]
    o = np.zeros((B, Hq, Sq, D), np.float32)
    rows = np.arange(Sq)
    row_blk = rows // 128
    if var == "q_scale_neighbour_block":
        row_blk = (row_blk + 1) % nblk
    with np.errstate(all="ignore"):
        for b in range(B):
            for h in range(Hq):
                hk = h % Hkv if var == "gqa_h_mod_hkv" else h // g
                qf, kf, vf = q_i8[b, h].astype(np.float32), k_i8[b, hk].astype(np.float32), v8[b, hk].astype(np.float32)
                qs = qsc[b, h][row_blk].astype(np.float32)
                m_i = np.full(Sq, -np.inf, np.float32)
                m_lo = np.zeros(Sq, np.float64)          # `huge`: the reference kept as the exact product m_i + m_lo
                l_i = np.zeros(Sq, np.float32)
                acc = np.zeros((Sq, D), np.float32)
                for j in range((Sk + 63) // 64):
                    n0, n1 = j * 64, min(j * 64 + 64, Sk)
                    r0 = (n0 // 128) * 128 if causal else 0
                    if r0 >= Sq:
                        break
                    s = (qf[r0:] @ kf[n0:n1].T).astype(np.float32)
                    ks = np.float32(ksc[b, hk, j])
                    if var == "score_order":        # s (qs ks) instead of (s qs) ks
                        qk = s * (qs[r0:, None] * ks)
                    else:
                        qk = s * qs[r0:, None] * ks
                    if var == "scores_x1.05":
                        qk = qk * np.float32(1.05)
                    if causal:
                        shift = 1 if var == "causal_off_by_one" else 0
                        cc = (n0 + np.arange(n1 - n0))[None, :]
                        qk = np.where(rows[r0:, None] + shift >= cc, qk, -np.inf)
                    m_ij = np.maximum(m_i[r0:], qk.max(axis=1))
                    if var == "huge_form":
                        # attn_fwd.hip `huge`: sc = fl(qs ks); the row reference as the exact product t sc = m_hi + m_lo; scores
                        # relative to the integer r nearest to it: arg = fl((s - r) sc + c1), c1 = fl(fl(fl(r sc - m_hi) - m_lo) + 8.807)
                        sc = (qs[r0:] * ks).astype(np.float32)
                        s64 = np.where(np.isfinite(qk), s.astype(np.float64), -np.inf)
                        t_prod = (s64 * sc[:, None].astype(np.float64)).max(axis=1)        # exact (int x fp32 fits in 53 bits)
                        up = t_prod.astype(np.float32) > m_i[r0:]
                        new_hi = np.where(up, t_prod.astype(np.float32), m_i[r0:])
                        new_lo = np.where(up, t_prod - t_prod.astype(np.float32).astype(np.float64), m_lo[r0:])
                        alpha = np.exp2(((m_i[r0:] - new_hi).astype(np.float64) + (m_lo[r0:] - new_lo)).astype(np.float32))
                        alpha = np.where(np.isfinite(m_i[r0:]), alpha, np.float32(0)).astype(np.float32)
                        r = np.clip(np.rint(new_hi / sc), -2.0 ** 22, 2.0 ** 22).astype(np.float32)
                        c1 = ((r.astype(np.float64) * sc - new_hi).astype(np.float32) - new_lo.astype(np.float32)).astype(np.float32) + FP8_OFF
                        arg = ((s64 - r[:, None]) * sc[:, None] + c1[:, None].astype(np.float64)).astype(np.float32)
                        m_lo[r0:] = new_lo
                        m_ij = new_hi
                    else:
                        alpha = np.exp2(m_i[r0:] - m_ij).astype(np.float32)
                        arg = (qk - m_ij[:, None] + FP8_OFF).astype(np.float32)
                    if var == "jitter_2ulp":
                        jit = rng.integers(-2, 3, arg.shape) * np.spacing(np.abs(arg))
                        arg = np.where(np.isfinite(arg), arg + jit, arg).astype(np.float32)
                    if var == "not_satfinite":
                        # the pre-round-4 bias folding: c1 = fl(fl(-kMagic sc - m) + 8.807), arg = fl(fma(kMagic + s, sc, c1))
                        sc = (qs[r0:] * ks).astype(np.float32)
                        c1 = ((-KMAGIC * sc - m_ij).astype(np.float32) + FP8_OFF).astype(np.float32)
                        sb = np.where(np.isfinite(qk), s.astype(np.float64) + float(KMAGIC), -np.inf)
                        arg = (sb * sc[:, None].astype(np.float64) + c1[:, None].astype(np.float64)).astype(np.float32)
                    p = np.exp2(arg).astype(np.float32)
                    if var == "l_order":          # row sum in reverse key order, one add at a time
                        ps = np.zeros(p.shape[0], np.float32)
                        for c in range(p.shape[1] - 1, -1, -1):
                            ps = (ps + p[:, c]).astype(np.float32)
                    else:
                        ps = p.sum(axis=1, dtype=np.float32)
                    l_i[r0:] = l_i[r0:] * alpha + ps
                    acc[r0:] *= alpha[:, None]
                    if var == "p_fp16":
                        pq = p.astype(np.float16).astype(np.float32)
                    elif var == "not_satfinite":
                        pq = _e4m3_nan_beyond(p)
                    else:
                        pq = orc.e4m3fn_round(p)
                    acc[r0:] += pq @ vf[n0:n1]
                    m_i[r0:] = m_ij
                o[b, h] = acc / l_i[:, None] * v_scale[b, hk][None, :]
    return orc.to_storage(o, "fp16")


# dist x shape: N(0,1), randint(-100, 100), peaky (q x 6), 1000 N(0,1); causal, ragged Sq != Sk with GQA, Sk = 1
DISTS = ["normal", "randint", "peaky", "x1000"]
SHAPES = [(1, 2, 2, 256, 256, 64, False), (1, 2, 2, 256, 256, 64, True), (1, 4, 2, 200, 333, 64, False), (1, 2, 2, 77, 1, 64, False)]
CASES = [(d,) + s for d in DISTS for s in SHAPES] + [("randint", 1, 2, 2, 512, 512, 128, False)]
SOUND = ["jitter_2ulp", "score_order", "l_order", "huge_form"]
MUTANTS = ["drop_last_key", "zero_v_row", "v_scale_x1.01", "scores_x1.05", "p_fp16", "not_satfinite", "causal_off_by_one",
           "gqa_h_mod_hkv", "q_scale_neighbour_block"]

_cache = {}


def _case(orc, c):
    if c not in _cache:
        dist, B, H, Hkv, Sq, Sk, D, causal = c
        q, k, v = _inputs(orc, dist, B, H, Hkv, Sq, Sk, D, seed=3)
        with np.errstate(all="ignore"):
            ref, slack, _, mid = orc.lowbit_fa_forward(q, k, v, is_causal=causal, smooth_k=dist != "x1000", pv="fp8", amax_floor=1e-7,
                                                    return_slack=True, return_intermediates=True)
        v8, v_scale = orc.per_channel_fp8(v)
        _cache[c] = (ref, slack, mid, v8, v_scale)
    return _cache[c]


def _flip_ok(o, ref, slack):
    try:
        _fp8_flip_close(o, ref, slack, "fp16")
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(map(str, c)))
def test_model_without_switches_is_the_oracle(oracle, c):
    ref, slack, mid, v8, v_scale = _case(oracle, c)
    o = _model(oracle, mid, v8, v_scale, c[-1])
    assert np.array_equal(o.view(np.uint32), ref.view(np.uint32))
    assert slack.shape == ref.shape and np.isfinite(slack).all() and (slack >= 0).all()


@pytest.mark.parametrize("var", SOUND)
@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(map(str, c)))
def test_bound_is_sound(oracle, c, var):
    """What a correct kernel may do differently passes against the plain oracle."""
    ref, slack, mid, v8, v_scale = _case(oracle, c)
    o = _model(oracle, mid, v8, v_scale, c[-1], var=var, seed=len(var))
    _fp8_flip_close(o, ref, slack, "fp16")


@pytest.mark.parametrize("var", MUTANTS)
def test_bound_is_sharp(oracle, var):
    """Each plain bug is rejected on at least one case."""
    rejected = []
    for c in CASES:
        if var == "drop_last_key" and c[5] == 1:
            continue
        ref, slack, mid, v8, v_scale = _case(oracle, c)
        o = _model(oracle, mid, v8, v_scale, c[-1], var=var)
        if not _flip_ok(o, ref, slack):
            rejected.append(c)
    assert rejected, f"{var} accepted on every case"


def test_slack_is_not_vacuous(oracle):
    """At 1000 N(0,1) (softmax references of ~1e6 binades) the slack exceeds the output-rounding allowance on at most 20 % of the
    elements - a bound proportional to |s| made every code there flippable - and V x 1.01 is rejected there."""
    for c in CASES:
        if c[0] == "x1000":
            ref, slack, mid, v8, v_scale = _case(oracle, c)
            wide = slack > 2.0 ** -9 * np.abs(ref) + 2.0 ** -12
            assert wide.mean() <= 0.2, (c, wide.mean())
    c = ("x1000",) + SHAPES[0]
    ref, slack, mid, v8, v_scale = _case(oracle, c)
    assert not _flip_ok(_model(oracle, mid, v8, v_scale, False, var="v_scale_x1.01"), ref, slack)


def test_old_checks_accept_these_mutants(oracle):
    """Why _fp8_flip_close exists: on B1 H2 S512 D64 N(0,1) the per-element bound of _fp8_close accepts V x 1.01, and the
    fp8 check of the fuzz (atol 0.2, rtol 6e-2, MSE 2e-5) accepts both the dropped last key and V x 1.01.  The new check
    rejects both."""
    q, k, v = _inputs(oracle, "normal", 1, 2, 2, 512, 512, 64, seed=3)
    ref, slack, _, mid = oracle.lowbit_fa_forward(q, k, v, pv="fp8", amax_floor=1e-7, return_slack=True, return_intermediates=True)
    v8, v_scale = oracle.per_channel_fp8(v)

    def fuzz_ok(o):
        return bool(np.all(np.abs(o - ref) <= 0.2 + 6e-2 * np.abs(ref))) and float(np.mean((o - ref) ** 2)) <= 2e-5

    o_drop = _model(oracle, mid, v8, v_scale, False, var="drop_last_key")
    o_vs = _model(oracle, mid, v8, v_scale, False, var="v_scale_x1.01")
    _fp8_close(o_vs, ref)
    assert fuzz_ok(o_drop) and fuzz_ok(o_vs)
    assert not _flip_ok(o_drop, ref, slack) and not _flip_ok(o_vs, ref, slack)


def test_bound_is_specific_to_the_key_tile_order(oracle):
    """P is rounded to e4m3 against the RUNNING row maximum, so walking the key tiles backwards (the HIP kernel does so for every
    other round of 64 Q blocks) rounds against other references: far more than boundary flips.  A comparison with a kernel's
    reversed rounds has to use the reversed restatement (`fp8_key_tiles_reversed`), which its own slack then covers."""
    q, k, v = _inputs(oracle, "normal", 1, 1, 1, 512, 512, 64, seed=1)
    fwd, slack = oracle.lowbit_fa_forward(q, k, v, pv="fp8", amax_floor=1e-7, return_slack=True)
    rev, slack_rev = oracle.lowbit_fa_forward(q, k, v, pv="fp8", amax_floor=1e-7, return_slack=True, fp8_key_tiles_reversed=True)
    assert not _flip_ok(rev, fwd, slack)
    _fp8_flip_close(rev, rev, slack_rev, "fp16")
