"""Numpy restatement of cached prefill (`lbfa_prefill`) and the cases its tests share (test infrastructure, in the style of
tests/kvcache_reference.py, which it builds on).

* `quant_q_blocks`: the in-kernel Q quantiser - blocks of 128 rows from row 0 of each (batch, head), the last block cut at
  q_lens[b]: `oracle.quant_per_block` on each sequence's valid rows.
* `oracle_prefill`: the REFERENCE of every value test: `oracle.attn_fwd_int8_fp16(..., tail="neg_inf")` on the numpy `CacheRef`
  state (never on the GPU's codes), one sequence at a time on its own length and its own valid query rows; causal (bottom-right
  aligned) = the non-causal oracle kernel, per query row i, on its first n - q_len + 1 + i keys with the scale of the row's block.
* `split_kv_prefill`: what the kernel computes - per 128-row Q block the tiles it can see, cut into key slices, an online softmax
  over 64-key tiles per slice, then the decode call's fixed-order combine (`split_kv_decode` generalised).
* `CASES`: the value cases of tests/test_gpu_prefill.py; tests/test_prefill_reference_cpu.py shows on every one of them that the
  numpy model stays inside the bounds (`o_bound`, `lse_bound` of kvcache_reference, unchanged, on every element).
* `oracle_state`: the state `oracle_prefill` reads - of a `CacheRef` its own, of a `v8_reference.CacheRefV8` the K state with
  V^ = `vhat()` as V, which is what a reader of the fp8 V cache sees.
* the census helpers of the prefill fuzz (tests/prefill_fuzz_cases.py): what a drawn case exercises, in the kernel's own terms
  (Q blocks, visible tiles, tiles per slice, tiles per page).
"""
import types

import numpy as np

import kvcache_reference as kr

BLKQ, BLKK = 128, 64
B, HQ, HKV = 2, 4, 2  # the common shape of the cases: what a case that names no B / HQ / HKV of its own gets


def shape_of(c):
    """(B, Hq, Hkv) of a value case"""
    return c.get("B", B), c.get("HQ", HQ), c.get("HKV", HKV)


def oracle_state(ref):
    """what `oracle_prefill` reads of a numpy cache: with an fp8 V cache (`CacheRefV8`) V is V^, the V a reader sees"""
    if not hasattr(ref, "vhat"):
        return ref
    return types.SimpleNamespace(k_codes=ref.k_codes, k_scale=ref.k_scale, v=ref.vhat(), seqlens=ref.seqlens)


def quant_q_blocks(orc, q, q_lens, sm_scale, qmax):
    """q [B,Hq,Sq,D] fp32-valued -> codes int8 [B,Hq,Sq,D] (zeros at and past q_lens[b]), scales fp32 [B,Hq,ceil(Sq/128)]
    (zero for a block with no valid row)"""
    nb, hq, sq, d = q.shape
    codes = np.zeros((nb, hq, sq, d), np.int8)
    scale = np.zeros((nb, hq, (sq + BLKQ - 1) // BLKQ), np.float32)
    for b in range(nb):
        ql = int(q_lens[b])
        if ql == 0:
            continue
        c, s = orc.quant_per_block(q[b:b + 1, :, :ql], np.float32(float(sm_scale) * kr.LOG2E), float(qmax), BLKQ, 1e-7)
        codes[b, :, :ql] = c[0]
        scale[b, :, :s.shape[2]] = s[0]
    return codes, scale


def oracle_prefill(orc, q_i8, q_scale, ref, q_lens, *, causal, out_dtype):
    """-> o [B,Hq,Sq,D] fp32 (rounded to out_dtype), lse2 [B,Hq,Sq] base 2; rows at or past q_lens[b] and rows that see no key are
    zeros and -inf.  `ref` is the CacheRef whose state the cache under test must hold."""
    nb, hq, sq, d = q_i8.shape
    o = np.zeros((nb, hq, sq, d), np.float32)
    lse2 = np.full((nb, hq, sq), -np.inf, np.float32)
    ref = oracle_state(ref)
    k_i8, k_scale, v16 = ref.k_codes, ref.k_scale, ref.v

    def run(b, rows, qs, n):
        ob, lb = orc.attn_fwd_int8_fp16(q_i8[b:b + 1, :, rows], k_i8[b:b + 1, :, :n], v16[b:b + 1, :, :n], qs,
                                        k_scale[b:b + 1, :, :(n + BLKK - 1) // BLKK], causal=False, out_dtype=out_dtype,
                                        return_lse=True, tail="neg_inf")
        o[b, :, rows] = ob[0]
        lse2[b, :, rows] = lb[0]

    for b in range(nb):
        n, ql = int(ref.seqlens[b]), int(q_lens[b])
        if ql == 0 or n == 0:
            continue
        if not causal:
            run(b, slice(0, ql), q_scale[b:b + 1, :, :(ql + BLKQ - 1) // BLKQ], n)
            continue
        for i in range(ql):
            ni = n - ql + 1 + i
            if ni > 0:
                run(b, slice(i, i + 1), q_scale[b:b + 1, :, i // BLKQ:i // BLKQ + 1], ni)
    return o, lse2


def oracle_prefill_rows(orc, q_i8, q_scale, ref, b, rows, *, q_len, causal, out_dtype):
    """`oracle_prefill` on the sampled query rows `rows` of sequence b alone (a long context, where every row would take minutes):
    the same per-row call on the row's visible keys with the scale of its block -> o [Hq, len(rows), D], lse2 [Hq, len(rows)]"""
    ref = oracle_state(ref)
    n = int(ref.seqlens[b])
    o = np.zeros((q_i8.shape[1], len(rows), q_i8.shape[3]), np.float32)
    lse2 = np.full((q_i8.shape[1], len(rows)), -np.inf, np.float32)
    for j, i in enumerate(rows):
        ni = (n - q_len + 1 + i) if causal else n
        if i >= q_len or ni <= 0:
            continue
        ob, lb = orc.attn_fwd_int8_fp16(q_i8[b:b + 1, :, i:i + 1], ref.k_codes[b:b + 1, :, :ni], ref.v[b:b + 1, :, :ni],
                                        q_scale[b:b + 1, :, i // BLKQ:i // BLKQ + 1], ref.k_scale[b:b + 1, :, :(ni + BLKK - 1) // BLKK],
                                        causal=False, out_dtype=out_dtype, return_lse=True, tail="neg_inf")
        o[:, j], lse2[:, j] = ob[0, :, 0], lb[0, :, 0]
    return o, lse2


def split_kv_prefill(orc, q_i8, q_scale, k_i8, k_scale, v16, seqlens, q_lens, *, causal, num_splits, out_dtype):
    """The prefill kernel in numpy: o [B,Hq,Sq,D] rounded to out_dtype, lse2 [B,Hq,Sq] base 2."""
    nb, hq, sq, d = q_i8.shape
    g = hq // k_i8.shape[1]
    o = np.zeros((nb, hq, sq, d), np.float32)
    lse2 = np.full((nb, hq, sq), -np.inf, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(nb):
            n, ql = int(seqlens[b]), int(q_lens[b])
            for qb in range((sq + BLKQ - 1) // BLKQ):
                r0, r1 = qb * BLKQ, min(qb * BLKQ + BLKQ, ql)
                if r1 <= r0:
                    continue  # no valid row: zeros, -inf
                rows = np.arange(r0, r1)
                lim = (n - ql + 1 + rows) if causal else np.full(len(rows), n)
                see = max(int(lim[-1]), 0)
                ntiles = (see + BLKK - 1) // BLKK
                tps = (ntiles + num_splits - 1) // num_splits
                for h in range(hq):
                    hk = h // g
                    qf = q_i8[b, h, r0:r1].astype(np.float32)
                    parts = []
                    for s in range(num_splits):
                        m = np.full(len(rows), -np.inf, np.float32)
                        l = np.zeros(len(rows), np.float32)
                        acc = np.zeros((len(rows), d), np.float32)
                        for t in range(s * tps, min((s + 1) * tps, ntiles)):
                            keys = np.arange(t * BLKK, (t + 1) * BLKK)
                            qk = (qf @ k_i8[b, hk, keys].astype(np.float32).T).astype(np.float32)
                            qk = qk * q_scale[b, h, qb] * k_scale[b, hk, t]
                            qk = np.where(keys[None, :] < lim[:, None], qk, np.float32(-np.inf))
                            m_new = np.maximum(m, qk.max(axis=1))
                            m_use = np.where(np.isinf(m_new), np.float32(0), m_new)
                            alpha = np.exp2(m - m_use).astype(np.float32)
                            p = np.exp2(qk - m_use[:, None]).astype(np.float32)
                            l = l * alpha + p.sum(axis=1, dtype=np.float32)
                            vt = np.where((keys < n)[:, None], v16[b, hk, keys], np.float32(0))
                            acc = acc * alpha[:, None] + p.astype(np.float16).astype(np.float32) @ vt.astype(np.float32)
                            m = m_new
                        parts.append((m, l, acc))
                    if num_splits == 1:
                        m, l, acc = parts[0]
                    else:  # the decode call's combine: 256 / D groups add contiguous runs of slices in order, then the groups
                        m = np.full(len(rows), -np.inf, np.float32)
                        for ms, _, _ in parts:
                            m = np.maximum(m, ms)
                        ng = 256 // d
                        chunk = (num_splits + ng - 1) // ng
                        l = acc = None
                        for gi in range(ng):
                            lg = np.zeros(len(rows), np.float32)
                            ag = np.zeros((len(rows), d), np.float32)
                            for ms, ls, accs in parts[gi * chunk:(gi + 1) * chunk]:
                                w = np.where(np.isinf(ms), np.float32(0),
                                             np.exp2(ms - np.where(np.isinf(m), np.float32(0), m))).astype(np.float32)
                                lg = lg + ls * w
                                ag = ag + accs * w[:, None]
                            l, acc = (lg, ag) if l is None else (l + lg, acc + ag)
                    inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
                    o[b, h, r0:r1] = acc * inv[:, None]
                    lse2[b, h, r0:r1] = np.where(l > 0, np.log2(np.where(l > 0, l, np.float32(1))) + m, np.float32(-np.inf))
    return orc.to_storage(o, out_dtype), lse2


# ------------------------------------------------------------------------------------------------------------------------
# the value cases: B 2, Hq 4, Hkv 2 - the smallest shapes at which each piece can go wrong.  Sq in {1, 65, 128, 129, 200} (below and
# above the decode limit, one full block, a block plus one row, a ragged second block), cached lengths n in {Sq, Sq + 63, Sq + 64,
# Sq + 65, 321}, both head dims and a padded one, both dtypes and layouts, int8 and +-7 codes, smooth_k off, a caller's sm_scale,
# ragged q_lens / seqlens (q_lens = 0, no keys, fewer keys than queries).  321 keys are 6 tiles: 7 and 9 slices exceed them.
# ------------------------------------------------------------------------------------------------------------------------
SPLITS = (0, 1, 2, 3, 7, 9)
CASES = [
    dict(Sq=1, lens=[1, 64], D=64, dtype="fp16", layout="HND"),
    dict(Sq=1, lens=[65, 66], D=128, dtype="bf16", layout="NHD", splits=(0, 2)),
    dict(Sq=65, lens=[65, 128], D=128, dtype="fp16", layout="NHD", splits=(0, 1, 3)),
    dict(Sq=65, lens=[129, 130], D=64, dtype="bf16", layout="HND", splits=(0, 2, 7)),
    dict(Sq=128, lens=[128, 321], D=64, dtype="fp16", layout="HND"),
    dict(Sq=128, lens=[191, 193], D=128, dtype="bf16", layout="NHD", splits=(1, 2)),
    dict(Sq=128, lens=[192, 321], D=128, dtype="fp16", layout="HND", k_bits=4, splits=(0, 3)),
    dict(Sq=129, lens=[129, 194], D=80, dtype="fp16", layout="NHD", splits=(0, 1, 2)),
    dict(Sq=129, lens=[192, 321], D=128, dtype="fp16", layout="HND", q_bits=4, k_bits=4, splits=(1, 7, 9)),
    dict(Sq=200, lens=[200, 263], D=64, dtype="fp16", layout="HND", smooth_k=False, sm_scale=0.2, splits=(0, 1, 3)),
    dict(Sq=200, lens=[264, 265], D=128, dtype="bf16", layout="HND", splits=(1, 2)),
    dict(Sq=200, lens=[321, 100], q_lens=[200, 37], D=64, dtype="fp16", layout="NHD"),
    dict(Sq=200, lens=[130, 100], q_lens=[0, 150], D=128, dtype="fp16", layout="HND", splits=(0, 1, 2)),   # fewer keys than queries
    dict(Sq=129, lens=[0, 321], q_lens=[129, 5], D=64, dtype="bf16", layout="HND", splits=(0, 1, 7)),      # a sequence with no keys
    # the pairs (Sq, n) of the lists above that the cases so far leave out
    dict(Sq=129, lens=[193, 130], D=64, dtype="fp16", layout="HND", splits=(0, 1, 2)),                     # n = Sq + 64, Sq + 1
    dict(Sq=1, lens=[321, 2], D=128, dtype="fp16", layout="HND", splits=(0, 1, 3, 9)),
    dict(Sq=65, lens=[321, 66], D=64, dtype="fp16", layout="NHD", k_bits=4, splits=(0, 1, 7)),
]
# M = Sq * G <= 64: the shapes at which prefill and decode are both held to the same oracle output
SHORT_CASES = [dict(Sq=16, lens=[130, 77], D=64, dtype="fp16", layout="HND", splits=(0, 1, 3)),
               dict(Sq=32, lens=[321, 40], D=128, dtype="bf16", layout="NHD", splits=(0, 1, 3))]
# the shapes of tests/test_gpu_prefill_containment.py that are held to the oracle (hostile memory; the others compare bits)
CONTAINMENT_LENS, CONTAINMENT_Q_LENS, CONTAINMENT_SQ = [1, 63, 64, 65, 130], [130, 1, 129, 0, 77], 130


def case_id(c):
    extra = "".join(f"-{k}{c[k]}" for k in ("q_bits", "k_bits", "smooth_k", "sm_scale", "B", "HQ", "HKV") if k in c)
    return f"Sq{c['Sq']}n{'_'.join(map(str, c['lens']))}" + (f"q{'_'.join(map(str, c['q_lens']))}" if "q_lens" in c else "") + \
        f"D{c['D']}{c['dtype']}{c['layout']}{extra}"


def _rand(orc, rng, shape, dtype, bias=0.0):
    return orc.to_storage(rng.standard_normal(shape, dtype=np.float32) + np.float32(bias), dtype)


_built = {}


def build_case(orc, c):
    """The data and the reference of one case, computed once and shared (treat as read-only): a dict with the inputs q, k, v
    [.., T, D] (un-padded), the two appends (t0 rows, then the rest, ragged by `lens`) as `steps`, the CacheRef state `ref`, the Q
    codes, the LSE correction and, per causal flag, the oracle's o / natural-log lse."""
    key = case_id(c)
    if key in _built:
        return _built[key]
    Sq, D, dtype = c["Sq"], c["D"], c["dtype"]
    B, HQ, HKV = shape_of(c)
    Dp = 64 if D <= 64 else 128
    lens = np.array(c["lens"])
    q_lens = np.array(c.get("q_lens", [Sq] * B))
    smooth_k, sm_scale = c.get("smooth_k", True), c.get("sm_scale", D ** -0.5)
    q_qmax, k_qmax = (127 if c.get("q_bits", 8) == 8 else 7), (127 if c.get("k_bits", 8) == 8 else 7)
    rng = np.random.default_rng(sum(map(ord, key)))
    T = max(int(lens.max()), 1)
    cap = (T + BLKK - 1) // BLKK * BLKK
    k = _rand(orc, rng, (B, HKV, T, D), dtype, bias=0.5)
    v = _rand(orc, rng, (B, HKV, T, D), dtype)
    q = _rand(orc, rng, (B, HQ, Sq, D), dtype)
    pad = lambda a: np.pad(a, [(0, 0)] * 3 + [(0, Dp - D)])
    t0 = max(1, T // 2)
    steps = [(0, t0, np.minimum(lens, t0))] + ([(t0, T, np.maximum(lens - t0, 0))] if T > t0 else [])
    ref = kr.CacheRef(orc, B, HKV, Dp, cap, dtype, qmax=k_qmax, smooth_k=smooth_k)
    for a, e, nl in steps:
        ref.append(pad(k[:, :, a:e]), pad(v[:, :, a:e]), nl)
    assert np.array_equal(ref.seqlens, lens)
    qp = pad(q)
    q_i8, q_scale = quant_q_blocks(orc, qp, q_lens, sm_scale, q_qmax)
    corr = kr.lse_correction(orc, qp, ref.km if smooth_k else None, dtype)
    out = dict(q=q, k=k, v=v, steps=steps, ref=ref, lens=lens, q_lens=q_lens, q_i8=q_i8, q_scale=q_scale, corr=corr,
               sm_scale=sm_scale, Dp=Dp, cap=cap, splits=c.get("splits", SPLITS), oracle={})
    for causal in (False, True):
        o_ref, lse2_ref = oracle_prefill(orc, q_i8, q_scale, ref, q_lens, causal=causal, out_dtype=dtype)
        out["oracle"][causal] = (o_ref, kr.natural_lse(lse2_ref, corr, sm_scale))
    _built[key] = out
    return out


def chosen_splits(Sq, max_k, batch=B, hq=HQ):
    """the documented rule: max(1, min(ceil(512 / (B Hq ceil(Sq / 128))), tiles / 4, 256))"""
    tiles = (max_k + BLKK - 1) // BLKK
    return max(1, min(-(-512 // (batch * hq * ((Sq + BLKQ - 1) // BLKQ))), tiles // 4, 256))


# ------------------------------------------------------------------------------------------------------------------------
# census helpers: what a case of tests/prefill_fuzz_cases.py exercises.  A fuzz case names Sq, G, Hkv, B, q_lens [B] (resolved),
# lens [B], splits, page and its append schedule; both causal flags are always run, so the causal tile counts are what counts.
# ------------------------------------------------------------------------------------------------------------------------
def q_blocks(c):
    return (c["Sq"] + BLKQ - 1) // BLKQ


def visible_tiles(c, b, qb, causal=True):
    """tiles the Q block `qb` of sequence b walks (0: no valid row, or no key below the limit of its last valid row)"""
    n, ql = c["lens"][b], c["q_lens"][b]
    last = min(qb * BLKQ + BLKQ - 1, ql - 1)
    if last < qb * BLKQ:
        return 0
    see = max(n - ql + 1 + last, 0) if causal else n
    return (see + BLKK - 1) // BLKK


def tiles_per_slice(c, b, qb, ns, causal=True):
    return -(-visible_tiles(c, b, qb, causal) // ns)


def effective_splits(c, ns):
    """a slice count of the case, 0 resolved by the documented rule on the host's bound of the lengths (the rows offered)"""
    return ns or chosen_splits(c["Sq"], max(1, sum(a["T"] for a in c["appends"])), batch=c["B"], hq=c["G"] * c["Hkv"])


def blocks_see_different_tiles(c):
    """distinct non-zero causal tile counts among the Q blocks of one sequence: each block gets its own tps"""
    return max(len({visible_tiles(c, b, qb) for qb in range(q_blocks(c))} - {0}) for b in range(c["B"]))


def slice_count_between_first_and_last_block(c):
    """four Q blocks and a slice count above the first block's causal tiles and below the last block's"""
    if q_blocks(c) < 4:
        return False
    return any(0 < visible_tiles(c, b, 0) < ns < visible_tiles(c, b, q_blocks(c) - 1)
               for b in range(c["B"]) for ns in map(lambda s: effective_splits(c, s), c["splits"]))


def empty_middle_block_next_to_a_full_one(c):
    """a Q block that is not the last of the grid, past q_lens[b] of one sequence while another sequence has rows in it"""
    return any(c["q_lens"][b] <= qb * BLKQ < c["q_lens"][b2]
               for qb in range(1, q_blocks(c) - 1) for b in range(c["B"]) for b2 in range(c["B"]))


def longest_slice(c):
    """most tiles any slice of the case walks: the trips of the look-ahead loop (two tiles a trip)"""
    return max([tiles_per_slice(c, b, qb, effective_splits(c, ns), causal) for b in range(c["B"]) for qb in range(q_blocks(c))
                for ns in c["splits"] for causal in (False, True)] or [0])


def slice_starts_on_odd_tile_inside_page(c):
    """some slice with keys begins on an odd tile that is not the first of its page"""
    tpp = c["page"] // BLKK
    for b in range(c["B"]):
        for qb in range(q_blocks(c)):
            for causal in (False, True):
                nt = visible_tiles(c, b, qb, causal)
                for ns in c["splits"]:
                    tps = -(-nt // effective_splits(c, ns))
                    if any(t0 % 2 and t0 % tpp for t0 in range(tps, nt, max(tps, 1))):
                        return True
    return False


def page_192_with_ragged_tiles_and_odd_tps(c):
    """page 192 (three tiles a page), a tile count that is no multiple of 3 and an odd tps > 1 on it"""
    if c["page"] != 192:
        return False
    return any(visible_tiles(c, b, qb, causal) % 3 and tiles_per_slice(c, b, qb, effective_splits(c, ns), causal) % 2
               and tiles_per_slice(c, b, qb, effective_splits(c, ns), causal) > 1
               for b in range(c["B"]) for qb in range(q_blocks(c)) for ns in c["splits"] for causal in (False, True))


def combine_second_trip(c):
    """more than 256 slices that hold keys, with hundreds of query rows per kv head"""
    return c["Sq"] * c["G"] > 64 and max(c["splits"]) > 256 and max(visible_tiles(c, b, 0, False) for b in range(c["B"])) > 256


def no_keys_next_to_a_full_sequence(c):
    return any(n == 0 and c["q_lens"][b] > 0 for b, n in enumerate(c["lens"])) and \
        any(n >= ql > 0 for n, ql in zip(c["lens"], c["q_lens"]))


def fewer_keys_than_queries(c):
    """0 < n < q_len: causal rows that see no key in front of rows that do"""
    return any(0 < n < ql for n, ql in zip(c["lens"], c["q_lens"]))


def q_len_cuts(c):
    """where q_lens cut: the set of 'row16' (inside a 16-row block), 'wave' (a 32-row edge that is no block edge), 'block' (a
    128-row edge), 'trailing' (whole trailing Q blocks without a valid row), 'zero'"""
    out = set()
    for ql in c["q_lens"]:
        if ql == 0:
            out.add("zero")
        elif ql < c["Sq"]:
            out.add("row16" if ql % 16 else "wave" if ql % BLKQ else "block")
            if (ql + BLKQ - 1) // BLKQ < q_blocks(c):
                out.add("trailing")
    return out


def key_offset_to_tile_edge(c):
    """(n - q_len) % 64 of the sequences that have both queries and keys: the causal limits on both sides of a tile edge"""
    return {(n - ql) % BLKK for n, ql in zip(c["lens"], c["q_lens"]) if n and ql}
