"""Cases of the decode fuzz (tests/test_decode_fuzz_cases_cpu.py, tests/test_gpu_decode_fuzz.py): pure numpy, no torch, no GPU.

`make_case(seed)` draws one case - a query geometry, ragged final lengths, an append schedule that reaches them, the decode
options, three slice counts and a page layout - stratified so that `seed % 16` walks every kernel instance (dtype x padded head
dim x 1 / 2 / 3 / 4 row blocks of 16 query rows).  `PINNED` names the geometry edges one by one, so the suite does not depend
on the draw for them.  `make_data` / `replay` / `decode_reference` turn a case into tensors, into the numpy cache
(`kvcache_reference.CacheRef`) and into the oracle's result on that cache: the CPU test and the GPU test share them, so both
look at the same numbers.

A case is a plain dict:
  name, dtype, Dp (padded head dim), D, mb, Sq, G, Hkv, B, lens [B], capacity, q_bits, k_bits, smooth_k, sm_scale (None: D^-1/2),
  dist ("normal" / "randint"), k_bias, q_layout, q_view (None, or (rows before, rows after, elements before, elements after) of
  the wider buffer q is a view of), is_causal, return_lse, splits (three distinct slice counts; 0: the chosen count),
  page, num_pages, page_seed, data_seed, and
  appends: [dict(T, new_lens ([B] or None: all T rows), layout, packed)] - `packed`: k and v are views into one buffer
  [B, T, 2 Hkv, D] (NHD) or [B, 2 Hkv, T, D] (HND) that holds them side by side.
"""
import numpy as np

import kvcache_reference as kr
import v8_reference as v8

SQ_CHOICES = [1, 2, 3, 4, 5, 7, 8, 11, 13, 16]
G_CHOICES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16]
HEAD_DIMS = {64: [64, 32, 40], 128: [128, 80, 96, 120]}
LEN_CHOICES = [0, 1, 2, "Sq-1", "Sq", 63, 64, 65, 127, 128, 129, 191, 200, 257, 320, 449]
SPLIT_CHOICES = [0, 1, 2, 3, 5, 7, 9, 22, 37, 300]
BITS = [(8, 8), (8, 8), (4, 4), (8, 4), (4, 8)]
PAGES = [64, 128, 192, 256]
SKIPPED_ROW = 1.0e4  # what the rows of an append past new_lens[b] hold: nothing may read them


def stratum(seed):
    """(dtype, padded head dim, row blocks) of seed % 16"""
    s = seed % 16
    return ("fp16", "bf16")[s & 1], (64, 128)[(s >> 1) & 1], (s >> 2) + 1


def _schedule(rng, lens, slack):
    """1-4 appends with a common T each whose per-sequence rows add up to `lens`.  The longest sequence takes every row of
    every append, so the T add up to max(lens) and fit the capacity max(lens) + slack however the host bounds them; one append
    may offer up to `slack` rows more than any sequence takes."""
    B, top = len(lens), max(lens)
    if top == 0:
        return [dict(T=1, new_lens=[0] * B)]
    n = int(rng.integers(1, 5))
    ts = []
    if min(lens) >= 1 and rng.integers(0, 2):  # a uniform first append: every sequence takes all of its rows
        ts.append(int(rng.choice([1, min(lens), int(rng.integers(1, min(lens) + 1))])))
    uniform = bool(ts)
    rest = top - sum(ts)
    while rest > 0:
        if len(ts) == n - 1 or n == 1:
            t = rest
        else:
            t = min(rest, int(rng.choice([1, 1, 2, 63, 64, 65, 70, 130, int(rng.integers(1, rest + 1))])))
        ts.append(t)
        rest -= t
    left = list(lens)
    out = []
    for i, t in enumerate(ts):
        after = sum(ts[i + 1:])
        if i == 0 and uniform:
            take = [t] * B
        else:
            take = []
            for r in left:
                lo, hi = max(0, r - after), min(t, r)
                take.append(int(rng.choice([lo, hi, int(rng.integers(lo, hi + 1))])))
        left = [r - x for r, x in zip(left, take)]
        out.append(dict(T=t, new_lens=None if i == 0 and uniform else take))
    assert all(r == 0 for r in left)
    ragged = [i for i, a in enumerate(out) if a["new_lens"] is not None]
    if slack and ragged and rng.integers(0, 2):
        out[int(rng.choice(ragged))]["T"] += int(rng.integers(1, slack + 1))
    return out


def _finish(case, rng):
    """the derived fields: capacity, schedule, pool size"""
    slack = case.pop("slack")
    case["capacity"] = max(1, max(case["lens"]) + slack)
    sched = case.get("appends") or _schedule(rng, case["lens"], slack)
    for a in sched:
        a.setdefault("layout", str(rng.choice(["HND", "NHD"])))
        a.setdefault("packed", bool(rng.integers(0, 2)))
    case["appends"] = sched
    assert sum(a["T"] for a in sched) <= max(case["capacity"], 1)
    case["max_pages"] = -(-case["capacity"] // case["page"])
    case["num_pages"] = case["B"] * case["max_pages"] + int(rng.integers(0, 4))
    case["mb"] = -(-case["Sq"] * case["G"] // 16)
    case["Dp"] = 64 if case["D"] <= 64 else 128
    return case


def make_case(seed):
    dtype, Dp, mb = stratum(seed)
    rng = np.random.default_rng(seed)
    D = int(rng.choice(HEAD_DIMS[Dp]))
    while True:
        Sq, G = int(rng.choice(SQ_CHOICES)), int(rng.choice(G_CHOICES))
        if -(-Sq * G // 16) == mb:
            break
    Hkv, B = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3]))
    lens = []
    for _ in range(B):
        x = LEN_CHOICES[int(rng.integers(0, len(LEN_CHOICES)))]
        lens.append(Sq - 1 if x == "Sq-1" else Sq if x == "Sq" else int(x))
    q_bits, k_bits = BITS[int(rng.integers(0, len(BITS)))]
    normal = bool(rng.integers(0, 2))
    smooth_k = bool(rng.integers(0, 4))
    # Integers of magnitude 100 overflow fp16 in dtype(q . km) once km is the mean of a handful of rows (a sequence whose first
    # append is short): the LSE is +inf by the operator's own definition and there is nothing to compare.  Integer data in
    # fp16 therefore run unsmoothed; in bf16 they keep the draw.
    if not normal and dtype == "fp16":
        smooth_k = False
    case = dict(
        name=f"seed{seed}", dtype=dtype, D=D, Sq=Sq, G=G, Hkv=Hkv, B=B, lens=lens, slack=int(rng.integers(0, 131)),
        q_bits=q_bits, k_bits=k_bits, smooth_k=smooth_k,
        sm_scale=None if rng.integers(0, 3) else float(rng.choice([0.07, 0.2, 1.0 / 3.0])),
        dist="normal" if normal else "randint", k_bias=float(rng.choice([0.0, 0.3, -0.5])) if normal else 0.0,
        q_layout=str(rng.choice(["HND", "NHD"])),
        q_view=tuple(int(x) for x in (rng.integers(0, 3), rng.integers(0, 3), 8 * rng.integers(0, 3), 8 * rng.integers(0, 3)))
        if rng.integers(0, 2) else None,
        is_causal=bool(rng.integers(0, 2)), return_lse=bool(rng.integers(0, 2)),
        splits=[int(x) for x in rng.choice(SPLIT_CHOICES, 3, replace=False)],
        page=int(rng.choice(PAGES)), page_seed=seed, data_seed=seed)
    return _finish(case, rng)


def _pin(name, seed, **kw):
    """a hand-written case: everything not given is the plain choice; the append schedule is drawn from `seed` unless given"""
    case = dict(name=name, slack=70, q_bits=8, k_bits=8, smooth_k=True, sm_scale=None, dist="normal", k_bias=0.3, q_layout="HND",
                q_view=None, is_causal=True, return_lse=True, page=64, page_seed=seed, data_seed=1000 + seed)
    case.update(kw)
    return _finish(case, np.random.default_rng(seed))


# The geometry edges (M = Sq * G query rows per kv head, 16 to a row block).  Where the first sequence is long and the second
# short, a workgroup of the first that wrote rows it does not own would finish after the owner and leave its values behind.
PINNED = [
    # head 3 holds rows 15 ... 19: its Q scale is gathered across row blocks 0 and 1.  9 slices at D = 128 are runs of 5 in one
    # batch of 8 whose last three indices are clamped; 22 slices are runs of 11, a partial second batch
    _pin("straddle-M20", 1, dtype="fp16", D=128, Sq=5, G=4, Hkv=2, B=2, lens=[449, 2], splits=[1, 9, 22]),
    # 3 row blocks run on the 4-block instance, the fourth wholly invalid; no smoothing, so no km anywhere
    _pin("mb3-M35", 2, dtype="bf16", D=64, Sq=5, G=7, Hkv=1, B=2, lens=[449, 2], splits=[1, 22, 300], smooth_k=False,
         is_causal=False, q_layout="NHD"),
    # int4-range codes with bf16 and Sq > 1; 37 slices at D = 128 are runs of 19
    _pin("M42-int4-bf16", 3, dtype="bf16", D=128, Sq=7, G=6, Hkv=2, B=1, lens=[257], splits=[2, 37, 300], q_bits=4, k_bits=4,
         page=128),
    # 3 row blocks, all 48 rows valid; a caller's sm_scale; 8-bit Q on 4-bit-range K
    _pin("mb3-full-M48", 4, dtype="fp16", D=128, Sq=3, G=16, Hkv=1, B=2, lens=[449, 1], splits=[1, 3, 22], sm_scale=0.2, k_bits=4,
         page=192, q_view=(1, 2, 8, 16)),
    # one row short of 64; 4-bit-range Q on 8-bit K; integer data, so the softmax is all but one-hot
    _pin("M63-q4k8", 5, dtype="fp16", D=64, Sq=7, G=9, Hkv=1, B=2, lens=[320, 65], splits=[0, 5, 300], q_bits=4, dist="randint",
         k_bias=0.0, is_causal=False, return_lse=False, page=256),
    # one head of 13 rows in one block, a padded head dim, a sequence shorter than the query: causal rows that see no key
    _pin("M13-short-seq", 6, dtype="bf16", D=40, Sq=13, G=1, Hkv=3, B=2, lens=[12, 129], splits=[1, 2, 7], q_layout="NHD",
         q_view=(0, 1, 0, 8)),
    # M = 33: one valid row in the third block; an empty sequence and a full last block; a padded head dim at D = 128
    _pin("M33-one-row-in-block-2", 7, dtype="fp16", D=80, Sq=11, G=3, Hkv=2, B=3, lens=[0, 191, 64], splits=[1, 7, 22], page=128,
         k_bias=-0.5),
    # 300 tiles in 300 slices: the only shape at which a slice past the 256th holds keys, so the combine's strided maximum
    # loop has something to find on its second trip.  Integer data: the maxima of two slices differ by hundreds of binades, and
    # a maximum taken over the first 256 slices alone overflows the weights of the others
    _pin("max-loop-second-trip", 8, dtype="fp16", D=64, Sq=2, G=8, Hkv=1, B=1, lens=[300 * 64 - 19], splits=[300, 257, 1],
         dist="randint", k_bias=0.0, slack=19, page=256,
         appends=[dict(T=19000, new_lens=None, layout="HND", packed=False), dict(T=181, new_lens=[181], layout="NHD", packed=True)]),
]


def default_cases(n=32, seed0=0):
    return PINNED + [make_case(seed0 + s) for s in range(n)]


# ------------------------------------------------------------------------------------------------------------------------
# census helpers
# ------------------------------------------------------------------------------------------------------------------------
def straddles(c):
    """some query head has rows in two 16-row blocks"""
    return 16 % c["Sq"] != 0 and c["Sq"] * c["G"] > 16


def combine_run(c, splits):
    """slices one combine group adds: ceil(splits / (256 / Dp))"""
    return -(-splits // (256 // c["Dp"]))


def has_blind_rows(c):
    """a causal case in which some query row of some sequence sees no key"""
    return c["is_causal"] and any(n < c["Sq"] for n in c["lens"])


# ------------------------------------------------------------------------------------------------------------------------
# a case's tensors (canonical [B, H, S, D] fp32 arrays holding storage-dtype values) and their strided carriers
# ------------------------------------------------------------------------------------------------------------------------
def _values(orc, rng, shape, c, bias=0.0):
    if c["dist"] == "normal":
        x = rng.standard_normal(shape, dtype=np.float32) + np.float32(bias)
    else:
        x = rng.integers(-100, 100, shape).astype(np.float32)
    return orc.to_storage(x, c["dtype"])


def make_data(orc, c):
    """-> q [B, Hq, Sq, D], [(k, v) [B, Hkv, T, D] per append]; rows past new_lens[b] hold SKIPPED_ROW"""
    rng = np.random.default_rng(c["data_seed"])
    kv = []
    for a in c["appends"]:
        shape = (c["B"], c["Hkv"], a["T"], c["D"])
        k, v = _values(orc, rng, shape, c, c["k_bias"]), orc.to_storage(rng.standard_normal(shape, dtype=np.float32), c["dtype"])
        if a["new_lens"] is not None:
            for b, n in enumerate(a["new_lens"]):
                k[b, :, n:] = SKIPPED_ROW
                v[b, :, n:] = SKIPPED_ROW
        kv.append((k, v))
    q = _values(orc, rng, (c["B"], c["G"] * c["Hkv"], c["Sq"], c["D"]), c)
    return q, kv


def _in_layout(x, layout):
    return x if layout == "HND" else np.ascontiguousarray(x.transpose(0, 2, 1, 3))


def carry_kv(k, v, a):
    """-> (buffer, index of k, index of v): k and v of append `a` in its layout, as views `buffer[index]` of one packed
    buffer, or (k, v, None) as two contiguous arrays"""
    k, v = _in_layout(k, a["layout"]), _in_layout(v, a["layout"])
    if not a["packed"]:
        return k, v, None
    axis = 1 if a["layout"] == "HND" else 2
    h = k.shape[axis]
    sel = lambda lo, hi: tuple(slice(lo, hi) if d == axis else slice(None) for d in range(4))
    return np.concatenate([k, v], axis=axis), sel(0, h), sel(h, 2 * h)


def carry_q(q, c, fill=np.nan):
    """-> (buffer, index): q in the case's layout as the view `buffer[index]` of a wider buffer full of `fill`, or (q, None)"""
    q = _in_layout(q, c["q_layout"])
    if c["q_view"] is None:
        return q, None
    r0, r1, e0, e1 = c["q_view"]
    axis = 2 if c["q_layout"] == "HND" else 1
    shape = list(q.shape)
    shape[axis] += r0 + r1
    shape[3] += e0 + e1
    buf = np.full(shape, fill, np.float32)
    idx = tuple(slice(r0, r0 + q.shape[axis]) if d == axis else slice(e0, e0 + q.shape[3]) if d == 3 else slice(None)
                for d in range(4))
    buf[idx] = q
    return buf, idx


# ------------------------------------------------------------------------------------------------------------------------
# the numpy cache and the reference result
# ------------------------------------------------------------------------------------------------------------------------
def _pad(x, c):
    return np.pad(x, [(0, 0)] * 3 + [(0, c["Dp"] - c["D"])])


def k_qmax(c):
    return 127 if c["k_bits"] == 8 else 7


def new_ref(orc, c):
    cap = -(-c["capacity"] // kr.BLKK) * kr.BLKK
    return kr.CacheRef(orc, c["B"], c["Hkv"], c["Dp"], cap, c["dtype"], qmax=k_qmax(c), smooth_k=c["smooth_k"])


def new_ref_v8(orc, c):
    """the numpy cache of the case's fp8 twin (`v_bits = 8`): the same K state, V as e4m3 codes and scales, `vhat()` what a
    reader sees"""
    cap = -(-c["capacity"] // kr.BLKK) * kr.BLKK
    return v8.CacheRefV8(orc, c["B"], c["Hkv"], c["Dp"], cap, c["dtype"], qmax=k_qmax(c), smooth_k=c["smooth_k"])


def ref_append(orc, c, ref, step, k, v):
    """append number `step` of the case into `ref`.  A uniform first append takes the dense operators' mean (`oracle.mean_seq`),
    as the cache does."""
    a = c["appends"][step]
    if step == 0 and a["new_lens"] is None and c["smooth_k"]:
        ref.km = orc.mean_seq(_pad(k, c), c["dtype"])[:, :, 0]
    ref.append(_pad(k, c), _pad(v, c), a["new_lens"])


def replay(orc, c, kv, new=new_ref):
    ref = new(orc, c)
    for step, (k, v) in enumerate(kv):
        ref_append(orc, c, ref, step, k, v)
    assert list(ref.seqlens) == list(c["lens"])
    return ref


def concatenated(c, kv):
    """per sequence the rows it took, in order: [(k [Hkv, n, D], v)]"""
    out = []
    for b in range(c["B"]):
        take = [a["T"] if a["new_lens"] is None else a["new_lens"][b] for a in c["appends"]]
        out.append(tuple(np.concatenate([x[i][b, :, :t] for x, t in zip(kv, take)], axis=1) for i in (0, 1)))
    return out


def sm_scale_of(c):
    return c["D"] ** -0.5 if c["sm_scale"] is None else c["sm_scale"]


def quantised_q(orc, c, q):
    """-> codes [B, Hq, Sq, Dp], scales [B, Hq]: one block per (batch, query head), sm_scale * log2(e) folded in"""
    return kr.quant_q(orc, _pad(q, c), sm_scale_of(c), 127 if c["q_bits"] == 8 else 7)


def decode_reference(orc, c, ref, q, v=None):
    """the oracle's kernel on `ref`'s state: -> O [B, Hq, Sq, D], natural-log LSE [B, Hq, Sq], corr (dtype(q . km) or None).
    `v`: the V it reads in place of `ref.v` - V^ = `ref.vhat()` for the fp8 twin"""
    q_i8, q_scale = quantised_q(orc, c, q)
    o, lse2 = kr.oracle_decode(orc, q_i8, q_scale, ref.k_codes, ref.k_scale, ref.v if v is None else v, ref.seqlens,
                               causal=c["is_causal"], out_dtype=c["dtype"])
    corr = kr.lse_correction(orc, _pad(q, c), ref.km, c["dtype"])
    return o[..., :c["D"]], kr.natural_lse(lse2, corr, sm_scale_of(c)), corr


def blind_rows(c):
    """[B, Hq, Sq] bool: query rows that see no key"""
    n = np.array(c["lens"])[:, None] - (c["Sq"] - 1 - np.arange(c["Sq"]))[None, :] * int(c["is_causal"])
    return np.broadcast_to((n <= 0)[:, None, :], (c["B"], c["G"] * c["Hkv"], c["Sq"]))


def chosen_splits(c):
    """`lbfa_decode_num_splits` for the case (the host bounds the lengths by the rows offered)"""
    groups, tiles = c["B"] * c["Hkv"], -(-sum(a["T"] for a in c["appends"]) // kr.BLKK)
    return max(1, min(-(-1024 // groups), tiles // 4, 256))
