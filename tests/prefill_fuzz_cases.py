"""Cases of the prefill fuzz (tests/test_prefill_fuzz_cases_cpu.py, tests/test_gpu_prefill_fuzz.py): pure numpy, no torch, no GPU.

The sibling of tests/decode_fuzz_cases.py for cached prefill (`lowbit_fa_prefill`) and the fp8 V cache, built from that module's
pieces: its append schedules (`_schedule`), its strided carriers (`carry_kv`, `carry_q`), its data conventions (`_values`,
`SKIPPED_ROW`) and its rule for km (`ref_append`).

`make_case(seed)` draws one case - a head geometry, a query length with ragged `q_lens`, key lengths placed around them, an
append schedule that reaches the key lengths, the options, three slice counts and a page layout with a `slots` permutation -
stratified so that `seed % 8` walks (dtype, padded head dim, v_bits).  Every case runs on the contiguous and on the paged cache
and with both causal flags, so 8 strata cover all 16 prefill kernel instances.  `PINNED` names the edges one by one.

A case is a plain dict with the fields of a decode-fuzz case (name, dtype, Dp, D, Sq, G, Hkv, B, lens [B], capacity, q_bits,
k_bits, smooth_k, sm_scale, dist, k_bias, q_layout, q_view, return_lse, splits, page, num_pages, max_pages, page_seed, data_seed,
appends) and
  v_bits (16 / 8; with 8 V is multiplied by 3, so the codes spread over the e4m3 range),
  q_lens_arg ([B] or None: what the operator is given), q_lens ([B]: the same with None resolved to Sq),
  num_slots and slots ([B] distinct: sequence b lives in slot slots[b] of the paged cache; the other slots stay empty),
  calls (ascending append steps after which the operator is called; the last step is always one: chunked use).
Drawn cases stay at B * Hq * Sq <= 6000 query rows and <= 705 keys.
"""
import numpy as np

import decode_fuzz_cases as fz
import kvcache_reference as kr
import prefill_reference as pr
import v8_reference as v8
from decode_fuzz_cases import BITS, HEAD_DIMS, PAGES, SKIPPED_ROW, carry_kv, carry_q  # noqa: F401  (the tests take them from here)

B_CHOICES, HKV_CHOICES, G_CHOICES = [1, 2, 3], [1, 2, 3], [1, 2, 3, 4, 5, 8]
SQ_CHOICES = [65, 127, 128, 129, 160, 200, 256, 257, 385, 400]
SQ_SHORT = [1, 5, 16, 32]  # with a G that keeps Sq * G <= 64: the shapes decode takes too
Q_LEN_CHOICES = [None, 0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, "Sq-1", "Sq"]
KEY_CHOICES = [0, 1, "ql-1", "ql", "ql+63", "ql+64", "ql+65", 321, 449, 641, 705]
SPLIT_CHOICES = [0, 1, 2, 3, 5, 7, 9, 13, 22, 37, 300]
MAX_ROWS, MAX_KEYS = 6000, 705
V8_MUL = 3.0  # tests/test_gpu_v8_cache.py: |V| up to ~ 15, codes all over the e4m3 range


def stratum(seed):
    """(dtype, padded head dim, v_bits) of seed % 8"""
    s = seed % 8
    return ("fp16", "bf16")[s & 1], (64, 128)[(s >> 1) & 1], (16, 8)[(s >> 2) & 1]


def _finish(case, rng):
    """the derived fields: resolved q_lens, then capacity, schedule and pool size as the decode fuzz derives them, slots, calls"""
    Sq = case["Sq"]
    arg = case["q_lens_arg"]
    case["q_lens"] = [Sq] * case["B"] if arg is None else [min(max(int(x), 0), Sq) for x in arg]
    spare = case.pop("spare_slots")
    case = fz._finish(case, rng)
    del case["mb"]  # decode's row blocks: prefill has Q blocks of 128 rows (prefill_reference.q_blocks)
    case["num_slots"] = case["B"] + spare
    case.setdefault("slots", [int(x) for x in rng.permutation(case["num_slots"])[:case["B"]]])
    last = len(case["appends"]) - 1
    case["calls"] = sorted(set(case.get("calls") or []) | {last})
    assert case["calls"][-1] == last and case["calls"][0] >= 0
    return case


def make_case(seed):
    dtype, Dp, v_bits = stratum(seed)
    rng = np.random.default_rng(seed)
    D = int(rng.choice(HEAD_DIMS[Dp]))
    while True:
        B, Hkv, G = int(rng.choice(B_CHOICES)), int(rng.choice(HKV_CHOICES)), int(rng.choice(G_CHOICES))
        if rng.integers(0, 6) == 0:
            Sq = int(rng.choice(SQ_SHORT))
            G = int(rng.choice([g for g in G_CHOICES if Sq * g <= 64]))
        else:
            Sq = int(rng.choice(SQ_CHOICES))
        if B * Hkv * G * Sq <= MAX_ROWS:
            break
    # q_lens: None for the whole batch one time in four (always half the time at the decode-sized end, where decode is held to
    # the same oracle output and takes no q_lens), else a draw per sequence
    if rng.integers(0, 2 if Sq * G <= 64 else 4) == 0:
        q_lens_arg = None
    else:
        q_lens_arg = []
        for _ in range(B):
            x = Q_LEN_CHOICES[int(rng.integers(0, len(Q_LEN_CHOICES)))]
            q_lens_arg.append(min(Sq, Sq if x in (None, "Sq") else Sq - 1 if x == "Sq-1" else int(x)))
    lens = []
    for b in range(B):
        ql = Sq if q_lens_arg is None else q_lens_arg[b]
        x = KEY_CHOICES[int(rng.integers(0, len(KEY_CHOICES)))]
        lens.append(max(0, ql + int(x[2:] or 0)) if isinstance(x, str) else int(x))
    assert max(lens) <= MAX_KEYS
    q_bits, k_bits = BITS[int(rng.integers(0, len(BITS)))]
    normal = bool(rng.integers(0, 3))
    smooth_k = bool(rng.integers(0, 4))
    if not normal and dtype == "fp16":  # the decode fuzz's rule: dtype(q . km) of integer data overflows fp16
        smooth_k = False
    case = dict(
        name=f"seed{seed}", dtype=dtype, D=D, v_bits=v_bits, Sq=Sq, G=G, Hkv=Hkv, B=B, q_lens_arg=q_lens_arg, lens=lens,
        slack=int(rng.integers(0, 131)), q_bits=q_bits, k_bits=k_bits, smooth_k=smooth_k,
        sm_scale=None if rng.integers(0, 3) else float(rng.choice([0.07, 0.2, 1.0 / 3.0])),
        dist="normal" if normal else "randint", k_bias=float(rng.choice([0.0, 0.3, -0.5])) if normal else 0.0,
        q_layout=str(rng.choice(["HND", "NHD"])),
        q_view=tuple(int(x) for x in (rng.integers(0, 3), rng.integers(0, 3), 8 * rng.integers(0, 3), 8 * rng.integers(0, 3)))
        if rng.integers(0, 2) else None,
        return_lse=bool(rng.integers(0, 2)), splits=[int(x) for x in rng.choice(SPLIT_CHOICES, 3, replace=False)],
        page=int(rng.choice(PAGES)), page_seed=seed, data_seed=seed, spare_slots=int(rng.integers(0, 3)))
    case = _finish(case, rng)
    if len(case["appends"]) > 1 and rng.integers(0, 3) == 0:  # chunked use: the operator after an earlier append as well
        case["calls"] = sorted({int(rng.integers(0, len(case["appends"]) - 1)), len(case["appends"]) - 1})
    return case


def _pin(name, seed, **kw):
    """a hand-written case: everything not given is the plain choice; the append schedule is drawn from `seed` unless given"""
    case = dict(name=name, v_bits=16, q_lens_arg=None, slack=70, q_bits=8, k_bits=8, smooth_k=True, sm_scale=None, dist="normal",
                k_bias=0.3, q_layout="HND", q_view=None, return_lse=True, page=64, page_seed=seed, data_seed=2000 + seed,
                spare_slots=1)
    case.update(kw)
    return _finish(case, np.random.default_rng(seed))


# The edges.  Seven of the pinned cases are fp8 ones, one per head dim of `HEAD_DIMS`: an fp8 case also runs the fp16-V kernels (on
# the cache that holds V^), so nothing is lost by that.
PINNED = [
    # Four Q blocks (128, 128, 128, 16 rows) on 705 keys: causally block 0 walks 7 tiles and block 3 twelve, so with 9 slices
    # block 0 has slices without a tile and tps = 1 while block 3 has tps = 2 and a last slice cut short; 3 slices is the rule's choice
    _pin("four-q-blocks", 1, dtype="fp16", D=128, v_bits=8, Sq=400, G=2, Hkv=2, B=1, lens=[705], splits=[9, 0, 1], page=128),
    # q_lens [128, 400], a cut at a Q block's edge: blocks 1, 2 (and 3) of sequence 0 have no valid row while sequence 1 fills them
    _pin("empty-middle-blocks", 2, dtype="bf16", D=80, v_bits=8, Sq=400, G=3, Hkv=1, B=2, q_lens_arg=[128, 400], lens=[192, 449],
         splits=[1, 2, 5], q_layout="NHD", k_bias=-0.5),
    # the largest group: head hl of the group writes workspace rows hl * Sq ... , 8 heads of 129 rows
    _pin("G8", 3, dtype="fp16", D=64, v_bits=8, Sq=129, G=8, Hkv=1, B=2, lens=[193, 321], splits=[0, 3, 7], q_view=(1, 2, 8, 16)),
    # no grouping at all, three kv heads, one sequence; 4-bit-range Q on 8-bit K; a caller's sm_scale with smoothing on
    _pin("G1-Hkv3", 4, dtype="bf16", D=96, v_bits=8, Sq=257, G=1, Hkv=3, B=1, lens=[321], splits=[1, 2, 13], q_bits=4,
         sm_scale=0.2, page=128, q_layout="NHD", q_view=(0, 1, 0, 8)),
    # 300 tiles in 300 slices with M = 258 rows per kv head: the combine's strided maximum loop finds something on its second
    # trip (the decode fuzz's max-loop-second-trip at prefill's size).  Integer data: the maxima of two slices differ by hundreds
    # of binades, and a maximum taken over the first 256 slices alone overflows the weights of the others
    _pin("combine-second-trip", 5, dtype="fp16", D=64, Sq=129, G=2, Hkv=1, B=1, lens=[300 * 64 - 19], splits=[300, 257, 1],
         dist="randint", k_bias=0.0, smooth_k=False, slack=19, page=256,
         appends=[dict(T=19000, new_lens=None, layout="HND", packed=False), dict(T=181, new_lens=[181], layout="NHD", packed=True)]),
    # pages of 192 keys (three tiles): 8 and 10 tiles are no multiple of 3; 3 slices of 8 tiles have tps = 3, 2 slices of 10
    # tiles tps = 5 - the second slice starts on tile 5, odd and the last of its page
    _pin("page192-odd-tps", 6, dtype="bf16", D=120, v_bits=8, Sq=160, G=3, Hkv=2, B=2, q_lens_arg=[160, 129], lens=[449, 640],
         splits=[2, 3, 7], page=192, k_bits=4),
    # a sequence with queries and no keys next to a full one
    _pin("no-keys-next-to-full", 7, dtype="fp16", D=32, v_bits=8, Sq=129, G=2, Hkv=2, B=2, lens=[0, 321], splits=[0, 1, 7],
         return_lse=False),
    # fewer keys than queries: the first q_len - n causal rows see nothing, in front of rows that do
    _pin("fewer-keys-than-queries", 8, dtype="bf16", D=40, v_bits=8, Sq=200, G=4, Hkv=1, B=2, q_lens_arg=[200, 150], lens=[100, 64],
         splits=[1, 2, 3], page=256, smooth_k=False),
    # chunked use: 128 keys, 128 more, 65 more, the operator after each append on the same 128 query rows
    _pin("chunked", 9, dtype="fp16", D=128, Sq=128, G=2, Hkv=2, B=2, lens=[321, 200], splits=[0, 1, 2], page=128, calls=[0, 1, 2],
         appends=[dict(T=128, new_lens=None), dict(T=128, new_lens=[128, 72]), dict(T=65, new_lens=[65, 0])]),
    # M = 64: the decode-sized end, where decode takes the same call; the second sequence is shorter than the query
    _pin("decode-sized", 10, dtype="bf16", D=64, Sq=16, G=4, Hkv=2, B=2, lens=[130, 7], splits=[0, 1, 3], q_layout="NHD"),
    # (found by the fuzz: cases that failed once stay here)
]


def default_cases(n=24, seed0=0):
    return PINNED + [make_case(seed0 + s) for s in range(n)]


# ------------------------------------------------------------------------------------------------------------------------
# a case's tensors, its numpy cache and the reference result
# ------------------------------------------------------------------------------------------------------------------------
def make_data(orc, c):
    """-> q [B, Hq, Sq, D], [(k, v) [B, Hkv, T, D] per append], drawn in the decode fuzz's order (per append k then v, then q).
    Rows of an append past new_lens[b] and rows of q at or past q_lens[b] hold SKIPPED_ROW: nothing may read them."""
    rng = np.random.default_rng(c["data_seed"])
    mul = np.float32(V8_MUL if c["v_bits"] == 8 else 1.0)
    kv = []
    for a in c["appends"]:
        shape = (c["B"], c["Hkv"], a["T"], c["D"])
        k = fz._values(orc, rng, shape, c, c["k_bias"])
        v = orc.to_storage(rng.standard_normal(shape, dtype=np.float32) * mul, c["dtype"])
        if a["new_lens"] is not None:
            for b, n in enumerate(a["new_lens"]):
                k[b, :, n:] = SKIPPED_ROW
                v[b, :, n:] = SKIPPED_ROW
        kv.append((k, v))
    q = fz._values(orc, rng, (c["B"], c["G"] * c["Hkv"], c["Sq"], c["D"]), c)
    for b, ql in enumerate(c["q_lens"]):
        q[b, :, ql:] = SKIPPED_ROW
    return q, kv


def new_ref(orc, c):
    """the numpy cache of the case: `CacheRef`, or `CacheRefV8` whose `vhat()` the oracle reads"""
    if c["v_bits"] == 16:
        return fz.new_ref(orc, c)
    cap = -(-c["capacity"] // kr.BLKK) * kr.BLKK
    return v8.CacheRefV8(orc, c["B"], c["Hkv"], c["Dp"], cap, c["dtype"], qmax=fz.k_qmax(c), smooth_k=c["smooth_k"])


ref_append = fz.ref_append  # append number `step` into the numpy cache, km by the decode fuzz's rule
concatenated = fz.concatenated
sm_scale_of = fz.sm_scale_of


def lens_after(c, step):
    """the key lengths once append `step` is in"""
    return [sum(a["T"] if a["new_lens"] is None else a["new_lens"][b] for a in c["appends"][:step + 1]) for b in range(c["B"])]


def quantised_q(orc, c, q):
    """-> q with the rows past q_lens zeroed and padded, codes [B, Hq, Sq, Dp], scales [B, Hq, Q blocks]"""
    qv = fz._pad(q, c).copy()
    for b, ql in enumerate(c["q_lens"]):
        qv[b, :, ql:] = 0
    q_i8, q_scale = pr.quant_q_blocks(orc, qv, c["q_lens"], sm_scale_of(c), 127 if c["q_bits"] == 8 else 7)
    return qv, q_i8, q_scale


def prefill_reference(orc, c, ref, q):
    """the oracle's kernel on `ref`'s present state: -> {causal: (O [B, Hq, Sq, D], natural-log LSE [B, Hq, Sq])}, corr"""
    qv, q_i8, q_scale = quantised_q(orc, c, q)
    corr = kr.lse_correction(orc, qv, ref.km, c["dtype"])
    out = {}
    for causal in (False, True):
        o, lse2 = pr.oracle_prefill(orc, q_i8, q_scale, ref, c["q_lens"], causal=causal, out_dtype=c["dtype"])
        out[causal] = (o[..., :c["D"]], kr.natural_lse(lse2, corr, sm_scale_of(c)))
    return out, corr


def dead_rows(c, lens, causal):
    """[B, Hq, Sq] bool: query rows at or past q_lens[b], and rows that see no key"""
    i = np.arange(c["Sq"])[None, :]
    n, ql = np.array(lens)[:, None], np.array(c["q_lens"])[:, None]
    lim = n - (ql - 1 - i) * int(causal)
    return np.broadcast_to(((i >= ql) | (lim <= 0))[:, None, :], (c["B"], c["G"] * c["Hkv"], c["Sq"]))


def decode_takes_it(c):
    """the shapes at which `lowbit_fa_decode` is the same call: M <= 64 and no q_lens short of Sq"""
    return c["Sq"] * c["G"] <= 64 and all(ql == c["Sq"] for ql in c["q_lens"])
