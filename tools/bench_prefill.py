#!/usr/bin/env python3
"""Event-timed cached prefill (`lowbit_fa_prefill`) against the other ways to compute a chunk over a cached context on the same GPU.

    python tools/bench_prefill.py [--steps K] [--warmup W] [--shapes NAME,...] [--out FILE]

Shapes: Hq 32 / Hkv 8, D in {128, 64}, a chunk of Sq in {128, 512, 2048, 8192} queries, causal (bottom-right), at the end of a
cached context of n in {4K, 32K, 128K} keys (the chunk's own keys included, Sq <= n), B in {1, 8}; the pure prefill Sq = n = 8192
causal; and Sq = 17 / 32 (Sq * G just above decode's 64 rows), non-causal, against a loop of `lowbit_fa_decode` calls.  Arms,
alternated step by step in one process (so drift hits all alike), each step bracketed by HIP events; median and the 10th .. 90th
percentile per arm:
  prefill        `lowbit_fa_prefill` on a filled `LowbitKVCache`, num_splits chosen by lbfa_prefill_num_splits
  prefill_1      the same with one key slice: decides whether the starting split rule stays
  prefill_v8     `lowbit_fa_prefill` on a `LowbitKVCache(..., v_bits=8)` holding the same keys (V as e4m3 codes with a scale per
                 key), the chosen num_splits.  Prefill is not bound by the stream: the arm only has to be no slower than `prefill` -
                 `prefill_v8_over_prefill` is the ratio of the medians, `prefill_v8_not_above_prefill_p90` the verdict
  prefill_k4     `lowbit_fa_prefill` on a `LowbitKVCache(..., k_bits=4, k_packed=True)` holding the same keys (the +-7 K codes two
                 to a byte), the chosen num_splits; measured like `prefill_v8`: `prefill_k4_over_prefill`,
                 `prefill_k4_not_above_prefill_p90`, and `prefill_k4_vs_prefill_output`, the accuracy price of 4-bit K codes
  dense_int8     the dense int8 operator on the 16-bit K, V at the same Sq x Sk, NON-causal (its causal mask needs Sq == Sk) - all a
                 user could do before; it takes the mean, quantises and re-reads the whole context on every call
  dense_causal   the dense int8 operator, causal, where Sq == Sk
  sdpa_fp16      torch's scaled_dot_product_attention on the fp16 K, V with the bottom-right mask (skipped where the score matrix
                 would not fit)
  decode_loop    Sq * G just above 64 only: `lowbit_fa_decode` over pieces of 64 rows per kv head (non-causal, like `prefill` there)
FLOPs of a call: 2 * B * Hq * pairs * D int8 (scores) + the same in fp16 (P V), pairs = Sq * (n - Sq) + Sq * (Sq + 1) / 2 causal,
Sq * n otherwise; share of the mixed roof 1 / (0.5 / 5000 + 0.5 / 2500) = 3333 TFLOP/s the README uses.  Small chunks are bound by
the stream of the cache instead: 3 D bytes per key and kv head over the call's time, as a share of the 6.3 TB/s ceiling.
Every arm is CHECKED before it is timed (`oracle_check`): the numpy oracle is too slow at the timed sizes, so each arm runs once
at a reduced shape of the same kind - B 1, Hq 8 / Hkv 2 (the same G), the same D, mask and num_splits, Sq cut to 256 and the
context to 1024 keys (Sq = n stays Sq = n) - and every element of its output is held to the operator bound
|dO| <= 2e-3 + 2e-3 |O| (tests/kvcache_reference.py `o_bound`) of ITS oracle on those inputs: `oracle_prefill` on a numpy cache
for the prefill arms (`prefill_v8`: on the numpy cache's codes and V^, tests/v8_reference.py; `prefill_k4`: on a numpy cache quantised with qmax 7), `oracle_decode` per 64-row piece for the decode loop, the dense oracle (`lowbit_fa_forward`) for the dense
arms, fp32 attention for fp16 SDPA.  A ratio above 1 ends the run with an error; the ratios go into the JSON
(`oracle_check`).  `max_abs_diff_vs_fp32_attention_last_rows` is a figure at the timed size, beside the check.
Prints one JSON document (and writes it to --out).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_prefill.py --calls-only [--shapes ...]

`--calls-only` fills the cache and makes ten untimed calls of `prefill` and `prefill_1` per shape: the run to put under the
profiler for per-kernel times (profiles/prefill_kernel_trace.json), separate from the timed run.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the references of the tests: prefill_reference, kvcache_reference

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HQ, HKV = 32, 8
G = HQ // HKV
HBM_CEILING = 6.3e12
PEAK_MIX_TF = 1.0 / (0.5 / 5000.0 + 0.5 / 2500.0)
SDPA_MAX_SCORES = 1 << 31  # elements of B x Hq x Sq x n beyond which the sdpa arm is skipped

SHAPES = []  # (name, B, Sq, n, D, causal)
for _d in (128, 64):
    for _b in (1, 8):
        for _n in (4096, 32768, 131072):
            for _sq in (128, 512, 2048, 8192):
                if _sq <= _n:
                    SHAPES.append((f"D{_d}_B{_b}_S{_n // 1024}K_q{_sq}", _b, _sq, _n, _d, True))
    SHAPES.append((f"D{_d}_B1_pure8K", 1, 8192, 8192, _d, True))
    for _sq in (17, 32):
        SHAPES.append((f"D{_d}_B8_S32K_q{_sq}", 8, _sq, 32768, _d, False))


def _pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p * (len(xs) - 1))))]


def flops(B, Sq, n, D, causal):
    pairs = Sq * (n - Sq) + Sq * (Sq + 1) // 2 if causal else Sq * n
    return 2.0 * B * HQ * pairs * D * 2  # int8 scores + fp16 P V


def _inputs(B, Sq, n, D, dev):
    torch.manual_seed(0)
    k = torch.randn((B, HKV, n, D), device=dev, dtype=torch.float16)
    v = torch.randn((B, HKV, n, D), device=dev, dtype=torch.float16)
    q = torch.randn((B, HQ, Sq, D), device=dev, dtype=torch.float16)
    return q, k, v


def _reference_rows(q, k, v, rows, n, Sq, causal):
    """fp32 attention of the query rows `rows` (a slice) of every head: the yardstick of the error column"""
    qs = q[:, :, rows].float().view(q.shape[0], HKV, G, -1, q.shape[-1])
    s = torch.einsum("bhgqd,bhkd->bhgqk", qs, k.float()) * q.shape[-1] ** -0.5
    if causal:
        i = torch.arange(Sq, device=q.device)[rows]
        s = s.masked_fill(torch.arange(n, device=q.device)[None, :] >= (n - Sq + 1 + i)[:, None], float("-inf"))
    return torch.einsum("bhgqk,bhkd->bhgqd", torch.softmax(s, dim=-1), v.float()).reshape(q.shape[0], HQ, -1, q.shape[-1])


def make_arms(lb, q, k, v, cache, causal, splits, with_sdpa, cache8=None, cache_k4=None):
    """name -> call, for inputs of any size: the timed arms and their reduced twins of `oracle_check` are built here alike"""
    Sq, n, dev = q.shape[2], k.shape[2], q.device
    arms = {
        "prefill": lambda: lb.lowbit_fa_prefill(q, cache, is_causal=causal, num_splits=splits),
        "prefill_1": lambda: lb.lowbit_fa_prefill(q, cache, is_causal=causal, num_splits=1),
        "dense_int8": lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v),
    }
    if cache8 is not None:
        arms["prefill_v8"] = lambda: lb.lowbit_fa_prefill(q, cache8, is_causal=causal, num_splits=splits)
    if cache_k4 is not None:
        arms["prefill_k4"] = lambda: lb.lowbit_fa_prefill(q, cache_k4, is_causal=causal, num_splits=splits)
    if causal and Sq == n:
        arms["dense_causal"] = lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, is_causal=True)
    if with_sdpa:
        mask = None
        if causal:
            mask = torch.arange(n, device=dev)[None, :] < (n - Sq + 1 + torch.arange(Sq, device=dev))[:, None]
        arms["sdpa_fp16"] = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True)
    if not causal and Sq * G > 64:
        piece = 64 // G
        arms["decode_loop"] = lambda: torch.cat([lb.lowbit_fa_decode(q[:, :, i:i + piece], cache) for i in range(0, Sq, piece)], dim=2)
    return arms


_oracle_refs = {}


def _oracle_references(D, Sq, n, causal):
    """the reduced problem (B 1, Hq 8 / Hkv 2) and the oracle output of every kind of arm on it, computed once per shape"""
    import numpy as np

    import types

    import kvcache_reference as kr
    import prefill_reference as pr
    import v8_reference as v8
    from oracle import lowbit_fa_oracle as orc
    key = (D, Sq, n, causal)
    if key in _oracle_refs:
        return _oracle_refs[key]
    hq, hkv, sm = 2 * G, 2, D ** -0.5
    rng = np.random.default_rng(1000 * D + Sq + n)
    mk = lambda h, rows: orc.to_storage(rng.standard_normal((1, h, rows, D), dtype=np.float32), "fp16")
    q, k, v = mk(hq, Sq), mk(hkv, n), mk(hkv, n)
    ref = v8.CacheRefV8(orc, 1, hkv, D, (n + 63) // 64 * 64, "fp16")  # the K state and the fp16 V are CacheRef's
    ref.append(k, v)
    q_i8, q_scale = pr.quant_q_blocks(orc, q, [Sq], sm, 127)
    # (oracle_prefill reads V^ of a CacheRefV8: the fp16 arms get the same K state with the fp16 V)
    ref16 = types.SimpleNamespace(k_codes=ref.k_codes, k_scale=ref.k_scale, v=ref.v, seqlens=ref.seqlens)
    want = {"prefill": pr.oracle_prefill(orc, q_i8, q_scale, ref16, [Sq], causal=causal, out_dtype="fp16")[0]}
    want["prefill_1"] = want["prefill"]
    want["prefill_v8"] = pr.oracle_prefill(orc, q_i8, q_scale, ref, [Sq], causal=causal, out_dtype="fp16")[0]
    ref4 = kr.CacheRef(orc, 1, hkv, D, (n + 63) // 64 * 64, "fp16", qmax=7)  # what the packed cache holds, a byte per code
    ref4.append(k, v)
    want["prefill_k4"] = pr.oracle_prefill(orc, q_i8, q_scale, ref4, [Sq], causal=causal, out_dtype="fp16")[0]
    want["dense_int8"] = orc.lowbit_fa_forward(q, k, v, is_causal=False, tail="neg_inf", amax_floor=1e-7)
    if causal and Sq == n:
        want["dense_causal"] = orc.lowbit_fa_forward(q, k, v, is_causal=True, tail="neg_inf", amax_floor=1e-7)
    s = np.einsum("bhgqd,bhkd->bhgqk", q.reshape(1, hkv, G, Sq, D).astype(np.float64), k.astype(np.float64)) * sm
    if causal:
        s = np.where(np.arange(n)[None, :] < (n - Sq + 1 + np.arange(Sq))[:, None], s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    want["sdpa_fp16"] = np.einsum("bhgqk,bhkd->bhgqd", p / p.sum(axis=-1, keepdims=True), v.astype(np.float64)).reshape(1, hq, Sq, D)
    if not causal and Sq * G > 64:  # decode quantises the rows of each piece as one block: its own oracle, piece by piece
        piece, parts = 64 // G, []
        for i in range(0, Sq, piece):
            c8, cs = kr.quant_q(orc, q[:, :, i:i + piece], sm, 127)
            parts.append(kr.oracle_decode(orc, c8, cs, ref.k_codes, ref.k_scale, ref.v, ref.seqlens, causal=False, out_dtype="fp16")[0])
        want["decode_loop"] = np.concatenate(parts, axis=2)
    _oracle_refs[key] = (q, k, v, want)
    return _oracle_refs[key]


def oracle_check(lb, name, Sq, n, D, causal, splits):
    """every arm at the reduced shape against its oracle's bound, every element: -> record for the JSON; raises beyond the bound"""
    import kvcache_reference as kr
    dev = torch.device("cuda:0")
    pure = Sq == n
    Sq_r = min(Sq, 256)
    n_r = Sq_r if pure else max(min(n, 1024), Sq_r)
    q, k, v, want = _oracle_references(D, Sq_r, n_r, causal)
    tq, tk, tv = (torch.from_numpy(a).to(torch.float16).to(dev) for a in (q, k, v))
    # (new_lens given: the mean of the first append is then taken as the numpy cache takes it, over the valid rows in float64)
    cache = lb.LowbitKVCache(1, 2, D, n_r, torch.float16, dev).append(tk, tv, new_lens=torch.full((1,), n_r, dtype=torch.int32))
    cache8 = lb.LowbitKVCache(1, 2, D, n_r, torch.float16, dev, v_bits=8).append(tk, tv, new_lens=torch.full((1,), n_r, dtype=torch.int32))
    cache_k4 = lb.LowbitKVCache(1, 2, D, n_r, torch.float16, dev, k_bits=4, k_packed=True).append(
        tk, tv, new_lens=torch.full((1,), n_r, dtype=torch.int32))
    ratios = {}
    with torch.no_grad():
        for a, fn in make_arms(lb, tq, tk, tv, cache, causal, splits, True, cache8, cache_k4).items():
            got = fn().float().cpu().numpy().astype("float64")
            err = abs(got - want[a])
            ratios[a] = float((err / kr.o_bound(want[a], "fp16")).max())
            if not ratios[a] <= 1.0:
                raise AssertionError(f"{name}: arm {a} is beyond the oracle bound at the reduced shape Sq {Sq_r} n {n_r} D {D} "
                                     f"causal {causal} splits {splits}: worst element at {ratios[a]:.3f} of it, max err {err.max():.3e}")
    return dict(reduced_shape=dict(B=1, Hq=2 * G, Hkv=2, Sq=Sq_r, context=n_r, D=D, causal=causal, num_splits=splits),
                bound="|dO| <= 2e-3 + 2e-3 |O| on every element, against the arm's own oracle", worst_ratio=ratios, passed=True)


def run_shape(name, B, Sq, n, D, causal, steps, warmup):
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    dev = torch.device("cuda:0")
    splits = _lib.load().lbfa_prefill_num_splits(B, HQ, Sq, n)
    checked_by_oracle = oracle_check(lb, name, Sq, n, D, causal, splits)
    q, k, v = _inputs(B, Sq, n, D, dev)
    cache = lb.LowbitKVCache(B, HKV, D, n, torch.float16, dev).append(k, v)
    cache8 = lb.LowbitKVCache(B, HKV, D, n, torch.float16, dev, v_bits=8).append(k, v)
    cache_k4 = lb.LowbitKVCache(B, HKV, D, n, torch.float16, dev, k_bits=4, k_packed=True).append(k, v)
    arms = make_arms(lb, q, k, v, cache, causal, 0, B * HQ * Sq * n <= SDPA_MAX_SCORES, cache8, cache_k4)
    with torch.no_grad():
        rows = slice(max(0, Sq - 64), Sq)  # the last rows see the most keys
        ref = _reference_rows(q, k, v, rows, n, Sq, causal)
        checked = [a for a in arms if a != "dense_int8" or not causal]  # the non-causal dense arm computes something else
        err = {a: float((arms[a]()[:, :, rows].float() - ref).abs().max()) for a in checked}
        for _ in range(warmup):
            for fn in arms.values():
                fn()
        ts = {a: [] for a in arms}
        for _ in range(steps):
            for a, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[a].append(e0.elapsed_time(e1) * 1e3)
    fl = flops(B, Sq, n, D, causal)
    stream_bytes = B * HKV * (n * 3 * D + (n // 64) * 4)
    rec = dict(shape=name, B=B, Hq=HQ, Hkv=HKV, Sq=Sq, context=n, D=D, causal=causal,
               num_splits=splits, flops=fl, cache_bytes=stream_bytes, oracle_check=checked_by_oracle,
               max_abs_diff_vs_fp32_attention_last_rows=err)
    for a in arms:
        rec[a + "_us"] = statistics.median(ts[a])
        rec[a + "_us_p10_p90"] = [_pct(ts[a], 0.1), _pct(ts[a], 0.9)]
    for a in ("prefill", "prefill_1"):
        rec[a + "_tflops"] = fl / (rec[a + "_us"] * 1e-6) / 1e12
        rec[a + "_share_of_mixed_roof"] = rec[a + "_tflops"] / PEAK_MIX_TF
        rec[a + "_share_of_hbm_ceiling_one_pass"] = stream_bytes / (rec[a + "_us"] * 1e-6) / HBM_CEILING
    rec["chosen_vs_one_slice"] = rec["prefill_us"] / rec["prefill_1_us"]
    rec["prefill_v8_over_prefill"] = rec["prefill_v8_us"] / rec["prefill_us"]
    rec["prefill_v8_not_above_prefill_p90"] = rec["prefill_v8_us"] <= rec["prefill_us_p10_p90"][1]
    d8 = (arms["prefill_v8"]().float() - arms["prefill"]().float())
    rec["prefill_v8_vs_prefill_output"] = dict(max_abs=float(d8.abs().max()), mse=float((d8 * d8).mean()))
    rec["prefill_k4_over_prefill"] = rec["prefill_k4_us"] / rec["prefill_us"]
    rec["prefill_k4_not_above_prefill_p90"] = rec["prefill_k4_us"] <= rec["prefill_us_p10_p90"][1]
    d4 = (arms["prefill_k4"]().float() - arms["prefill"]().float())
    rec["prefill_k4_vs_prefill_output"] = dict(max_abs=float(d4.abs().max()), mse=float((d4 * d4).mean()))
    for a in arms:
        if not a.startswith("prefill"):
            rec[f"{a}_over_prefill"] = rec[a + "_us"] / rec["prefill_us"]
    return rec


def calls_only(B, Sq, n, D, causal, calls=10):
    import lowbit_quant_fa2_paddle_amd as lb
    dev = torch.device("cuda:0")
    q, k, v = _inputs(B, Sq, n, D, dev)
    cache = lb.LowbitKVCache(B, HKV, D, n, torch.float16, dev).append(k, v)
    for _ in range(calls):
        lb.lowbit_fa_prefill(q, cache, is_causal=causal)
        lb.lowbit_fa_prefill(q, cache, is_causal=causal, num_splits=1)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--calls-only", action="store_true", help="untimed calls for a profiler run")
    a = ap.parse_args()
    want = a.shapes.split(",")
    if a.calls_only:
        for name, B, Sq, n, D, causal in SHAPES:
            if name in want:
                calls_only(B, Sq, n, D, causal)
                torch.cuda.empty_cache()
        return
    res = dict(label="builder measurement", tool="tools/bench_prefill.py", device=torch.cuda.get_device_name(0),
               torch=torch.__version__, steps=a.steps, warmup=a.warmup,
               timing="HIP events around one call per arm, arms alternated within every step, median and 10th..90th percentile; "
                      "the times include the host's launch path",
               results=[])
    for name, B, Sq, n, D, causal in SHAPES:
        if name in want:
            try:
                res["results"].append(run_shape(name, B, Sq, n, D, causal, a.steps, a.warmup))
            except torch.cuda.OutOfMemoryError as e:  # "where memory allows"
                res["results"].append(dict(shape=name, skipped=f"out of memory: {str(e)[:80]}"))
            torch.cuda.empty_cache()
            print(json.dumps(res["results"][-1]), flush=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
