#!/usr/bin/env python3
"""Event-timed decode step (Sq = 1) over the int8 KV cache against the other ways to compute it on the same GPU.

    python tools/bench_decode.py [--steps K] [--warmup W] [--shapes B1_S4K,...] [--out FILE]

Shapes: Hq 32 / Hkv 8, D 128, Sq 1, B in {1, 8, 64} x context in {4K, 32K, 128K}.  Arms, alternated step by step in one process
(so drift hits all alike), each step bracketed by HIP events; median and the 10th .. 90th percentile spread per arm:
  decode       `lowbit_fa_decode` on a filled `LowbitKVCache`, num_splits chosen by lbfa_decode_num_splits
  decode_1     the same with num_splits = 1
  decode_paged      `lowbit_fa_decode` on a `LowbitPagedKVCache` holding the same keys in pages of 64 handed out in a RANDOM order:
                    the worst case, one table look-up per tile and no locality between tiles
  decode_paged_256  the same with pages of 256 keys
  decode_v8         `lowbit_fa_decode` on a `LowbitKVCache(..., v_bits=8)` holding the same keys: V as e4m3 codes with one fp32
                    scale per key, 2 D + 4 bytes per key and kv head instead of 3 D
  decode_v8_paged_256  the same on a `LowbitPagedKVCache(..., v_bits=8)` with pages of 256 keys in a random order
  decode_k4         `lowbit_fa_decode` on a `LowbitKVCache(..., k_bits=4, k_packed=True)` holding the same keys: the +-7 K codes two
                    to a byte, 2.5 D bytes per key and kv head instead of 3 D
  decode_k4_v8      the same with `v_bits=8` as well: 1.5 D + 4 bytes per key and kv head, the smallest cache
  decode_k4_v8_paged_256  the same on a `LowbitPagedKVCache` with pages of 256 keys in a random order
  dense_int8   the dense int8 operator at Sq = 1 on the 16-bit K / V (`lowbit_fa_qk_int8_pv_fp16_triton`): what the library offered
               for a decode step before the cache existed - it re-smooths and re-quantises K on every call
  sdpa_fp16    torch's scaled_dot_product_attention on the fp16 K / V, the Hq / Hkv query heads of a kv head as its query rows
Traffic model of `decode`: per key and kv head D code bytes + 2 D bytes of V, one fp32 scale per 64 keys, plus q and o - over
the time of the whole CALL (host launch path and combine included; the streaming kernel alone: the profiler run below), as a
share of the 6.3 TB/s streaming ceiling of the part.
Prints one JSON document (and writes it to --out).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_decode.py --calls-only [--shapes ...]

`--calls-only` fills the caches and makes ten calls of `decode`, `decode_1`, `decode_paged`, `decode_v8`, `decode_k4` and `decode_k4_v8` per shape, untimed: the run to put
under the profiler for per-kernel times (profiles/decode_kernel_trace.json), separate from the timed run.
The yardstick of the paged arms is the `decode` arm of the same run: `decode_paged*_vs_decode` is the ratio of the medians and
`decode_paged*_within_decode_p10_p90` says whether the paged median lies inside the contiguous arm's 10th .. 90th percentile band.
The fp8-V arms are measured against it too: `decode_v8*_speedup_vs_decode` is decode's median over theirs (its ceiling, from the
bytes alone, is 3 D / (2 D + 4)), `decode_v8*_median_below_decode_p10` says whether the median lies below the 10th percentile of
the `decode` arm, each has its share of the HBM ceiling under its own traffic model, and `decode_v8_vs_decode_output` is what the
format costs in accuracy: max |dO| and the mean squared difference of the `decode_v8` output against the `decode` output.
The packed-K arms likewise: `decode_k4_speedup_vs_decode` (ceiling 3 D / 2.5 D) and `decode_k4_v8*_speedup_vs_decode_v8` (ceiling
(2 D + 4) / (1.5 D + 4)) against the yardstick of the same run, `*_median_below_*_p10`, the share of the HBM ceiling under each
arm's own traffic model, and `decode_k4_vs_decode_output`: the accuracy price of 4-bit K codes (that of `k_bits=4` without packing).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HQ, HKV, D = 32, 8, 128
HBM_CEILING = 6.3e12
SHAPES = [(f"B{b}_S{s // 1024}K", b, s) for b in (1, 8, 64) for s in (4096, 32768, 131072)]


def _pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p * (len(xs) - 1))))]


def _paged_cache(lb, k, v, page, seed, v_bits=16, **kw):
    """the keys of k, v in a paged cache whose pages are handed out in a random order"""
    B, S = k.shape[0], k.shape[2]
    per_seq = (S + page - 1) // page
    g = torch.Generator()
    g.manual_seed(seed)
    order = torch.randperm(B * per_seq, generator=g).tolist()
    return lb.LowbitPagedKVCache(B * per_seq, page, HKV, D, B, per_seq, torch.float16, k.device, page_order=order,
                                 v_bits=v_bits, **kw).append(k, v)


def run_shape(name, B, S, steps, warmup):
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    k = torch.randn((B, HKV, S, D), device=dev, dtype=torch.float16)
    v = torch.randn((B, HKV, S, D), device=dev, dtype=torch.float16)
    q = torch.randn((B, HQ, 1, D), device=dev, dtype=torch.float16)
    cache = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev).append(k, v)
    paged64, paged256 = _paged_cache(lb, k, v, 64, 1), _paged_cache(lb, k, v, 256, 2)
    cache8 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, v_bits=8).append(k, v)
    paged256_8 = _paged_cache(lb, k, v, 256, 2, v_bits=8)
    k4 = dict(k_bits=4, k_packed=True)
    cache_k4 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, **k4).append(k, v)
    cache_k4_8 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, v_bits=8, **k4).append(k, v)
    paged256_k4_8 = _paged_cache(lb, k, v, 256, 2, v_bits=8, **k4)
    q_rows = q.view(B, HKV, HQ // HKV, D)  # the query heads of a kv head as query rows of one head
    arms = {
        "decode": lambda: lb.lowbit_fa_decode(q, cache),
        "decode_1": lambda: lb.lowbit_fa_decode(q, cache, num_splits=1),
        "decode_paged": lambda: lb.lowbit_fa_decode(q, paged64),
        "decode_paged_256": lambda: lb.lowbit_fa_decode(q, paged256),
        "decode_v8": lambda: lb.lowbit_fa_decode(q, cache8),
        "decode_v8_paged_256": lambda: lb.lowbit_fa_decode(q, paged256_8),
        "decode_k4": lambda: lb.lowbit_fa_decode(q, cache_k4),
        "decode_k4_v8": lambda: lb.lowbit_fa_decode(q, cache_k4_8),
        "decode_k4_v8_paged_256": lambda: lb.lowbit_fa_decode(q, paged256_k4_8),
        "dense_int8": lambda: lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v),
        "sdpa_fp16": lambda: F.scaled_dot_product_attention(q_rows, k, v),
    }
    with torch.no_grad():
        ref = arms["sdpa_fp16"]().view(B, HQ, 1, D).float()
        err = {a: float((arms[a]().float() - ref).abs().max()) for a in ("decode", "decode_1", "dense_int8", "decode_v8", "decode_k4", "decode_k4_v8")}
        same = {a: bool(torch.equal(arms[a](), arms["decode"]())) for a in ("decode_paged", "decode_paged_256")}
        same["decode_v8_paged_256_to_decode_v8"] = bool(torch.equal(arms["decode_v8_paged_256"](), arms["decode_v8"]()))
        d8 = arms["decode_v8"]().float() - arms["decode"]().float()
        v8_cost = dict(max_abs=float(d8.abs().max()), mse=float((d8 * d8).mean()), rms_of_decode_output=float(arms["decode"]().float().pow(2).mean().sqrt()))
        same["decode_k4_v8_paged_256_to_decode_k4_v8"] = bool(torch.equal(arms["decode_k4_v8_paged_256"](), arms["decode_k4_v8"]()))
        d4 = arms["decode_k4"]().float() - arms["decode"]().float()
        k4_cost = dict(max_abs=float(d4.abs().max()), mse=float((d4 * d4).mean()), rms_of_decode_output=v8_cost["rms_of_decode_output"])
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
    splits = _lib.load().lbfa_decode_num_splits(B, HKV, S)
    bytes_needed = B * HKV * (S * 3 * D + (S // 64) * 4) + 2 * B * HQ * D * 2
    bytes_needed_v8 = B * HKV * (S * (2 * D + 4) + (S // 64) * 4) + 2 * B * HQ * D * 2  # D code bytes + D e4m3 bytes + a scale per key
    bytes_needed_k4 = B * HKV * (S * 5 * D // 2 + (S // 64) * 4) + 2 * B * HQ * D * 2  # D / 2 packed code bytes + 2 D bytes of V
    bytes_needed_k4_v8 = B * HKV * (S * (3 * D // 2 + 4) + (S // 64) * 4) + 2 * B * HQ * D * 2
    rec = dict(shape=name, B=B, Hq=HQ, Hkv=HKV, Sq=1, context=S, D=D, num_splits=splits, bytes_needed=bytes_needed,
               bytes_needed_v8=bytes_needed_v8, max_abs_diff_vs_sdpa=err, paged_bit_identical_to_decode=same,
               decode_v8_vs_decode_output=v8_cost, bytes_needed_k4=bytes_needed_k4, bytes_needed_k4_v8=bytes_needed_k4_v8,
               decode_k4_vs_decode_output=k4_cost)
    for a in arms:
        rec[a + "_us"] = statistics.median(ts[a])
        rec[a + "_us_p10_p90"] = [_pct(ts[a], 0.1), _pct(ts[a], 0.9)]
    rec["decode_share_of_hbm_ceiling"] = bytes_needed / (rec["decode_us"] * 1e-6) / HBM_CEILING
    for a in ("decode_1", "dense_int8", "sdpa_fp16"):
        rec[f"speedup_vs_{a}"] = rec[a + "_us"] / rec["decode_us"]
    lo, hi = rec["decode_us_p10_p90"]
    for a in ("decode_paged", "decode_paged_256"):
        rec[f"{a}_vs_decode"] = rec[a + "_us"] / rec["decode_us"]
        rec[f"{a}_within_decode_p10_p90"] = lo <= rec[a + "_us"] <= hi
        rec[f"{a}_slower_beyond_spread"] = rec[a + "_us_p10_p90"][0] > hi
    rec["decode_v8_speedup_ceiling"] = 3 * D / (2 * D + 4)
    for a in ("decode_v8", "decode_v8_paged_256"):
        rec[f"{a}_share_of_hbm_ceiling"] = bytes_needed_v8 / (rec[a + "_us"] * 1e-6) / HBM_CEILING
        rec[f"{a}_speedup_vs_decode"] = rec["decode_us"] / rec[a + "_us"]
        rec[f"{a}_median_below_decode_p10"] = rec[a + "_us"] < lo
    rec["decode_k4_speedup_ceiling"] = 3 * D / (2.5 * D)
    rec["decode_k4_v8_speedup_ceiling_vs_decode_v8"] = (2 * D + 4) / (1.5 * D + 4)
    rec["decode_k4_share_of_hbm_ceiling"] = bytes_needed_k4 / (rec["decode_k4_us"] * 1e-6) / HBM_CEILING
    rec["decode_k4_speedup_vs_decode"] = rec["decode_us"] / rec["decode_k4_us"]
    rec["decode_k4_median_below_decode_p10"] = rec["decode_k4_us"] < lo
    lo8 = rec["decode_v8_us_p10_p90"][0]
    for a in ("decode_k4_v8", "decode_k4_v8_paged_256"):
        rec[f"{a}_share_of_hbm_ceiling"] = bytes_needed_k4_v8 / (rec[a + "_us"] * 1e-6) / HBM_CEILING
        rec[f"{a}_speedup_vs_decode_v8"] = rec["decode_v8_us"] / rec[a + "_us"]
        rec[f"{a}_speedup_vs_decode"] = rec["decode_us"] / rec[a + "_us"]
        rec[f"{a}_median_below_decode_v8_p10"] = rec[a + "_us"] < lo8
    # faster than the dense operator by more than the run-to-run spread: its fastest decile against our slowest
    rec["beats_dense_int8_beyond_spread"] = rec["dense_int8_us_p10_p90"][0] > rec["decode_us_p10_p90"][1]
    return rec


def calls_only(B, S, calls=10):
    import lowbit_quant_fa2_paddle_amd as lb
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    k = torch.randn((B, HKV, S, D), device=dev, dtype=torch.float16)
    v = torch.randn((B, HKV, S, D), device=dev, dtype=torch.float16)
    q = torch.randn((B, HQ, 1, D), device=dev, dtype=torch.float16)
    cache = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev).append(k, v)
    paged = _paged_cache(lb, k, v, 64, 1)
    cache8 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, v_bits=8).append(k, v)
    cache_k4 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, k_bits=4, k_packed=True).append(k, v)
    cache_k4_8 = lb.LowbitKVCache(B, HKV, D, S, torch.float16, dev, k_bits=4, k_packed=True, v_bits=8).append(k, v)
    for _ in range(calls):
        lb.lowbit_fa_decode(q, cache)
        lb.lowbit_fa_decode(q, cache, num_splits=1)
        lb.lowbit_fa_decode(q, paged)
        lb.lowbit_fa_decode(q, cache8)
        lb.lowbit_fa_decode(q, cache_k4)
        lb.lowbit_fa_decode(q, cache_k4_8)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--calls-only", action="store_true", help="untimed calls for a profiler run")
    a = ap.parse_args()
    want = a.shapes.split(",")
    if a.calls_only:
        for name, B, S in SHAPES:
            if name in want:
                calls_only(B, S)
                torch.cuda.empty_cache()
        return
    res = dict(label="builder measurement", tool="tools/bench_decode.py", device=torch.cuda.get_device_name(0),
               torch=torch.__version__, steps=a.steps, warmup=a.warmup,
               timing="HIP events around one call per arm, arms alternated within every step, median and 10th..90th percentile; "
                      "the times include the host's launch path (one to three launches per call)",
               results=[])
    for name, B, S in SHAPES:
        if name in want:
            try:
                res["results"].append(run_shape(name, B, S, a.steps, a.warmup))
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
