#!/usr/bin/env python3
"""Benchmark of the low-bit FlashAttention-2 forward hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c2|c3|c4|c4m|c5] [--full] [--dump-outputs DIR]

A "step" is one pass of the whole operator (`lowbit_fa_qk_int8_pv_fp16_triton`: smooth-K mean + per-block
quantisation of Q and K + fused attention) over one batch of synthetic fp16 inputs already resident in HBM.
Default workload = BASELINE.json configs[1]: qk_int8_pv_fp16, HND, B=4 H=32 S=4096 D=64, non-causal.
For N > 1 (launched by torch.distributed.run, one rank per GPU) every rank processes its own batch shard of
that size (the op is independent per (batch, head): no data-path collective) - weak scaling.
Rank 0 prints ONE JSON line.  metric = attention TFLOP/s with the reference's FLOP formula
4*B*H*D*S*S (halved for causal; utils/benchmark.py:212-214).

A plain run sets up, warms up, times the K steps (`value`, `ms_per_step`, and `roofline` from HIP events around the attention
launch of timed steps), writes the output of the last timed step if --dump-outputs is given, and prints the line.  Everything else
runs only with --full: `accuracy` against fp32 SDPA, `fa2_reference` (torch's flash SDPA and this library's own fp16 kernel),
`cpu_baseline`, and, measured in the same process on the same device:
  * `sweep` (N = 1): the whole BASELINE metric range - S in {4K, 8K, 16K, 32K} x D in {64, 128} x {non-causal, causal} for
    qk_int8_pv_fp16 plus C3 / C4 / C4-mixed / the C5 per-GPU shard - whole-operator and attention-kernel TFLOP/s, roofline
    fraction, torch's flash SDPA and this library's own fp16 kernel on the same inputs (example/draw/draw_single.py:15-21
    is the reference's version of this table);
  * `c5_strong` (every N): BASELINE configs[4] itself, qk_int8_pv_fp8 B=32 H32 S32768 D128 split over the N ranks
    (B = 32 / N each, no data-path collective), and the RCCL all-gather of the output shards for N > 1.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# dense MFMA peaks from /opt/skills/guides/MI355X_MICROARCH.md (Matrix cores): fp16/bf16 ~2.5 PF, int8 = 2x,
# non-scaled fp8 = fp16 rate.  Half of the FLOPs are int8 (QK^T), half fp16/fp8 (PV) -> harmonic mix.
PEAK_F16_TF = 2500.0
PEAK_I8_TF = 5000.0
PEAK_MIX_TF = 1.0 / (0.5 / PEAK_I8_TF + 0.5 / PEAK_F16_TF)  # 3333 TFLOP/s

WORKLOADS = {
    # name: (api, B, H, Hkv, S, D, layout, causal, extra kwargs, description)
    "c2": ("int8_fp16", 4, 32, 32, 4096, 64, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S4096 D64 non-causal (BASELINE configs[1])"),
    "c3": ("int8_fp16", 4, 32, 32, 16384, 128, "NHD", True, {}, "qk_int8_pv_fp16 NHD causal B4 H32 S16384 D128 (BASELINE configs[2])"),
    "c4": ("int4_fp16", 4, 32, 32, 8192, 64, "HND", False, {"q_bits": 4}, "qk_int4_pv_fp16 HND B4 H32 S8192 D64 (BASELINE configs[3])"),
    "c4m": ("int4_fp16", 4, 32, 32, 8192, 64, "HND", False, {"q_bits": 8}, "q_int8_k_int4 HND B4 H32 S8192 D64 (BASELINE configs[3], mixed)"),
    "c5": ("int8_fp8", 4, 32, 32, 32768, 128, "HND", False, {}, "qk_int8_pv_fp8 B4 H32 S32768 D128 per GPU (BASELINE configs[4] = B32 over 8 GPUs)"),
    "s8k": ("int8_fp16", 4, 32, 32, 8192, 64, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S8192 D64 non-causal"),
    "s16k": ("int8_fp16", 4, 32, 32, 16384, 64, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S16384 D64 non-causal"),
    "s32k": ("int8_fp16", 4, 32, 32, 32768, 64, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S32768 D64 non-causal"),
    "d128": ("int8_fp16", 4, 32, 32, 4096, 128, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S4096 D128 non-causal"),
    "c2c": ("int8_fp16", 4, 32, 32, 4096, 64, "HND", True, {}, "qk_int8_pv_fp16 HND B4 H32 S4096 D64 causal"),
    "d128c": ("int8_fp16", 4, 32, 32, 4096, 128, "HND", True, {}, "qk_int8_pv_fp16 HND B4 H32 S4096 D128 causal"),
    "d128s16k": ("int8_fp16", 4, 32, 32, 16384, 128, "HND", False, {}, "qk_int8_pv_fp16 HND B4 H32 S16384 D128 non-causal"),
}
# reference's published TFLOP/s for the exact default workload (INT8 non-causal S=4K, B4 H32 D64,
# hardware not stated, kernel-only timing): example/draw/draw_single.py:15-16
PUBLISHED = {"c2": 199.5, "s8k": 201.59, "s16k": 200.47, "s32k": 201.16, "c2c": 167.77}
# --dump-outputs: larger outputs are written as a sample of whole rows of this many bytes in fp32
DUMP_MAX_BYTES = 32 << 20


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def cpu_baseline(B, H, S, D, causal, budget_s=12.0):
    """Naive SDPA (the repo's `manual_scaled_dot_product_attention`, src/core.py:46-69, restated in
    oracle/lowbit_fa_oracle.py) on the host cores, fp32, on a bounded sample of (b,h) slices of the same workload; the op
    is independent per slice so throughput extrapolates linearly.  Paddle is not installed: torch CPU tensor ops stand in
    for the reference's Paddle-CPU path, numpy/BLAS if torch's CPU path fails."""
    import numpy as np
    from oracle import lowbit_fa_oracle as orc
    rng = np.random.default_rng(0)
    q = rng.standard_normal((1, 1, S, D), dtype=np.float32)
    k = rng.standard_normal((1, 1, S, D), dtype=np.float32)
    v = rng.standard_normal((1, 1, S, D), dtype=np.float32)
    impl = "numpy/BLAS (oracle.sdpa_naive)"
    run = lambda: orc.sdpa_naive(q, k, v, is_causal=causal)
    threads = len(os.sched_getaffinity(0))
    try:
        import torch
        tq, tk, tv = (torch.from_numpy(a) for a in (q, k, v))
        orc.sdpa_naive_torch(tq[:, :, :256], tk[:, :, :256], tv[:, :, :256], is_causal=causal)
        run = lambda: orc.sdpa_naive_torch(tq, tk, tv, is_causal=causal)
        impl = "torch CPU ops (oracle.sdpa_naive_torch)"
        threads = int(torch.get_num_threads())
    except Exception:
        try:
            from threadpoolctl import threadpool_info
            threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
        except Exception:
            pass
    run()  # warm the thread pool
    n, t0 = 0, time.perf_counter()
    while True:
        run()
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s or n >= B * H:
            break
    flops = orc.attention_flops(1, 1, S, S, D, causal) * n
    return {"value": round(flops / el / 1e12, 5), "unit": "TFLOP/s", "cores": int(threads), "kind": "port",
            "sample": f"{n} of {B * H} (batch,head) slices of the workload, fp32 naive SDPA "
                      f"(src/core.py:46-69 restated, {impl}), {el:.1f} s"}


def make_inputs(torch, dev, B, H, Hkv, S, D, layout, seed, dist_kind="normal", dtype="fp16"):
    """normal: q,k,v ~ N(0,1) (example/test_sageattn_operator.py:43-52).  randint: the reference's bench distribution
    q,k = randint(-100,100), v ~ N(0,1) (utils/benchmark.py:215-230) - one-hot softmax rows.  normal_exact: N(0,1) with a step
    in channel 0 that puts the first 64 keys 2^23 below all later ones for every query - every Q block overflows its lazy
    pass at the first vote and runs the exact path (row max per tile) over otherwise N(0,1) scores."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    tdt = torch.float16 if dtype == "fp16" else torch.bfloat16
    shp_q = (B, H, S, D) if layout == "HND" else (B, S, H, D)
    shp_k = (B, Hkv, S, D) if layout == "HND" else (B, S, Hkv, D)
    if dist_kind in ("normal", "normal_exact"):
        q = torch.randn(shp_q, generator=g, device=dev, dtype=torch.float32)
        k = torch.randn(shp_k, generator=g, device=dev, dtype=torch.float32)
        if dist_kind == "normal_exact":
            a = 8.0 * (D / 64.0) ** 0.5
            q[..., 0] += a
            ks = k if layout == "HND" else k.transpose(1, 2)
            ks[:, :, :64, 0] -= a
            ks[:, :, 64:, 0] += a
        q, k = q.to(tdt), k.to(tdt)
    else:
        q = torch.randint(-100, 100, shp_q, generator=g, device=dev).to(tdt)
        k = torch.randint(-100, 100, shp_k, generator=g, device=dev).to(tdt)
    v = torch.randn(shp_k, generator=g, device=dev, dtype=torch.float32).to(tdt)
    return q, k, v


def dump_outputs(torch, out_dir, o):
    """--dump-outputs: what the timed path returned in its last step (the operator's `o`) as <out_dir>/o.npy in fp32.  An output
    of more than DUMP_MAX_BYTES in fp32 is written as a fixed sample of its rows (one row = the head dim of one (batch, head,
    token)): row indices drawn by numpy's default_rng(0), in ascending order, so the same arguments always pick the same rows."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    out = o
    rows = o.reshape(-1, o.shape[-1])
    keep = DUMP_MAX_BYTES // (4 * rows.shape[1])
    if rows.shape[0] > keep:
        idx = np.sort(np.random.default_rng(0).choice(rows.shape[0], keep, replace=False))
        out = rows.index_select(0, torch.from_numpy(idx).to(rows.device))
    np.save(os.path.join(out_dir, "o.npy"), out.float().cpu().numpy())


def accuracy_vs_sdpa(torch, o, q, k, v, layout, causal, n_slices=4, row_chunk=2048):
    """The reference's "Loss" column (utils/benchmark.py:276-291: MSE of the kernel's output against SDPA) for the output `o`
    of a TIMED launch: fp32 softmax(q k^T / sqrt(D)) v on `n_slices` sampled (batch, head) slices, computed on the GPU in fp32
    outside the timed region (query rows in chunks: no S x S matrix beyond row_chunk rows)."""
    qh, kh, vh, oh = (t if layout == "HND" else t.transpose(1, 2) for t in (q, k, v, o))
    B, H, S, D = qh.shape
    Hkv = kh.shape[1]
    picks = [(0, 0), (B - 1, H - 1), (B // 2, H // 3), (min(1, B - 1), H // 2)]
    picks = list(dict.fromkeys(picks))[:max(1, min(n_slices, B * H))]
    se, n, mx, ref_sq = 0.0, 0, 0.0, 0.0
    for b, h in picks:
        hk = h // (H // Hkv)
        kk, vv = kh[b, hk].float(), vh[b, hk].float()
        for r0 in range(0, S, row_chunk):
            r1 = min(S, r0 + row_chunk)
            sc = (qh[b, h, r0:r1].float() @ kk.t()) * (D ** -0.5)
            if causal:
                cols = torch.arange(kk.shape[0], device=sc.device)[None, :]
                rows = torch.arange(r0, r1, device=sc.device)[:, None]
                sc = sc.masked_fill(cols > rows, float("-inf"))
            ref = torch.softmax(sc, dim=-1) @ vv
            d = oh[b, h, r0:r1].float() - ref
            se += float((d * d).sum())
            ref_sq += float((ref * ref).sum())
            mx = max(mx, float(d.abs().max()))
            n += d.numel()
    return {"mse": float(f"{se / n:.3e}"), "max_abs": float(f"{mx:.3e}"), "ref_mean_sq": float(f"{ref_sq / n:.3e}"),
            "slices": [list(x) for x in picks], "vs": "fp32 softmax(q k^T / sqrt(D)) v on the same inputs, computed on the GPU "
            "outside the timed region (utils/benchmark.py:276-291 'Loss')", "of": "output of the last timed launch"}


def time_fn(torch, f, iters, warmup=2, warm_s=0.1):
    torch.cuda.synchronize()
    tw, nw = time.perf_counter(), 0
    while nw < warmup or (time.perf_counter() - tw) < warm_s:
        f()
        nw += 1
        if nw % 4 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def sweep_point(torch, lb, lib, dev, name, spec, iters, refs=True, dist_kind="normal", dtype="fp16", accuracy=True):
    """One row of the `sweep` table: whole operator + attention kernel (library-recorded HIP events) + the two 16-bit
    comparison points on the same inputs."""
    api, B, H, Hkv, S, D, layout, causal, extra, desc = spec
    fn = {"int8_fp16": lb.lowbit_fa_qk_int8_pv_fp16_triton, "int4_fp16": lb.lowbit_fa_qk_int4_pv_fp16_triton,
          "int8_fp8": lb.lowbit_fa_qk_int8_pv_fp8_cuda}[api]
    q, k, v = make_inputs(torch, dev, B, H, Hkv, S, D, layout, 99, dist_kind, dtype)
    f = lambda: fn(q, k, v, tensor_layout=layout, is_causal=causal, **extra)
    flops = 4.0 * B * H * D * S * S / (2 if causal else 1)
    # un-counted launches for >= 150 ms (at least 3): the row before may have left the device idle (host-side baselines, frees)
    torch.cuda.synchronize()
    tw, nw = time.perf_counter(), 0
    while nw < 3 or (time.perf_counter() - tw) < 0.15:
        f()
        nw += 1
        if nw % 4 == 0:
            torch.cuda.synchronize()
    evs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o_last = None
    for e0, e1 in evs:
        lib.lbfa_profile_next_attn(e0.cuda_event, e1.cuda_event)
        o_last = f()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    ks = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    kms = sum(ks) / iters
    peak = PEAK_I8_TF if api == "int8_fp8" else PEAK_MIX_TF
    row = {"workload": name, "api": api, "B": B, "H": H, "S": S, "D": D, "layout": layout, "causal": causal,
           "dist": dist_kind, "dtype": dtype,
           "ms": round(dt * 1e3, 4), "tflops": round(flops / dt / 1e12, 1), "kernel_ms": round(kms, 4),
           "kernel_ms_median": round(ks[len(ks) // 2], 4),
           "kernel_tflops": round(flops / (kms * 1e-3) / 1e12, 1), "frac": round(flops / (kms * 1e-3) / 1e12 / peak, 4)}
    if accuracy:
        row["accuracy"] = accuracy_vs_sdpa(torch, o_last, q, k, v, layout, causal, n_slices=2 if S >= 16384 else 4)
    del o_last
    if refs and api != "int8_fp8":
        try:
            from torch.nn.attention import sdpa_kernel, SDPBackend
            qh, kh, vh = (t if layout == "HND" else t.transpose(1, 2) for t in (q, k, v))
            with sdpa_kernel(SDPBackend.FLASH_ATTENTION):
                d2 = time_fn(torch, lambda: torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, is_causal=causal), max(3, iters // 2))
            row["torch_fa2_tflops"] = round(flops / d2 / 1e12, 1)
            row["vs_torch_fa2"] = round(d2 / dt, 3)
        except Exception as e:
            row["torch_fa2_error"] = str(e)[:80]
        from lowbit_quant_fa2_paddle_amd import core as _core
        d3 = time_fn(torch, lambda: _core.flash_attn_fp16(q, k, v, tensor_layout=layout, is_causal=causal), max(3, iters // 2))
        row["own_fp16_tflops"] = round(flops / d3 / 1e12, 1)
        row["vs_own_fp16"] = round(d3 / dt, 3)
    del q, k, v
    return row


def run_sweep(torch, lb, lib, dev):
    rows = []
    # one throw-away point first: library / allocator / flash-backend initialisation must not land in the first row
    sweep_point(torch, lb, lib, dev, "warm-up", ("int8_fp16", 1, 8, 8, 2048, 64, "HND", False, {}, "warm-up"), 3, accuracy=False)
    sweep_point(torch, lb, lib, dev, "warm-up", ("int8_fp16", 1, 8, 8, 2048, 128, "HND", True, {}, "warm-up"), 3, accuracy=False)
    its = {4096: 40, 8192: 16, 16384: 6, 32768: 3}
    for D in (64, 128):
        for causal in (False, True):
            for S in (4096, 8192, 16384, 32768):
                nm = f"int8_fp16 S{S // 1024}K D{D}{' causal' if causal else ''}"
                spec = ("int8_fp16", 4, 32, 32, S, D, "HND", causal, {}, nm)
                rows.append(sweep_point(torch, lb, lib, dev, nm, spec, its[S]))
    for nm in ("c3", "c4", "c4m", "c5"):
        rows.append(sweep_point(torch, lb, lib, dev, nm, WORKLOADS[nm], 3, refs=(nm != "c5")))
    # the same shapes on other inputs: the reference's own bench distribution (every Q block leaves the lazy pass at its first
    # vote), N(0,1) scores forced onto the exact path, and bf16 storage (V is converted to fp16 as src/core.py:307-308 does)
    for dist_kind in ("randint", "normal_exact"):
        for nm, S, it in (("c2", 4096, 40), ("s16k", 16384, 6), ("c3", 16384, 3)):
            row = sweep_point(torch, lb, lib, dev, f"{nm} {dist_kind}", WORKLOADS[nm], it, refs=False, dist_kind=dist_kind)
            if dist_kind == "randint" and nm in PUBLISHED:  # the like-for-like comparison: the reference's own input distribution
                row["vs_published"] = {"whole_op": round(row["tflops"] / PUBLISHED[nm], 3), "kernel_only": round(row["kernel_tflops"] / PUBLISHED[nm], 3),
                                       "published_tflops": PUBLISHED[nm]}
            rows.append(row)
    for nm, spec, it in (("c2 bf16", WORKLOADS["c2"], 40), ("c3 bf16", WORKLOADS["c3"], 3),
                         ("int8_fp16 S8K D128 bf16", ("int8_fp16", 4, 32, 32, 8192, 128, "HND", False, {}, ""), 16)):
        rows.append(sweep_point(torch, lb, lib, dev, nm, spec, it, refs=False, dtype="bf16"))
    torch.cuda.empty_cache()
    return rows


def c5_strong(torch, lb, dev, world, rank, distributed, dist, share, steps=3):
    """BASELINE configs[4]: qk_int8_pv_fp8, B=32 H=32 S=32768 D=128 split over `world` ranks by batch."""
    Bg, H, S, D = 32, 32, 32768, 128
    if Bg % world != 0:
        return None
    B = Bg // world
    q, k, v = make_inputs(torch, dev, B, H, H, S, D, "HND", 4321 + rank)
    f = lambda: lb.lowbit_fa_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout="HND", is_causal=False)
    o = f()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    t0 = time.perf_counter()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i in range(steps):
        o = f()
        evs[i + 1].record()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    el = (time.perf_counter() - t0) / steps
    step_ms = [round(evs[i].elapsed_time(evs[i + 1]), 2) for i in range(steps)]  # per launch: a slow FIRST one = memory first touch
    rank_ms = [round(el * 1e3, 3)]
    if distributed:
        tt = torch.tensor([el], device="cpu" if share else dev, dtype=torch.float64)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)  # per-rank times: a future SCALE record shows imbalance between the shards
        rank_ms = [round(float(x.item()) * 1e3, 3) for x in allt]
        el = max(float(x.item()) for x in allt)
    flops = 4.0 * Bg * H * D * S * S
    res = {"workload": "qk_int8_pv_fp8 B32 H32 S32768 D128 (BASELINE configs[4]), batch split over the ranks, strong scaling",
           "B_per_gpu": B, "ms": round(el * 1e3, 3), "tflops_total": round(flops / el / 1e12, 1), "steps": steps,
           "rank_ms_min": min(rank_ms), "rank_ms_max": max(rank_ms), "rank_ms": rank_ms, "step_ms_rank0": step_ms}
    if distributed:
        from lowbit_quant_fa2_paddle_amd import dist as lbdist
        try:  # the gather is reported, never part of `value`: a backend that cannot do it must not lose the bench line
            lbdist.all_gather_batch(o)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(2):
                lbdist.all_gather_batch(o)
            torch.cuda.synchronize()
            dist.barrier()
            res["allgather_ms"] = round((time.perf_counter() - t0) / 2 * 1e3, 3)
            res["allgather_bytes_per_rank"] = int(o.numel() * o.element_size())
        except Exception as e:
            res["allgather_error"] = str(e)[:160]
    del q, k, v, o
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--dist", default="normal", choices=["normal", "randint", "normal_exact"],
                    help="normal: q,k,v ~ N(0,1) (example/test_sageattn_operator.py:43-52); randint: the reference "
                         "bench distribution q,k = randint(-100,100), v ~ N(0,1) (utils/benchmark.py:215-230); "
                         "normal_exact: N(0,1) scores forced onto the exact softmax path (see make_inputs)")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"], help="storage dtype of q, k, v and o")
    ap.add_argument("--prewarm-ms", type=float, default=300.0,
                    help="un-counted operator launches for at least this long BEFORE the --warmup steps: the first launches "
                         "of a process run slow (clock ramp, code-object and allocator first touch), and 5 warm-up steps of "
                         "0.5 ms do not cover that")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: accuracy vs fp32 SDPA, torch's flash SDPA and "
                         "the own fp16 kernel, the sweep, C5 strong scaling and the CPU baseline (each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the output of the last timed step to DIR/o.npy (fp32; a fixed sample of rows beyond 32 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernel-timer-every", type=int, default=2,
                    help="bracket the attention kernel of every N-th timed step with HIP events (each pair costs the step ~6 us of "
                         "queue barriers: timing every step would tax `value` by 1 %%)")
    ap.add_argument("--no-fa2", action="store_true", help="skip the torch flash-attention comparison point")
    ap.add_argument("--gather", action="store_true", help="N>1: also time the RCCL all-gather of the output shards")
    ap.add_argument("--no-sweep", action="store_true", help="skip the S x D x causal sweep (N = 1) that fills the `sweep` key")
    ap.add_argument("--no-c5", action="store_true", help="skip the C5 strong-scaling measurement that fills `c5_strong`")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    import lowbit_quant_fa2_paddle_amd as lb
    from lowbit_quant_fa2_paddle_amd import _lib
    _lib.load()  # fail loudly when the HIP library is missing

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE=1 here)")
    distributed = world > 1
    # LBFA_BENCH_SHARE_GPU=1 (rehearsal on a one-GPU box): ranks share the visible devices round-robin and rendezvous
    # over gloo - RCCL cannot place two ranks on one device.  The driver's multi-GPU runs use one GPU per rank + nccl.
    share = os.environ.get("LBFA_BENCH_SHARE_GPU") == "1"
    dev_index = local_rank % torch.cuda.device_count() if share else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    api, B, H, Hkv, S, D, layout, causal, extra, desc = WORKLOADS[args.workload]
    fn = {"int8_fp16": lb.lowbit_fa_qk_int8_pv_fp16_triton, "int4_fp16": lb.lowbit_fa_qk_int4_pv_fp16_triton,
          "int8_fp8": lb.lowbit_fa_qk_int8_pv_fp8_cuda}[api]

    q, k, v = make_inputs(torch, dev, B, H, Hkv, S, D, layout, 1234 + rank, args.dist, args.dtype)

    def step():
        return fn(q, k, v, tensor_layout=layout, is_causal=causal, **extra)

    # per-launch timing of the dominant kernel with HIP events recorded by the library itself on the launch stream
    # (lbfa_profile_next_attn: the next fused-attention launch is bracketed by the two events), inside the timed region
    lib = _lib.load()
    attn_events = []
    timed_steps = [i for i in range(args.steps) if i % max(1, args.kernel_timer_every) == 0]
    for _ in timed_steps:  # created and materialised before the timed region (the library re-records them)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); e1.record()
        attn_events.append((e0, e1, e0.cuda_event, e1.cuda_event))

    def arm_kernel_timer(i):
        if i % max(1, args.kernel_timer_every) == 0:
            ev = attn_events[i // max(1, args.kernel_timer_every)]
            lib.lbfa_profile_next_attn(ev[2], ev[3])

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    # stated pre-warm (not part of --warmup, not timed): operator launches until `prewarm_ms` of wall time have passed
    torch.cuda.synchronize()
    tp0, prewarm_steps = time.perf_counter(), 0
    while (time.perf_counter() - tp0) * 1e3 < args.prewarm_ms:
        for _ in range(8):
            o = step()
        torch.cuda.synchronize()
        prewarm_steps += 8
    for _ in range(args.warmup):
        o = step()
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        arm_kernel_timer(i)
        o = step()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    if distributed:
        tt = torch.tensor([elapsed], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    ms_per_step = elapsed / args.steps * 1e3
    flops_rank = 4.0 * B * H * D * S * S / (2 if causal else 1)
    value = world * flops_rank / (elapsed / args.steps) / 1e12
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, args.dump_outputs, o)

    kern_all = sorted(ev[0].elapsed_time(ev[1]) for ev in attn_events)
    kern_ms = sum(kern_all) / max(len(kern_all), 1)
    kern_med = kern_all[len(kern_all) // 2] if kern_all else 0.0
    achieved = flops_rank / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
    # fp8 PV runs on the block-scaled MFMA (2x the fp16 rate = the int8 rate): both halves of the FLOPs at 5 PFLOP/s
    peak = PEAK_I8_TF if api == "int8_fp8" else PEAK_MIX_TF
    traffic = None
    tf = os.path.join(ROOT, "profiles", "traffic.json")  # HBM bytes per launch from rocprofv3 --pmc passes
    if os.path.exists(tf):
        try:
            traffic = json.load(open(tf)).get(args.workload)
        except Exception:
            traffic = None

    gather_ms = None
    if distributed and args.gather:
        from lowbit_quant_fa2_paddle_amd import dist as lbdist
        barrier()
        t0 = time.perf_counter()
        for _ in range(5):
            lbdist.all_gather_batch(o)
        barrier()
        gather_ms = (time.perf_counter() - t0) / 5 * 1e3

    # FA2-class fp16 comparison point on the SAME GPU and inputs (the reference's headline claim is "2.4x over
    # FlashAttention-2"): torch's flash-attention SDPA backend (AOTriton on ROCm).  Reported, never part of `value`.
    fa2 = None
    if args.full and rank == 0 and not args.no_fa2 and api != "int8_fp8":
        try:
            from torch.nn.attention import sdpa_kernel, SDPBackend
            qh, kh, vh = (t if layout == "HND" else t.transpose(1, 2) for t in (q, k, v))
            with sdpa_kernel(SDPBackend.FLASH_ATTENTION):
                for _ in range(3):
                    torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, is_causal=causal)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, is_causal=causal)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 10
            fa2 = {"impl": "torch.nn.functional.scaled_dot_product_attention, FLASH_ATTENTION backend, fp16, same inputs",
                   "tflops": round(flops_rank / dt / 1e12, 2), "ms": round(dt * 1e3, 4),
                   "speedup_whole_op": round((flops_rank / (elapsed / args.steps)) / (flops_rank / dt), 3),
                   "speedup_kernel_only": round(achieved / (flops_rank / dt / 1e12), 3) if achieved else None}
        except Exception as e:  # backend not available for this shape/build
            fa2 = {"impl": "torch SDPA flash backend", "error": str(e)[:120]}
        # ... and this library's own un-quantised kernel (lbfa_sdpa_fwd: same tiling, fp16 MFMAs for both products)
        from lowbit_quant_fa2_paddle_amd import core as _core
        for _ in range(3):
            _core.flash_attn_fp16(q, k, v, tensor_layout=layout, is_causal=causal)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            _core.flash_attn_fp16(q, k, v, tensor_layout=layout, is_causal=causal)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 10
        fa2["own_fp16_kernel"] = {"impl": "lbfa_sdpa_fwd (this library, un-quantised fp16 QK^T and PV), same inputs",
                                  "tflops": round(flops_rank / dt / 1e12, 2), "ms": round(dt * 1e3, 4),
                                  "lowbit_speedup_whole_op": round(dt / (elapsed / args.steps), 3)}

    acc = None
    if args.full and rank == 0:
        acc = accuracy_vs_sdpa(torch, o, q, k, v, layout, causal)
    if distributed:
        dist.barrier()
    del q, k, v, o
    torch.cuda.empty_cache()
    sweep = None
    if args.full and rank == 0 and world == 1 and not args.no_sweep and args.workload == "c2":
        sweep = run_sweep(torch, lb, lib, dev)
    c5s = None
    if args.full and not args.no_c5 and args.workload == "c2":
        c5s = c5_strong(torch, lb, dev, world, rank, distributed, dist if distributed else None, share)
    # the host-side baseline last: 12 s of all host cores and tens of GB of host memory in front of the big-footprint GPU runs above
    # coincided with `c5_strong` reading 25 % slow on some pool devices (round 4; the B = 4 shard of the same kernel was unaffected)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(B, H, S, D, causal)

    if rank == 0:
        out = {
            "metric": "attention TFLOP/s, qk_int8_pv_fp16 B4 H32 D64 S=4096 fwd" if args.workload == "c2" else f"attention TFLOP/s, {desc}",
            "value": round(value, 2),
            "unit": "TFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "full": args.full,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / PUBLISHED[args.workload], 3) if (args.workload in PUBLISHED and world == 1) else None,
            "dtype": "int8 (QK^T) + fp16 (PV), fp32 softmax/accumulate" if api != "int8_fp8" else "int8 (QK^T) + fp8 e4m3 (PV), fp32 softmax/accumulate",
            "data": f"synthetic, {({'normal': 'q,k,v ~ N(0,1)', 'randint': 'q,k = randint(-100,100), v ~ N(0,1)', 'normal_exact': 'N(0,1) with the first key tile 2^23 below the rest (exact softmax path)'})[args.dist]} {args.dtype}, resident in HBM",
            "config": {"workload": desc, "global_batch": B * world, "heads": H, "seq_len": S, "head_dim": D,
                       "layout": layout, "causal": causal, "parallelism": f"batch-shard x{world} (no data-path collective)",
                       "timed": "whole operator: smooth-K mean + per-block quant(Q,K) + fused attention",
                       "kernel_only_tflops_per_gpu": round(achieved, 2), "fwd_latency_ms": round(ms_per_step, 4),
                       "prewarm": f"{prewarm_steps} un-counted operator launches (>= {args.prewarm_ms:.0f} ms) before the {args.warmup} warm-up steps",
                       "kernel_timer": f"HIP events around the attention launch of every {max(1, args.kernel_timer_every)}-th timed step: {len(kern_all)} samples",
                       "baseline_note": "vs_baseline = value / reference's published kernel-only TFLOP/s on unnamed NVIDIA hardware (BASELINE.md). "
                                        "The reference measured on q, k = randint(-100, 100) (utils/benchmark.py:215-230), `value` is on N(0,1): the "
                                        "like-for-like ratio is sweep row 'c2 randint' -> vs_published (whole_op / kernel_only)"},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 4), "traffic": traffic,
                         "frac_of_fp16_roof": round(achieved / PEAK_F16_TF, 4),
                         "hbm_GBps": (round(traffic / (kern_ms * 1e-3) / 1e9, 1) if (traffic and kern_ms > 0) else None),
                         "kernel": ("attn_fwd_kernel" if api == "int8_fp8" else "attn_fwd16_kernel"), "kernel_ms": round(kern_ms, 4), "kernel_ms_median": round(kern_med, 4),
                         "achieved_median": round(flops_rank / (kern_med * 1e-3) / 1e12, 2) if kern_med > 0 else None,
                         "peak_note": ("int8 MFMA for QK^T and block-scaled e4m3 MFMA for PV: 5000 both" if api == "int8_fp8" else
                                       "mixed roof 1/(0.5/5000 + 0.5/2500): half the FLOPs int8 MFMA, half fp16 MFMA")},
            "accuracy": acc,
            "cpu_baseline": cpu,
            "fa2_reference": fa2,
        }
        if gather_ms is not None:
            out["config"]["allgather_ms"] = round(gather_ms, 3)
        if sweep is not None:
            out["sweep"] = sweep
        if c5s is not None:
            out["c5_strong"] = c5s
        print(json.dumps(out), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
