#!/usr/bin/env python3
"""Event-timed packed-batch backward (`lbfa_backward_varlen` behind autograd) against the dense backward, same GPU.

    python tools/bench_bwd_varlen.py [--steps K] [--warmup W] [--out FILE]

Cases (int8 QK, fp16 PV, fp16 inputs, H = 32):
  equal_4x4096_d64   4 x 4096 tokens, D = 64, not causal, against the dense backward at C2 (B 4, S 4096, HND).
  mixed_d64 / d128   a seeded draw of lengths from 256..8192 summing to about 64K tokens, causal, against
                     (a) the dense backward on the same sequences padded to B x max, and
                     (b) a Python loop of per-sequence dense backward calls (NHD, B = 1).
Each time is the backward alone (autograd.grad of a saved forward, retain_graph), median over K steps of HIP events.
TFLOP/s count the useful work of the packed batch, 10 H D sum_b len_b^2 (halved for causal), for every contender.
Prints one JSON document (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H = 32


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def mixed_lengths(seed=0, total=65536, lo=256, hi=8192):
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < total:
        lens.append(int(rng.integers(lo, hi + 1)))
    return lens


def _varlen(lens, D, causal, steps, warmup, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    tot = sum(lens)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    q, k, v = (torch.randn((tot, H, D), device=dev, dtype=torch.float16).requires_grad_() for _ in range(3))
    do = torch.randn((tot, H, D), device=dev, dtype=torch.float16)
    o = lb.sageattn_varlen(q, k, v, cu, cu, max(lens), max(lens), is_causal=causal)
    ms = _time(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), steps, warmup)
    return ms, (q, k, v, do)


def _dense(B, S, D, causal, layout, steps, warmup, dev):
    import lowbit_quant_fa2_paddle_amd as lb
    shape = (B, H, S, D) if layout == "HND" else (B, S, H, D)
    q, k, v = (torch.randn(shape, device=dev, dtype=torch.float16).requires_grad_() for _ in range(3))
    do = torch.randn(shape, device=dev, dtype=torch.float16)
    o = lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, tensor_layout=layout, is_causal=causal)
    ms = _time(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), steps, warmup)
    del o, q, k, v, do
    return ms


def _loop(lens, D, causal, packed, steps, warmup):
    import lowbit_quant_fa2_paddle_amd as lb
    q, k, v, do = packed
    starts = np.concatenate([[0], np.cumsum(lens)])
    items = []
    for b, n in enumerate(lens):
        s = slice(int(starts[b]), int(starts[b]) + n)
        qb, kb, vb = (t.detach()[s][None].requires_grad_() for t in (q, k, v))
        ob = lb.lowbit_fa_qk_int8_pv_fp16_triton(qb, kb, vb, tensor_layout="NHD", is_causal=causal)
        items.append((ob, (qb, kb, vb), do[s][None]))

    def run():
        for ob, ins, dob in items:
            torch.autograd.grad(ob, ins, dob, retain_graph=True)

    return _time(run, steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = dict(label="builder measurement", tool="tools/bench_bwd_varlen.py", device=torch.cuda.get_device_name(0),
               torch=torch.__version__, steps=a.steps, warmup=a.warmup, H=H,
               flop_count="backward 10*H*D*sum_b len_b^2, halved for causal (useful work of the packed batch, for every contender)",
               operator="sageattn_varlen (int8 QK, fp16 PV, fp16 inputs) backward vs lowbit_fa_qk_int8_pv_fp16_triton backward",
               results=[])

    lens = [4096] * 4
    flops = 10.0 * H * 64 * sum(n * n for n in lens)
    ms_v, _ = _varlen(lens, 64, False, a.steps, a.warmup, dev)
    torch.cuda.empty_cache()
    ms_d = _dense(4, 4096, 64, False, "HND", a.steps, a.warmup, dev)
    res["results"].append(dict(case="equal_4x4096_d64", causal=False, D=64, lens=lens, tokens=sum(lens),
                               varlen_bwd_ms=ms_v, varlen_bwd_tflops=flops / ms_v / 1e9,
                               dense_c2_bwd_ms=ms_d, dense_c2_bwd_tflops=flops / ms_d / 1e9, varlen_vs_dense=ms_d / ms_v))
    torch.cuda.empty_cache()

    lens = mixed_lengths()
    for D in (64, 128):
        flops = 10.0 * H * D * sum(n * n for n in lens) * 0.5
        ms_v, packed = _varlen(lens, D, True, a.steps, a.warmup, dev)
        ms_l = _loop(lens, D, True, packed, a.steps, a.warmup)
        del packed
        torch.cuda.empty_cache()
        ms_p = _dense(len(lens), max(lens), D, True, "NHD", a.steps, a.warmup, dev)
        torch.cuda.empty_cache()
        res["results"].append(dict(case=f"mixed_d{D}", causal=True, D=D, B=len(lens), tokens=sum(lens), max_len=max(lens),
                                   padding_fraction=1.0 - sum(n * n for n in lens) / (len(lens) * max(lens) ** 2),
                                   lens=lens, varlen_bwd_ms=ms_v, varlen_bwd_tflops=flops / ms_v / 1e9,
                                   dense_padded_bwd_ms=ms_p, dense_padded_useful_tflops=flops / ms_p / 1e9,
                                   varlen_vs_padded=ms_p / ms_v,
                                   dense_loop_bwd_ms=ms_l, dense_loop_useful_tflops=flops / ms_l / 1e9, varlen_vs_loop=ms_l / ms_v))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
