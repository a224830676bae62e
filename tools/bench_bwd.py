#!/usr/bin/env python3
"""Event-timed attention backward (`lbfa_backward` behind autograd) against torch's own fp16 SDPA backward, same GPU.

    python tools/bench_bwd.py [--steps K] [--warmup W] [--out FILE]

Per shape: the backward alone (autograd.grad of a saved forward, retain_graph) and forward + backward, median over K steps of
HIP events; TFLOP/s with 10 B Hq Sq Sk D for the backward and 14 B Hq Sq Sk D for forward + backward, halved for causal.
torch's SDPA runs on the same fp16 inputs; the backend it picked is read from the kernel names of one profiled step.
Prints one JSON document (and writes it to --out).
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

SHAPES = [
    # name, layout, causal, B, H, S, D
    ("C2", "HND", False, 4, 32, 4096, 64),
    ("C2_causal", "HND", True, 4, 32, 4096, 64),
    ("D128_S8K", "HND", False, 1, 32, 8192, 128),
    ("C3", "NHD", True, 4, 32, 16384, 128),
]


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


def _sdpa_backend(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if "attn" in e.name.lower() or "attention" in e.name.lower()})
    return names[:6]


def run_shape(name, layout, causal, B, H, S, D, steps, warmup):
    import lowbit_quant_fa2_paddle_amd as lb
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shape = (B, H, S, D) if layout == "HND" else (B, S, H, D)
    q, k, v = (torch.randn(shape, device=dev, dtype=torch.float16).requires_grad_() for _ in range(3))
    do = torch.randn(shape, device=dev, dtype=torch.float16)
    flops = 10.0 * B * H * S * S * D * (0.5 if causal else 1.0)
    flops_fb = 14.0 * B * H * S * S * D * (0.5 if causal else 1.0)
    rec = dict(shape=name, layout=layout, causal=causal, B=B, H=H, S=S, D=D)

    def ours_fwd():
        return lb.lowbit_fa_qk_int8_pv_fp16_triton(q, k, v, tensor_layout=layout, is_causal=causal)

    o = ours_fwd()
    ms = _time(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), steps, warmup)
    ms_fb = _time(lambda: torch.autograd.grad(ours_fwd(), (q, k, v), do), steps, warmup)
    rec["int8_bwd_ms"], rec["int8_bwd_tflops"] = ms, flops / ms / 1e9
    rec["int8_fwd_bwd_ms"], rec["int8_fwd_bwd_tflops"] = ms_fb, flops_fb / ms_fb / 1e9
    del o

    # torch's SDPA takes [B, H, S, D]; NHD inputs are viewed as such (strided), as a caller would pass them
    tq, tk, tv, tdo = (t.transpose(1, 2) if layout == "NHD" else t for t in (q, k, v, do))

    def sdpa_fwd():
        return F.scaled_dot_product_attention(tq, tk, tv, is_causal=causal)

    o = sdpa_fwd()
    ms = _time(lambda: torch.autograd.grad(o, (q, k, v), tdo, retain_graph=True), steps, warmup)
    ms_fb = _time(lambda: torch.autograd.grad(sdpa_fwd(), (q, k, v), tdo), steps, warmup)
    rec["sdpa_bwd_ms"], rec["sdpa_bwd_tflops"] = ms, flops / ms / 1e9
    rec["sdpa_fwd_bwd_ms"], rec["sdpa_fwd_bwd_tflops"] = ms_fb, flops_fb / ms_fb / 1e9
    rec["sdpa_kernels"] = _sdpa_backend(lambda: torch.autograd.grad(sdpa_fwd(), (q, k, v), tdo))
    del o
    rec["bwd_speed_vs_sdpa"] = rec["sdpa_bwd_ms"] / rec["int8_bwd_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()
    want = a.shapes.split(",")
    res = dict(label="builder measurement", tool="tools/bench_bwd.py", device=torch.cuda.get_device_name(0),
               torch=torch.__version__, steps=a.steps, warmup=a.warmup,
               flop_count="backward 10*B*Hq*Sq*Sk*D, forward+backward 14*B*Hq*Sq*Sk*D, halved for causal",
               operator="lowbit_fa_qk_int8_pv_fp16_triton (int8 QK, fp16 PV) vs torch.nn.functional.scaled_dot_product_attention fp16",
               results=[])
    for s in SHAPES:
        if s[0] in want:
            res["results"].append(run_shape(*s, a.steps, a.warmup))
            torch.cuda.empty_cache()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
