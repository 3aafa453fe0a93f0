"""Timing probe: fp8 (e4m3) vs bf16 index-attention forward (not a pytest test).

The protocol of tests/gpu_index_bwd_perf.py: device events, 3 warm-up launches
of each kernel per shape, then `reps` windows of `iters` launches; the median
window and the min..max spread are printed. The fp8 and bf16 windows are
interleaved (bf16, fp8, bf16, fp8, ...) in one process on the SAME index
lists; the fp8 tensors are the e4m3 cast of the bf16 ones. Reports ms, TF/s
on 4*tokens*hq*topk*d FLOPs and gathered GB/s (K+V row bytes touched per
launch, 2 B/element for bf16 and 1 B/element for fp8), and the bf16/fp8 time
ratio.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional.flex_flash_attn import (
    _flex_flash_attn_forward_index,
)
from magi_attention.utils import build_index_attn_indices


def _window(fn, iters):
    ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def run(tokens=4096, hq=128, d=128, s_kv=8192, topk=2048, iters=10, reps=5):
    dev = "cuda"
    torch.manual_seed(0)
    q = (torch.randn(tokens, hq, d, device=dev) * 0.5).bfloat16()
    k = (torch.randn(s_kv, 1, d, device=dev) * 0.5).bfloat16()
    v = (torch.randn(s_kv, 1, d, device=dev) * 0.5).bfloat16()
    q8, k8, v8 = (t.to(torch.float8_e4m3fn) for t in (q, k, v))
    if s_kv <= 65536:
        idx = build_index_attn_indices(
            1, 1, tokens, s_kv, topk, topk, device=dev
        ).view(tokens, topk)
    else:
        # HBM-resident regime: sample WITH replacement (perf only - the
        # without-replacement builder would need tokens x s_kv scores)
        idx = (
            torch.randint(0, s_kv, (tokens, topk), device=dev)
            .sort(dim=-1).values.int()
        )
    scale = d ** (-0.5)

    def bf16():
        _flex_flash_attn_forward_index(q, k, v, idx, scale, 0.0)

    def fp8():
        _flex_flash_attn_forward_index(q8, k8, v8, idx, scale, 0.0)

    for _ in range(3):
        bf16()
        fp8()
    torch.cuda.synchronize()
    wb, w8 = [], []
    for _ in range(reps):
        wb.append(_window(bf16, iters))
        w8.append(_window(fp8, iters))
    flops = 4.0 * tokens * hq * topk * d
    rows = 2.0 * tokens * topk * d  # K + V elements touched per launch
    mb, m8 = statistics.median(wb), statistics.median(w8)
    print(
        f"tokens={tokens} hq={hq} d={d} s_kv={s_kv} topk={topk}\n"
        f"  bf16 {mb:8.3f} ms [{min(wb):.3f}..{max(wb):.3f}]  "
        f"{flops / mb / 1e9:7.1f} TF/s  gather {rows * 2 / mb / 1e6:6.0f} GB/s\n"
        f"  fp8  {m8:8.3f} ms [{min(w8):.3f}..{max(w8):.3f}]  "
        f"{flops / m8 / 1e9:7.1f} TF/s  gather {rows * 1 / m8 / 1e6:6.0f} GB/s\n"
        f"  bf16/fp8 time ratio {mb / m8:.2f}",
        flush=True,
    )


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    if args:
        run(*args)
    else:
        run(4096, 128, 128, 8192, 2048)     # DiT ratio-128
        run(16384, 128, 128, 16384, 2048)   # bigger grid
        run(8192, 32, 128, 16384, 1024)     # ratio-32 (W=1 head block)
        run(8192, 64, 64, 16384, 2048)      # d=64
        # HBM-resident gathers (KV pool >> aggregate L2)
        run(8192, 128, 128, 1048576, 2048)  # ratio-128, cold gather
        run(8192, 32, 128, 1048576, 1024)   # ratio-32, cold gather
        run(4096, 16, 128, 8192, 2048)      # small GQA ratio (hq=16)
