"""Timing probe: the dense kernels on bf16 against fp16 q/k/v (not a pytest
test).

Dense causal, 16k tokens, hq = hk = 32, d 128: forward alone and forward +
backward through flex_flash_attn_func, both dtypes in one process. Both use
the same MFMA shape and move the same bytes, so parity is the expectation.
Device events, 3 warm-up calls, then 7 windows of 5 calls per (dtype, mode),
all taken round-robin so drift hits all alike; prints one JSON line per
(dtype, mode) with the median, min and max window in ms per call and TFLOPS/s
(4 * area * hq * d forward, x 3.5 forward + backward), then the fp16 / bf16
ratio of the medians. A third variant, fp16_bf16vals, runs the fp16 kernels on
values rounded through bf16: it separates what the fp16 instructions cost from
what fp16 DATA costs. It is there because fp16 measured 3-5 % slower than
bf16 although the hot loops differ in two opcodes only; with bf16-rounded
values forward + backward timed as bf16 does (profiles/fp16_dense.md).

usage: gpu_fp16_perf.py [SEQLEN]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from magi_attention.functional import flex_flash_attn_func  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
HQ = HK = 32
D = 128
ROUNDS, ITERS, WARMUP = 7, 5, 3


def make(dtype, via=None):
    """via: round the values through that dtype first (same bits set as there)"""
    g = torch.Generator().manual_seed(42)
    q, k, v, do = ((torch.randn(S, h, D, generator=g) * 0.5).to(via or dtype)
                   .to(dtype).cuda() for h in (HQ, HK, HK, HQ))
    i32 = dict(dtype=torch.int32, device="cuda")
    qr = torch.tensor([[0, S]], **i32)
    tm = torch.tensor([1], **i32)

    def fwd():
        with torch.no_grad():
            flex_flash_attn_func(q, k, v, qr, qr, tm, max_seqlen_q=S,
                                 max_seqlen_k=S)

    def fwd_bwd():
        q.grad = k.grad = v.grad = None
        q.requires_grad_(True)
        k.requires_grad_(True)
        v.requires_grad_(True)
        out, _ = flex_flash_attn_func(q, k, v, qr, qr, tm, max_seqlen_q=S,
                                      max_seqlen_k=S)
        out.backward(do)

    return {"fwd": fwd, "fwd_bwd": fwd_bwd}


def window(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    # fp16_bf16vals: the fp16 kernels on values rounded to bf16 first, i.e.
    # with the three low mantissa bits clear - same instructions as fp16,
    # same operand bit activity as bf16
    fns = {(name, mode): fn
           for name, dtype, via in (
               ("bf16", torch.bfloat16, None), ("fp16", torch.float16, None),
               ("fp16_bf16vals", torch.float16, torch.bfloat16))
           for mode, fn in make(dtype, via).items()}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    res = {key: [] for key in fns}
    for _ in range(ROUNDS):
        for key, fn in fns.items():
            res[key].append(window(fn))
    area = S * (S + 1) / 2
    med = {}
    for (name, mode), ms in res.items():
        ms = sorted(ms)
        med[name, mode] = ms[len(ms) // 2]
        fl = 4 * area * HQ * D * (3.5 if mode == "fwd_bwd" else 1.0)
        print(json.dumps({
            "dtype": name, "mode": mode, "seqlen": S,
            "ms_median": med[name, mode], "ms_min": ms[0], "ms_max": ms[-1],
            "tflops_median": fl / med[name, mode] / 1e9,
        }))
    for mode in ("fwd", "fwd_bwd"):
        print(json.dumps({
            "mode": mode,
            "fp16_over_bf16": med["fp16", mode] / med["bf16", mode],
            "fp16_bf16vals_over_bf16":
                med["fp16_bf16vals", mode] / med["bf16", mode],
        }))


if __name__ == "__main__":
    main()
