"""Timing probe for the index-attention backward kernel (not a pytest test).

Times the forward, the dpsum preprocess and the gather/scatter backward
separately with device events: 3 warm-up launches of every timed call at
every shape, then `reps` windows of `iters` launches each (each window a few
hundred ms at the DiT shape); the median window and the min..max spread are
printed. Reports the bwd/fwd ratio, achieved TF/s on 5*2*tokens*hq*topk*d
FLOPs and the fp32 atomic byte volume 2*tokens*topk*d*4 B (dK + dV, after
the in-workgroup reduction over heads).
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention import _ffa_lib
from magi_attention._ffa_lib import (
    MagiFfaBwdArgs,
    MagiFfaIndexBwdArgs,
    check,
    current_stream_ptr,
    ptr,
)
from magi_attention.functional.flex_flash_attn import (
    _flex_flash_attn_forward_index,
)
from magi_attention.utils import build_index_attn_indices


def _time(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(reps):
        ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
        ev0.record()
        for _ in range(iters):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        windows.append(ev0.elapsed_time(ev1) / iters)
    return statistics.median(windows), min(windows), max(windows)


def run(tokens=4096, hq=128, d=128, s_kv=8192, topk=2048, iters=10, reps=5):
    dev = "cuda"
    torch.manual_seed(0)
    q = torch.randn(tokens, hq, d, dtype=torch.bfloat16, device=dev)
    k = torch.randn(s_kv, 1, d, dtype=torch.bfloat16, device=dev)
    v = torch.randn_like(k)
    dout = torch.randn_like(q)
    idx = build_index_attn_indices(
        1, 1, tokens, s_kv, topk, topk, device=dev
    ).view(tokens, topk)
    scale = d ** (-0.5)
    lib = _ffa_lib.lib()

    out, meta = _flex_flash_attn_forward_index(q, k, v, idx, scale, 0.0)
    lse = meta.lse
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k, dtype=torch.float32)
    dv = torch.zeros_like(v, dtype=torch.float32)
    dpsum = torch.empty(tokens, hq, dtype=torch.float32, device=dev)

    def fwd():
        _flex_flash_attn_forward_index(q, k, v, idx, scale, 0.0)

    def pre():
        a = MagiFfaBwdArgs(
            dout=ptr(dout), out=ptr(out), dpsum=ptr(dpsum),
            total_q=tokens, hq=hq, d=d, out_is_fp32=0,
            stream=current_stream_ptr(),
        )
        check(lib.magi_ffa_bwd_preprocess(a), "preprocess")

    def bwd():
        # accumulators are not re-zeroed between launches: the kernel's work
        # does not depend on their contents
        a = MagiFfaIndexBwdArgs(
            dout=ptr(dout), q=ptr(q), k=ptr(k), v=ptr(v), lse=ptr(lse),
            dpsum=ptr(dpsum), indices_2d=ptr(idx),
            dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
            total_q=tokens, total_k=s_kv, max_topk=topk,
            hq=hq, hk=1, d=d, softmax_scale=scale, softcap=0.0,
            stream=current_stream_ptr(),
        )
        check(lib.magi_ffa_bwd_index(a), "bwd_index")

    pre()
    f_ms, f_lo, f_hi = _time(fwd, iters, reps)
    p_ms, p_lo, p_hi = _time(pre, iters, reps)
    b_ms, b_lo, b_hi = _time(bwd, iters, reps)
    flops_f = 4.0 * tokens * hq * topk * d
    flops_b = 10.0 * tokens * hq * topk * d
    atomic_bytes = 2.0 * tokens * topk * d * 4
    print(
        f"tokens={tokens} hq={hq} d={d} s_kv={s_kv} topk={topk}\n"
        f"  fwd        {f_ms:8.3f} ms [{f_lo:.3f}..{f_hi:.3f}]  "
        f"{flops_f / f_ms / 1e9:7.1f} TF/s\n"
        f"  preprocess {p_ms:8.3f} ms [{p_lo:.3f}..{p_hi:.3f}]\n"
        f"  bwd        {b_ms:8.3f} ms [{b_lo:.3f}..{b_hi:.3f}]  "
        f"{flops_b / b_ms / 1e9:7.1f} TF/s  bwd/fwd {b_ms / f_ms:.2f}  "
        f"atomics {atomic_bytes / 1e9:.2f} GB -> "
        f"{atomic_bytes / b_ms / 1e6:.0f} GB/s",
        flush=True,
    )


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    if args:
        run(*args)
    else:
        run(4096, 128, 128, 8192, 2048)  # the bench's DiT shape
        run(4096, 16, 128, 8192, 2048)   # small GQA ratio (W=1 head block)
