"""Timing probe for q_block_size on the index path (not a pytest test).

Each row is one block-granular mask served two ways in the same process:
  block     q_block_size = B: one list per block of B q token rows, the BLOCK
            kernels (magi_ffa_fwd_index_block / magi_ffa_bwd_index_block);
  per-token the baseline: the same lists expanded to one per token with
            repeat_interleave(B, 0), the per-token kernels (magi_ffa_fwd_index
            / magi_ffa_bwd_index), which is what such a caller ran before.
Forward and backward kernel launches are timed with device events: 3 warm-up
launches of each call at each shape, then `reps` rounds that alternate one
window of `iters` launches of either way; the median window, the min..max
spread and the per-token / block ratio are printed, with achieved TF/s on
4 (fwd) and 10 (bwd) * tokens*hq*topk*d FLOPs. The forward call includes the
out/lse fills of _flex_flash_attn_forward_index on both sides; the backward
is the gather/scatter kernel alone (dpsum preprocess is row-wise and the same
for both). Before timing, out and lse of the two ways are compared.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention import _ffa_lib
from magi_attention._ffa_lib import check, current_stream_ptr, ptr
from magi_attention.functional import _ffa_launch
from magi_attention.functional.flex_flash_attn import (
    _flex_flash_attn_forward_index,
)


def _time_pair(fa, fb, iters, reps):
    for fn in (fa, fb):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    wins = ([], [])
    for _ in range(reps):
        for fn, w in zip((fa, fb), wins):
            ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
            ev0.record()
            for _ in range(iters):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            w.append(ev0.elapsed_time(ev1) / iters)
    return [(statistics.median(w), min(w), max(w)) for w in wins]


def run(tokens, hq, d, B, topk, s_kv=16384, iters=10, reps=5):
    dev = "cuda"
    torch.manual_seed(0)
    q = torch.randn(tokens, hq, d, dtype=torch.bfloat16, device=dev)
    k = torch.randn(s_kv, 1, d, dtype=torch.bfloat16, device=dev)
    v = torch.randn_like(k)
    dout = torch.randn_like(q)
    nb = -(-tokens // B)
    idx_b = torch.stack(
        [torch.randperm(s_kv, device=dev)[:topk] for _ in range(nb)]
    ).int().contiguous()
    idx_t = idx_b.repeat_interleave(B, 0)[:tokens].contiguous()
    scale = d ** (-0.5)
    lib = _ffa_lib.lib()

    def fwd(idx, qb):
        return _flex_flash_attn_forward_index(q, k, v, idx, scale, 0.0,
                                              q_block_size=qb)

    out, meta = fwd(idx_t, 1)
    out_b, meta_b = fwd(idx_b, B)
    rel = ((out_b.double() - out.double()).norm() / out.double().norm()).item()
    dlse = (meta_b.lse - meta.lse).abs().max().item()
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k, dtype=torch.float32)
    dv = torch.zeros_like(v, dtype=torch.float32)
    dpsum = _ffa_launch.bwd_dpsum(dout, out)

    def bwd(idx, qb):
        # accumulators are not re-zeroed between launches: the kernel's work
        # does not depend on their contents
        cls = (_ffa_lib.MagiFfaIndexBwdBlockArgs if qb > 1
               else _ffa_lib.MagiFfaIndexBwdArgs)
        a = cls(
            dout=ptr(dout), q=ptr(q), k=ptr(k), v=ptr(v), lse=ptr(meta.lse),
            dpsum=ptr(dpsum), indices_2d=ptr(idx),
            dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
            total_q=tokens, total_k=s_kv, max_topk=topk,
            hq=hq, hk=1, d=d, softmax_scale=scale, softcap=0.0,
            stream=current_stream_ptr(),
        )
        if qb > 1:
            a.q_block_size = qb
            check(lib.magi_ffa_bwd_index_block(a), "bwd_index_block")
        else:
            check(lib.magi_ffa_bwd_index(a), "bwd_index")

    print(f"tokens={tokens} hq={hq} d={d} B={B} topk={topk} s_kv={s_kv}  "
          f"out rel-L2 diff {rel:.2e}, lse max diff {dlse:.2e}")
    for name, fl, fn in (("fwd", 4.0, fwd), ("bwd", 10.0, bwd)):
        (b_ms, b_lo, b_hi), (t_ms, t_lo, t_hi) = _time_pair(
            lambda: fn(idx_b, B), lambda: fn(idx_t, 1), iters, reps)
        tf = fl * tokens * hq * topk * d / 1e9
        print(
            f"  {name} block     {b_ms:8.3f} ms [{b_lo:.3f}..{b_hi:.3f}] "
            f"{tf / b_ms:6.1f} TF/s\n"
            f"  {name} per-token {t_ms:8.3f} ms [{t_lo:.3f}..{t_hi:.3f}] "
            f"{tf / t_ms:6.1f} TF/s   per-token / block {t_ms / b_ms:.2f}x",
            flush=True,
        )


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    if args:
        run(*args)
    else:
        run(16384, 32, 128, 64, 2048)  # DiT-like block selection
        run(16384, 8, 128, 16, 2048)   # small GQA group (NSA-style)
        run(16384, 8, 128, 4, 2048)    # 32 rows: the 1-wave launch
        run(16384, 16, 128, 4, 2048)   # 64 rows: the 2-wave launch
        run(4096, 128, 128, 4, 2048)   # hq already fills the tiles
