"""Timing probe for k_block_size on the index path (not a pytest test).

Each row is one K-block-granular selection served two ways in the same
process, both with the same q_block_size = B:
  kblock    k_block_size = Bk: lists of topk / Bk K block ids, the KBLOCK
            kernels (magi_ffa_fwd_index_kblock / magi_ffa_bwd_index_kblock);
  expanded  the baseline: the same lists expanded on the host to topk row ids
            (id*Bk + arange(Bk)), k_block_size = 1, which is what such a caller
            ran before (per-token kernels for B = 1, BLOCK kernels for B > 1).
Forward and backward are timed with device events: 3 warm-up calls of each way
at each shape, then `reps` rounds that alternate one window of `iters` calls of
either way; the median window, the min..max spread and the expanded / kblock
ratio are printed, with achieved TF/s on 4 (fwd) and 10 (bwd) *
tokens*hq*topk*d FLOPs. The forward call includes the out/lse fills of
_flex_flash_attn_forward_index and the backward call the row-wise dpsum
preprocess of _ffa_launch.bwd_index, the same on both sides. Before timing,
out and lse of the two ways are compared.

Measured on an MI355X (profiles/index_k_block.md; d 128, 16k tokens, 2048
rows; expanded / kblock, above 1 = kblock faster; windows spread <= 0.4 %, up
to 7 % on the sub-millisecond forwards):
  hq  (Bk, B)    fwd     bwd        hq  (Bk, B)    fwd     bwd
   8  (16, 1)    0.87x   0.97x      32  (16, 1)    0.92x   0.97x
   8  (64, 1)    0.87x   0.96x      32  (64, 1)    0.92x   0.96x
   8  (64, 16)   0.84x   1.03x      32  (64, 16)   0.86x   1.04x
   8  (128, 64)  0.84x   0.96x      32  (128, 64)  0.85x   1.03x
The forward loses at every shape; the backward is level.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

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


def run(tokens, hq, d, Bk, B, topk, s_kv=16384, iters=10, reps=5):
    dev = "cuda"
    torch.manual_seed(0)
    q = torch.randn(tokens, hq, d, dtype=torch.bfloat16, device=dev)
    k = torch.randn(s_kv, 1, d, dtype=torch.bfloat16, device=dev)
    v = torch.randn_like(k)
    dout = torch.randn_like(q)
    nl = -(-tokens // B)
    # topk / Bk distinct blocks per list
    idx_kb = torch.rand(nl, s_kv // Bk, device=dev).argsort(1)[
        :, :topk // Bk].int().contiguous()
    idx_ex = (idx_kb[:, :, None] * Bk + torch.arange(
        Bk, device=dev, dtype=torch.int32)).reshape(nl, topk).contiguous()
    scale = d ** (-0.5)
    ways = ((idx_kb, Bk), (idx_ex, 1))

    def fwd(idx, kb):
        return _flex_flash_attn_forward_index(
            q, k, v, idx, scale, 0.0, q_block_size=B, k_block_size=kb)

    (out_kb, meta_kb), (out, meta) = [fwd(*w) for w in ways]
    rel = ((out_kb.double() - out.double()).norm() / out.double().norm()).item()
    dlse = (meta_kb.lse - meta.lse).abs().max().item()
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k, dtype=torch.float32)
    dv = torch.zeros_like(v, dtype=torch.float32)

    def bwd(idx, kb):
        # accumulators are not re-zeroed between calls: the kernel's work
        # does not depend on their contents
        _ffa_launch.bwd_index(dout, q, k, v, out, meta.lse, idx, dq, dk, dv,
                              scale, 0.0, q_block_size=B, k_block_size=kb)

    print(f"tokens={tokens} hq={hq} d={d} Bk={Bk} B={B} topk={topk} "
          f"s_kv={s_kv}  out rel-L2 diff {rel:.2e}, lse max diff {dlse:.2e}")
    for name, fl, fn in (("fwd", 4.0, fwd), ("bwd", 10.0, bwd)):
        (b_ms, b_lo, b_hi), (t_ms, t_lo, t_hi) = _time_pair(
            lambda: fn(*ways[0]), lambda: fn(*ways[1]), iters, reps)
        tf = fl * tokens * hq * topk * d / 1e9
        print(
            f"  {name} kblock   {b_ms:8.3f} ms [{b_lo:.3f}..{b_hi:.3f}] "
            f"{tf / b_ms:6.1f} TF/s\n"
            f"  {name} expanded {t_ms:8.3f} ms [{t_lo:.3f}..{t_hi:.3f}] "
            f"{tf / t_ms:6.1f} TF/s   expanded / kblock {t_ms / b_ms:.2f}x",
            flush=True,
        )


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    if args:
        run(*args)
    else:
        for hq in (8, 32):
            for Bk, B in ((16, 1), (64, 1), (64, 16), (128, 64)):
                run(16384, hq, 128, Bk, B, 2048)
