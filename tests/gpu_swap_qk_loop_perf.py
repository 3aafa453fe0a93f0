"""Timing probe for swap_bwd_qk_loop in the dense backward (not a pytest test).

Per shape it times the whole backward step, _flex_flash_attn_backward (table
merge where there is one, preprocess, then the two passes or the one-pass
kernel), flag off against flag on in one process. out and lse come from the
default forward, once. D = 128, bf16, 16384 q and k tokens.
Shapes: kb<K>_g<G> is a block-sparse table under auto_range_merge, q blocks of
128 rows, each attending 1024 k rows as 1024 / K seeded k blocks of K rows
(K = 16, 32, 64, 128), hq = 8, hk = 8 / G; causal16k is one causal range, hq =
hk = 8; varlen8x2k is eight causal documents of 2048 tokens, hq = hk = 16
(bench.py's varlen shape).
Per shape: 3 warm-up calls of each variant, then `reps` calls of each,
alternating, each between device events; ms as mean [min, max]. Before timing
the gradients with the flag on are compared with the flag off (rel-L2).

  python tests/gpu_swap_qk_loop_perf.py [shape ...]

The script sets no time limit of its own: give each call one, e.g.
`timeout -k 10 300 python tests/gpu_swap_qk_loop_perf.py kb16_g1`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional.flex_flash_attn import (
    _flex_flash_attn_backward, _flex_flash_attn_forward)

D, T, QB, ROWS = 128, 16384, 128, 1024
SHAPES = {f"kb{kb}_g{g}": ("sparse", kb, 8, 8 // g)
          for g in (1, 4) for kb in (16, 32, 64, 128)}
SHAPES["causal16k"] = ("causal", T, 8, 8)
SHAPES["varlen8x2k"] = ("causal", 2048, 16, 16)


def tables(kind, n, dev):
    """(q_ranges, k_ranges, types) of the flat table"""
    if kind == "causal":  # documents of n tokens
        qr = kr = [[s, s + n] for s in range(0, T, n)]
        ty = [1] * len(qr)
    else:
        g = torch.Generator().manual_seed(1)
        qr, kr = [], []
        for i in range(T // QB):
            for b in torch.randperm(T // n, generator=g)[:ROWS // n].sort().values.tolist():
                qr.append([i * QB, (i + 1) * QB])
                kr.append([b * n, (b + 1) * n])
        ty = [0] * len(qr)
    return [torch.tensor(x, dtype=torch.int32, device=dev) for x in (qr, kr, ty)]


def run(name, reps=10):
    kind, n, hq, hk = SHAPES[name]
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    q, k, v, dout = ((torch.randn(T, h, D, generator=gen) * 0.5).bfloat16().to(dev)
                     for h in (hq, hk, hk, hq))
    qr, kr, tm = tables(kind, n, dev)
    merge = kind == "sparse"
    common = dict(q=q, k=k, v=v, sink=None, sink_layout="sh", softcap=0.0,
                  softmax_scale=D ** -0.5, deterministic=False, sm_margin=0)
    if merge:
        from magi_attention.functional.flex_flash_attn import _merged_tables
        fq, fk, ft, starts = _merged_tables(qr, kr, tm)
    else:
        fq, fk, ft, starts = qr, kr, tm, None
    out, meta = _flex_flash_attn_forward(
        out=None, lse=None, q_ranges=fq, k_ranges=fk, attn_type_map=ft,
        out_type=None, disable_fwd_atomic_reduction=False, qk_starts=starts,
        **common)
    print(f"{name}: hq={hq} hk={hk} table entries={qr.shape[0]} "
          f"auto_range_merge={merge}", flush=True)

    def step(swap):
        return _flex_flash_attn_backward(
            dout=dout, out=out, lse=meta.lse, dq=None, dk=None, dv=None,
            dsink=None, q_ranges=qr, k_ranges=kr, attn_type_map=tm,
            dq_type=None, dk_type=None, dv_type=None,
            disable_bwd_dkv_atomic_reduction=False, max_seqlen_k=n,
            auto_range_merge=merge, swap_bwd_qk_loop=swap, **common)[:3]

    def timed(swap):
        ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
        ev0.record()
        step(swap)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    on, off = step(True), step(False)
    torch.cuda.synchronize()
    for a, b, what in zip(on, off, ("dq", "dk", "dv")):
        print(f"  {what} on vs off rel-L2 "
              f"{((a - b).norm() / b.norm()).item():.3e}", flush=True)
    del on, off
    for _ in range(3):
        timed(True), timed(False)
    times = {True: [], False: []}
    for r in range(reps):
        for swap in ((True, False) if r % 2 == 0 else (False, True)):
            times[swap].append(timed(swap))
    mean = {s: sum(ts) / len(ts) for s, ts in times.items()}
    for s, ts in times.items():
        print(f"  step {'on ' if s else 'off'} {mean[s]:8.2f} ms "
              f"[{min(ts):.2f}, {max(ts):.2f}]", flush=True)
    print(f"  on/off {mean[True] / mean[False]:.3f}", flush=True)


if __name__ == "__main__":
    for shape in sys.argv[1:] or list(SHAPES):
        run(shape)
