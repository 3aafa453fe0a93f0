"""Timing probe for the direct 16-bit dQ/dK/dV stores (not a pytest test).

Times the whole backward as autograd runs it - out.backward(dout) after one
forward with retain_graph, so the zero-fills of the gradient buffers, the
dpsum preprocess, the dq and dkv passes and the final casts are all inside -
with the flags off and with the flags on, in one process. Per shape: 3
warm-up calls of both variants, then `reps` rounds; each round times one
window of `iters` calls of "off" and one of "on" with device events, and the
order of the two alternates from round to round. Printed: the median window
and min..max of each, the ratio of the medians, the median of the per-round
ratios, and the bytes the direct path no longer moves (counted from shapes).
The first gradients of the two variants are compared bit for bit.

  python tests/gpu_bwd_direct_perf.py [shape ...]    shapes: see SHAPES

The script sets no time limit of its own: run one shape per process and give
each its own, e.g. `timeout -k 10 150 python tests/gpu_bwd_direct_perf.py
dense64k`. All windows come from one process, so the spread it prints is
between rounds of one run, not between runs.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional import flex_flash_attn_func

D = 128
# name -> (total tokens, hq = hk, documents (all causal, equal length), iters)
SHAPES = {
    "dense16k": (16384, 32, 1, 10),
    "dense64k": (65536, 32, 1, 3),
    # the varlen shape of bench.py --full: 8 causal documents of 2k, 16 heads
    "varlen8x2k": (16384, 16, 8, 40),
    # the same documents, twice as many, at the dense shapes' 32 heads
    "varlen16x2k": (32768, 32, 16, 10),
}


def saved_bytes(n, h):
    """Traffic per backward that exists only on the f32 atomic path, for the
    three gradients of n x h x D elements each: the zero-fill writes 4 B
    where the direct path's writes 2 B (2 saved); the atomic read-modify-write
    moves at least 4 + 4 B at the L2 where the store writes 2 B (6 saved);
    the cast pass reads 4 B and writes 2 B (6 saved)."""
    return 3 * n * h * D * (2 + 6 + 6)


def run(name, reps=7):
    n, h, docs, iters = SHAPES[name]
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    q, k, v, dout = (
        (torch.randn(n, h, D, generator=g) * 0.5).bfloat16().to(dev)
        for _ in range(4)
    )
    L = n // docs
    rs = [[i * L, (i + 1) * L] for i in range(docs)]
    qr = torch.tensor(rs, dtype=torch.int32, device=dev)
    kr = qr.clone()
    tm = torch.ones(docs, dtype=torch.int32, device=dev)

    def variant(direct):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, _ = flex_flash_attn_func(
            *leaves, qr, kr, tm, max_seqlen_q=L, max_seqlen_k=L,
            disable_fwd_atomic_reduction=direct,
            disable_bwd_dkv_atomic_reduction=direct,
        )

        def bwd():
            out.backward(dout, retain_graph=True)
            grads = [t.grad for t in leaves]
            for t in leaves:
                t.grad = None
            return grads

        return bwd

    fns = {"off": variant(False), "on": variant(True)}
    first = {}
    for _ in range(3):
        for key, fn in fns.items():
            first[key] = fn()
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for a, b in zip(first["off"], first["on"]))
    del first

    def window(fn):
        ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
        ev0.record()
        for _ in range(iters):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / iters

    times = {"off": [], "on": []}
    for r in range(reps):
        for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
            times[key].append(window(fns[key]))
    med = {key: statistics.median(ts) for key, ts in times.items()}
    per_round = [b / a for a, b in zip(times["off"], times["on"])]
    gb = saved_bytes(n, h) / 1e9
    print(
        f"{name}: tokens={n} hq=hk={h} d={D} docs={docs} x {L} causal, "
        f"{reps} rounds of {iters} calls, gradients bit-equal: {equal}\n"
        f"  off {med['off']:9.3f} ms [{min(times['off']):.3f}.."
        f"{max(times['off']):.3f}]\n"
        f"  on  {med['on']:9.3f} ms [{min(times['on']):.3f}.."
        f"{max(times['on']):.3f}]\n"
        f"  on/off {med['on'] / med['off']:.4f} (medians)  "
        f"{statistics.median(per_round):.4f} (median of per-round ratios, "
        f"{min(per_round):.4f}..{max(per_round):.4f})\n"
        f"  saved {med['off'] - med['on']:.3f} ms; bytes not moved "
        f"{gb:.2f} GB",
        flush=True,
    )


if __name__ == "__main__":
    for shape in sys.argv[1:] or list(SHAPES):
        run(shape)
