"""Timing probe for sparse_load in the dense forward (not a pytest test).

Per shape it times the forward launch alone (_ffa_launch.fwd into preallocated
out / lse; k_cum is built inside the call, as a caller pays for it), flag off
against flag on in one process, in two epilogue modes:
  direct  16-bit direct store (the q ranges of every table here are disjoint);
  merge   lock-guarded merge into an f32 out. The buffers are not reset
          between calls, so every call after the first merges into a live
          (out, lse): the same traffic for both variants.
Shapes (D = 128, bf16, hq = 32, 8192 q and k tokens): kb<K>_g<G>[_pack] is a
block-sparse merged table, q blocks of 64 tokens, each attending ROWS = 512
k rows as ROWS / K seeded k blocks of K rows (K = 16, 32, 64, 128), segments
in ascending k order; G = hq / hk (1 or 8), _pack = pack_gqa on in both
variants. Flag off is the segment-loop launch.
Per measurement: 2 warm-up calls of each variant, then `reps` rounds; a round
times one window of `iters` calls of each variant with device events, the
order alternating from round to round. Printed: median window and min..max
per variant, and on/off as the median of the per-round ratios with its
range. Before timing, flag-on out / lse are compared with flag-off (rel-L2
and max abs; not bit-equal by design).

  python tests/gpu_sparse_load_perf.py [shape ...]

The script sets no time limit of its own: give each call one, e.g.
`timeout -k 10 300 python tests/gpu_sparse_load_perf.py kb16_g1`."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional import _ffa_launch
from magi_attention.functional.flex_flash_attn import _get_locks, _merged_tables

D, T, HQ, QB, ROWS = 128, 8192, 32, 64, 512
SHAPES = {f"kb{kb}_g{g}{'_pack' if pack else ''}": (kb, g, pack)
          for g, pack in ((1, False), (8, False), (8, True))
          for kb in (16, 32, 64, 128)}


def tables(kb, dev):
    """(q_ranges, k_ranges, types, qk_starts) of the merged table"""
    g = torch.Generator().manual_seed(1)
    qr, kr = [], []
    for i in range(T // QB):
        for b in torch.randperm(T // kb, generator=g)[:ROWS // kb].sort().values.tolist():
            qr.append([i * QB, (i + 1) * QB])
            kr.append([b * kb, (b + 1) * kb])
    qr, kr = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (qr, kr))
    return _merged_tables(qr, kr, torch.zeros(len(qr), dtype=torch.int32, device=dev))


def run(name, reps=7, iters=100):
    kb, G, pack = SHAPES[name]
    hk, dev = HQ // G, "cuda"
    gen = torch.Generator().manual_seed(0)
    q, k, v = ((torch.randn(T, h, D, generator=gen) * 0.5).bfloat16().to(dev)
               for h in (HQ, hk, hk))
    qr, kr, tm, starts = tables(kb, dev)
    print(f"{name}: hq={HQ} hk={hk} pack_gqa={pack}; {T // QB} q blocks of {QB} "
          f"tokens x {ROWS // kb} k blocks of {kb} rows", flush=True)

    def make(sparse, direct):
        out = torch.zeros(T, HQ, D, device=dev,
                          dtype=torch.bfloat16 if direct else torch.float32)
        lse = torch.full((T, HQ), float("-inf"), device=dev)
        locks = None if direct else _get_locks(T, HQ, q.device)

        def fn():
            _ffa_launch.fwd(
                q, k, v, out, lse, qr, kr, tm, locks=locks, max_logits=None,
                qk_starts=starts, max_seqlen_q=QB, softmax_scale=D ** -0.5,
                softcap=0.0, disable_fwd_atomic_reduction=direct, sm_margin=0,
                deterministic=False, pack_gqa=pack, sparse_load=sparse)
        return fn, out, lse

    def window(fn):
        ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
        ev0.record()
        for _ in range(iters):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / iters * 1e3

    for direct in (True, False):
        made = {key: make(key == "on", direct) for key in ("off", "on")}
        for fn, _, _ in made.values():
            fn()
        torch.cuda.synchronize()
        (_, o0, l0), (_, o1, l1) = made["off"], made["on"]
        live = ~torch.isinf(l0)
        rel = ((o0.float() - o1.float()).norm() / o0.float().norm()).item()
        tag = f"  {'direct' if direct else 'merge '}"
        print(f"{tag} on vs off: out rel-L2 {rel:.3e}, lse max abs "
              f"{(l0 - l1)[live].abs().max().item():.3e}, -inf pattern equal "
              f"{torch.equal(torch.isinf(l0), torch.isinf(l1))}", flush=True)
        for fn, _, _ in made.values():
            fn()
        times = {key: [] for key in made}
        for r in range(reps):
            for key in (list(made) if r % 2 == 0 else list(made)[::-1]):
                times[key].append(window(made[key][0]))
        for key, ts in times.items():
            print(f"{tag} sparse {key:3s} {statistics.median(ts):10.1f} us "
                  f"[{min(ts):.1f}..{max(ts):.1f}]", flush=True)
        per_round = [b / a for a, b in zip(times["off"], times["on"])]
        print(f"{tag} on/off {statistics.median(per_round):.4f} (median of "
              f"per-round ratios, {min(per_round):.4f}..{max(per_round):.4f})",
              flush=True)


if __name__ == "__main__":
    for shape in sys.argv[1:] or list(SHAPES):
        run(shape)
