"""Timing probe for swap_ab (the split-k forward) (not a pytest test).

Per shape it times the forward launch alone (_ffa_launch.fwd into preallocated
out / lse; no zero-fill, no cast), swap_ab off against on in one process. Off
is the default launch, which this flag leaves untouched: the baseline. Two
epilogue modes:
  direct  16-bit direct store (the q ranges of every table here are disjoint);
  merge   lock-guarded merge into an f32 out. The buffers are not reset
          between calls, so every call after the first merges into a live
          (out, lse): the same traffic for both variants.
Shapes (D = 128, bf16, 16384 q and k tokens, hq = hk = H, MHA):
  bs<B>_h<H>   block-sparse: q blocks of B tokens, each attending a seeded
               quarter (32) of the 128 k blocks of 128 rows, as merged tables
               (one q range per block, its k blocks as segments: what
               auto_range_merge builds);
  causal16k_h<H>  one causal range of 16384 tokens: what the flag costs where
               it is not meant.
QT is the launcher's own choice (2) unless MAGI_FWD_SPLITK_QT is set. Per measurement: 2 warm-up calls of each variant,
then `reps` rounds; a round times one window of `iters` calls of each variant
with device events, the order alternating from round to round. Printed: median
window and min..max per variant, the ratio of the medians and the median of the
per-round ratios with its range. Before timing, swap_ab-on out / lse are
compared with off (rel-L2 and max abs; not bit-equal by design).

  python tests/gpu_swap_ab_perf.py [shape ...]

The script sets no time limit of its own: give each call one, e.g.
`timeout -k 10 300 python tests/gpu_swap_ab_perf.py bs16_h8`."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional import _ffa_launch
from magi_attention.functional.flex_flash_attn import _get_locks, _merged_tables

D, T, KB = 128, 16384, 128
NK = T // KB // 4
SHAPES = {f"bs{b}_h{h}": (b, h) for h in (8, 32) for b in (16, 32, 64, 128, 256)}
SHAPES.update({f"causal16k_h{h}": (0, h) for h in (8,)})


def tables(block, dev):
    """(q_ranges, k_ranges, types, qk_starts, max_seqlen_q)"""
    if not block:
        r = torch.tensor([[0, T]], dtype=torch.int32, device=dev)
        return r, r.clone(), torch.ones(1, dtype=torch.int32, device=dev), None, T
    g = torch.Generator().manual_seed(1)
    qr, kr = [], []
    for i in range(T // block):
        for kb in torch.randperm(T // KB, generator=g)[:NK].sort().values.tolist():
            qr.append([i * block, (i + 1) * block])
            kr.append([kb * KB, (kb + 1) * KB])
    qr, kr = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (qr, kr))
    tm = torch.zeros(len(qr), dtype=torch.int32, device=dev)
    return _merged_tables(qr, kr, tm) + (block,)


def run(name, reps=7):
    block, H = SHAPES[name]
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    q, k, v = ((torch.randn(T, H, D, generator=gen) * 0.5).bfloat16().to(dev)
               for _ in range(3))
    qr, kr, tm, starts, msq = tables(block, dev)
    qt = int(os.environ.get("MAGI_FWD_SPLITK_QT", 0)) or 2
    print(f"{name}: hq=hk={H} q ranges={qr.shape[0]} of {msq} tokens; "
          f"workgroups: off {qr.shape[0] * H * -(-msq // 256)} (8 waves), "
          f"on {qr.shape[0] * H * -(-msq // (32 * qt))} (4 waves, QT={qt})",
          flush=True)
    iters = 10 if not block else 50

    def make(on, direct):
        out = torch.zeros(T, H, D, device=dev,
                          dtype=torch.bfloat16 if direct else torch.float32)
        lse = torch.full((T, H), float("-inf"), device=dev)
        locks = None if direct else _get_locks(T, H, q.device)

        def fn():
            _ffa_launch.fwd(
                q, k, v, out, lse, qr, kr, tm, locks=locks, max_logits=None,
                qk_starts=starts, max_seqlen_q=msq, softmax_scale=D ** -0.5,
                softcap=0.0, disable_fwd_atomic_reduction=direct, sm_margin=0,
                deterministic=False, swap_ab=on)
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
        print(f"  {'direct' if direct else 'merge '} on vs off: out rel-L2 "
              f"{rel:.3e}, lse max abs {(l0 - l1)[live].abs().max().item():.3e}, "
              f"-inf pattern equal {torch.equal(torch.isinf(l0), torch.isinf(l1))}",
              flush=True)
        for fn, _, _ in made.values():
            fn()
        times = {key: [] for key in made}
        for r in range(reps):
            for key in (list(made) if r % 2 == 0 else list(made)[::-1]):
                times[key].append(window(made[key][0]))
        tag = f"  {'direct' if direct else 'merge '}"
        for key, ts in times.items():
            print(f"{tag} swap_ab {key:3s} {statistics.median(ts):10.1f} us "
                  f"[{min(ts):.1f}..{max(ts):.1f}]", flush=True)
        per_round = [b / a for a, b in zip(times["off"], times["on"])]
        ratio = statistics.median(times["on"]) / statistics.median(times["off"])
        print(f"{tag} on/off {ratio:.4f} (medians)  "
              f"{statistics.median(per_round):.4f} (median of per-round ratios, "
              f"{min(per_round):.4f}..{max(per_round):.4f})", flush=True)


if __name__ == "__main__":
    for shape in sys.argv[1:] or list(SHAPES):
        run(shape)
