"""Timing probe for pack_gqa in the dense forward (not a pytest test).

Per shape it times the forward launch alone (_ffa_launch.fwd into preallocated
out / lse; no zero-fill, no cast), pack off against pack on in one process, in
two epilogue modes:
  direct  16-bit direct store (the q ranges of every table here are disjoint);
  merge   lock-guarded merge into an f32 out. The buffers are not reset
          between calls, so every call after the first merges into a live
          (out, lse): the same traffic for both variants.
Shapes (D = 128, bf16, 8192 q and k tokens):
  bs<B>_g<G>   block-sparse: q blocks of B tokens, each attending 4 seeded
               k blocks of 128 rows, as merged tables (one q range per block,
               its k blocks as segments: what auto_range_merge builds);
  causal8k_g<G>  one causal range of 8192 tokens.
G = hq / hk with hq = 32. Per measurement: 2 warm-up calls of each variant,
then `reps` rounds; a round times one window of `iters` calls of each variant
with device events, the order alternating from round to round. Printed: median
window and min..max per variant, the ratio of the medians and the median of the
per-round ratios with its range, the workgroup counts and the wave count the
launcher takes. Before timing, pack-on out / lse are compared with pack-off
(rel-L2 and max abs; not bit-equal by design).

  python tests/gpu_pack_gqa_perf.py [shape ...]

The script sets no time limit of its own: give each call one, e.g.
`timeout -k 10 300 python tests/gpu_pack_gqa_perf.py bs16_g8`."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention.functional import _ffa_launch
from magi_attention.functional.flex_flash_attn import _get_locks, _merged_tables

D, T, HQ, KB, NK = 128, 8192, 32, 128, 4
SHAPES = {f"bs{b}_g{g}": (b, g) for g in (4, 8) for b in (16, 32, 64, 128)}
SHAPES.update({f"causal8k_g{g}": (0, g) for g in (4, 8)})


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
    block, G = SHAPES[name]
    hk, dev = HQ // G, "cuda"
    gen = torch.Generator().manual_seed(0)
    q, k, v = ((torch.randn(T, h, D, generator=gen) * 0.5).bfloat16().to(dev)
               for h in (HQ, hk, hk))
    qr, kr, tm, starts, msq = tables(block, dev)
    rows = msq * G
    waves = 4 if rows <= 128 else 8
    print(f"{name}: hq={HQ} hk={hk} q ranges={qr.shape[0]} of {msq} tokens; "
          f"workgroups: pack off {qr.shape[0] * HQ * -(-msq // 256)} (8 waves), "
          f"pack on {qr.shape[0] * hk * -(-rows // (32 * waves))} ({waves} waves)",
          flush=True)
    iters = 20 if not block else 200

    def make(pack, direct):
        out = torch.zeros(T, HQ, D, device=dev,
                          dtype=torch.bfloat16 if direct else torch.float32)
        lse = torch.full((T, HQ), float("-inf"), device=dev)
        locks = None if direct else _get_locks(T, HQ, q.device)

        def fn():
            _ffa_launch.fwd(
                q, k, v, out, lse, qr, kr, tm, locks=locks, max_logits=None,
                qk_starts=starts, max_seqlen_q=msq, softmax_scale=D ** -0.5,
                softcap=0.0, disable_fwd_atomic_reduction=direct, sm_margin=0,
                deterministic=False, pack_gqa=pack)
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
        print(f"  {'direct' if direct else 'merge '} pack on vs off: out rel-L2 "
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
            print(f"{tag} pack {key:3s} {statistics.median(ts):10.1f} us "
                  f"[{min(ts):.1f}..{max(ts):.1f}]", flush=True)
        per_round = [b / a for a, b in zip(times["off"], times["on"])]
        ratio = statistics.median(times["on"]) / statistics.median(times["off"])
        print(f"{tag} on/off {ratio:.4f} (medians)  "
              f"{statistics.median(per_round):.4f} (median of per-round ratios, "
              f"{min(per_round):.4f}..{max(per_round):.4f})", flush=True)


if __name__ == "__main__":
    for shape in sys.argv[1:] or list(SHAPES):
        run(shape)
