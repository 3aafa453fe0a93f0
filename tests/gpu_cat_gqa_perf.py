"""Timing probe for cat_gqa in the dense backward (not a pytest test).

Per shape and per store mode (f32 atomic dK/dV, and the direct 16-bit store
where the variant allows it) it times, cat off against cat on in one process:
  dkv    the dK/dV pass(es) alone - the fused kernel, or dV then dK, whichever
         the host layer picks for the shape - launched over one preprocessed
         argument struct (no zero-fill, no dq pass);
  bwd    the whole _flex_flash_attn_backward call: zero-fills, the dpsum
         preprocess, the dq pass and the dK/dV pass(es).
Per measurement: 2 warm-up calls of each variant, then `reps` rounds; a round
times one window of `iters` calls of each variant with device events, and the
order of the variants alternates from round to round. Printed: the median
window and min..max of each variant, the ratio of the medians and the median
of the per-round ratios with its range, and the dK/dV workgroup count of each
variant. Before timing, the cat-on gradients are compared with the cat-off
ones (rel-L2; the sums are reordered, so not bit for bit).

  python tests/gpu_cat_gqa_perf.py [--no-cat] [shape ...]   shapes: see SHAPES

--no-cat times the cat-off variants only and never names cat_gqa, so the same
file also runs over a tree that has no such argument: the figures to hold this
tree's cat-off times against.

The script sets no time limit of its own: run one shape per process and give
each its own, e.g. `timeout -k 10 300 python tests/gpu_cat_gqa_perf.py cfg5`.
All windows come from one process, so the spread it prints is between rounds
of one run, not between runs.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from magi_attention import env
from magi_attention.functional import _ffa_launch
from magi_attention.functional.flex_flash_attn import (
    _flex_flash_attn_backward,
    _flex_flash_attn_forward,
)

D = 128
# name -> (total tokens, hq, hk, documents (all causal, equal length),
#          iters of a dkv window, iters of a whole-backward window)
SHAPES = {
    # BASELINE config 5: 128k causal, GQA 64:8
    "cfg5": (131072, 64, 8, 1, 1, 1),
    "dense16k_32_8": (16384, 32, 8, 1, 10, 6),
    "dense16k_32_4": (16384, 32, 4, 1, 10, 6),
    # 8 causal documents of 2k: cat_gqa leaves 8 x hk x 8 workgroups of 256
    # k rows, fewer than the chip's 256 CUs
    "varlen8x2k_32_8": (16384, 32, 8, 8, 40, 20),
}


def workgroups(L, docs, heads):
    """dK/dV grid of one pass: k blocks x head extent x ranges"""
    knobs_bigseq = int(os.environ.get("MAGI_BWD_BIGSEQ", 1024))
    span = 32 * (8 if L >= knobs_bigseq else 4)
    return -(-L // span) * heads * docs


def run(name, with_cat, reps=5):
    n, hq, hk, docs, it_dkv, it_bwd = SHAPES[name]
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    q, k, v, dout = (
        (torch.randn(n, h, D, generator=g) * 0.5).bfloat16().to(dev)
        for h in (hq, hk, hk, hq)
    )
    L = n // docs
    rs = [[i * L, (i + 1) * L] for i in range(docs)]
    qr = torch.tensor(rs, dtype=torch.int32, device=dev)
    kr = qr.clone()
    tm = torch.ones(docs, dtype=torch.int32, device=dev)
    scale = D ** -0.5
    out, meta = _flex_flash_attn_forward(
        q=q, k=k, v=v, sink=None, sink_layout="sh", out=None, lse=None,
        q_ranges=qr, k_ranges=kr, attn_type_map=tm, softmax_scale=scale,
        softcap=0.0, out_type=None, disable_fwd_atomic_reduction=False,
        deterministic=False, sm_margin=0, max_seqlen_q=L,
    )
    out, lse = out.to(torch.bfloat16), meta.lse
    split = env.is_bwd_split_dkv(L, D)
    print(f"{name}: tokens={n} hq={hq} hk={hk} d={D} docs={docs} x {L} causal,"
          f" dK/dV {'split (dV, dK)' if split else 'fused'}; workgroups per "
          f"pass: cat off {workgroups(L, docs, hq)}, cat on "
          f"{workgroups(L, docs, hk)}", flush=True)

    def cat_kw(cat):
        return {"cat_gqa": cat} if with_cat else {}

    def whole(cat, direct):
        def fn():
            return _flex_flash_attn_backward(
                dout=dout, q=q, k=k, v=v, sink=None, sink_layout="sh",
                out=out, lse=lse, dq=None, dk=None, dv=None, dsink=None,
                q_ranges=qr, k_ranges=kr, attn_type_map=tm,
                softmax_scale=scale, softcap=0.0, dq_type=None, dk_type=None,
                dv_type=None, disable_bwd_dkv_atomic_reduction=direct,
                deterministic=False, sm_margin=0, max_seqlen_k=L,
                **cat_kw(cat),
            )[:3]
        return fn

    def dkv_only(cat, direct):
        gdt = torch.bfloat16 if direct else torch.float32
        dq = torch.zeros_like(q, dtype=torch.float32)
        dk, dv = (torch.zeros_like(k, dtype=gdt) for _ in range(2))
        dpsum = torch.empty(n, hq, dtype=torch.float32, device=dev)
        args = _ffa_launch.bwd_args(
            dout, out, dpsum, q=q, k=k, v=v, lse=lse, dq=dq, dk=dk, dv=dv,
            q_ranges=qr, k_ranges=kr, attn_type_map=tm, max_seqlen_k=L,
            softmax_scale=scale, softcap=0.0, **cat_kw(cat),
        )
        _ffa_launch.bwd_preprocess(args)
        _, e_dkv, e_dv, e_dk = _ffa_launch._bwd_entries(args)
        entries = (e_dv, e_dk) if split else (e_dkv,)
        keep = (args, dq, dk, dv, dpsum)

        def fn():
            for e in entries:
                _ffa_launch.check(e(keep[0]), "dkv")
        return fn

    def measure(what, make, iters, direct):
        cats = (False, True) if with_cat else (False,)
        fns = {("on" if c else "off"): make(c, direct) for c in cats}
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()

        def window(fn):
            ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
            ev0.record()
            for _ in range(iters):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            return ev0.elapsed_time(ev1) / iters

        times = {key: [] for key in fns}
        for r in range(reps):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            for key in order:
                times[key].append(window(fns[key]))
        tag = f"  {what:4s} {'direct' if direct else 'f32   '}"
        for key, ts in times.items():
            print(f"{tag} cat {key:3s} {statistics.median(ts):10.3f} ms "
                  f"[{min(ts):.3f}..{max(ts):.3f}]", flush=True)
        if with_cat:
            per_round = [b / a for a, b in zip(times["off"], times["on"])]
            print(f"{tag} on/off "
                  f"{statistics.median(times['on']) / statistics.median(times['off']):.4f}"
                  f" (medians)  {statistics.median(per_round):.4f} (median of "
                  f"per-round ratios, {min(per_round):.4f}..{max(per_round):.4f})",
                  flush=True)

    if with_cat:
        a, b = whole(False, False)(), whole(True, False)()
        torch.cuda.synchronize()
        for x, y, nm in zip(a, b, ("dq", "dk", "dv")):
            rel = ((x - y).norm() / x.norm().clamp_min(1e-30)).item()
            print(f"  cat on vs off {nm}: rel-L2 {rel:.3e}", flush=True)
        del a, b
    for direct in ((False, True) if with_cat else (False,)):
        # without cat_gqa the direct store is refused under GQA: the cat-off
        # column of the direct rows is the f32 fallback the flag gives there
        if direct:
            measure("dkv", lambda c, d: dkv_only(c, d and c), it_dkv, True)
        else:
            measure("dkv", dkv_only, it_dkv, False)
        measure("bwd", whole, it_bwd, direct)


if __name__ == "__main__":
    argv = sys.argv[1:]
    no_cat = "--no-cat" in argv
    shapes = [a for a in argv if a != "--no-cat"]
    for shape in shapes or list(SHAPES):
        run(shape, not no_cat)
