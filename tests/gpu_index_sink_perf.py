"""Timing probe for the index-attention forward with an attention sink and
max_logits (not a pytest test).

Per shape (DiT ratio-128 and ratio-32, bf16 and fp8) it times the off path
and, where the checkout has them, sink "sh" / "ssh", max_logits, both, and the
alternative route (off + a separate magi_ffa_sink_postprocess launch on the
bf16 out). Device events, 5 warm-up calls, then 7 windows of 40 calls per
mode, the modes taken round-robin twice; prints one JSON line per (shape,
mode): median, min and max window in ms per call.

usage: gpu_index_sink_perf.py [TREE [TAG]]   TREE = checkout whose package is
timed (default: this one), so an older checkout can be timed by the same
script in alternation with this one.
"""
import inspect
import json
import os
import sys

here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = sys.argv[1] if len(sys.argv) > 1 else here
tag = sys.argv[2] if len(sys.argv) > 2 else "this"
sys.path.insert(0, os.path.abspath(tree))

import torch  # noqa: E402

from magi_attention.functional import flex_flash_attn as F  # noqa: E402
from magi_attention.utils import build_index_attn_indices  # noqa: E402

fwd = F._flex_flash_attn_forward_index
HAS = "sink" in inspect.signature(fwd).parameters
ROUNDS, ITERS = 7, 40
FP8 = torch.float8_e4m3fn


def time_fn(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / ITERS)
    return res


def run(name, tokens, hq, d, s_kv, topk, fp8):
    torch.manual_seed(0)
    dev = "cuda"
    q = torch.randn(tokens, hq, d, device=dev)
    k = torch.randn(s_kv, 1, d, device=dev)
    v = torch.randn(s_kv, 1, d, device=dev)
    if fp8:
        q, k, v = [(t * 0.5).to(FP8) for t in (q, k, v)]
    else:
        q, k, v = [t.bfloat16() for t in (q, k, v)]
    idx = build_index_attn_indices(1, 1, tokens, s_kv, topk, topk,
                                   device=dev).view(tokens, topk)
    scale = d ** -0.5
    modes = {"off": lambda: fwd(q, k, v, idx, scale, 0.0)}
    if HAS:
        sh = torch.randn(4, hq, device=dev) * 2 + 2
        ssh = torch.randn(tokens, 4, hq, device=dev) * 2 + 2
        ml = torch.full((hq,), float("-inf"), device=dev)

        def post():
            o, m = fwd(q, k, v, idx, scale, 0.0)
            F._apply_sink_postprocess(o, m.lse, sh, "sh", tokens, hq, d)

        modes.update({
            "sink_sh": lambda: fwd(q, k, v, idx, scale, 0.0, sink=sh),
            "sink_ssh": lambda: fwd(q, k, v, idx, scale, 0.0, sink=ssh,
                                    sink_layout="ssh"),
            "max_logits": lambda: fwd(q, k, v, idx, scale, 0.0,
                                      max_logits=ml),
            "sink_sh+ml": lambda: fwd(q, k, v, idx, scale, 0.0, sink=sh,
                                      max_logits=ml),
            "off+postprocess": post,
        })
    # alternate the modes round-robin twice so drift hits all alike
    out = {}
    for rep in range(2):
        for mname, fn in modes.items():
            out.setdefault(mname, []).extend(time_fn(fn))
    for mname, r in out.items():
        r = sorted(r)
        rec = dict(tag=tag, case=name, mode=mname, median_ms=r[len(r) // 2],
                   min_ms=r[0], max_ms=r[-1], n=len(r))
        print(json.dumps(rec), flush=True)


for fp8 in (False, True):
    p = "fp8" if fp8 else "bf16"
    run(f"{p}-dit-r128", 4096, 128, 128, 8192, 2048, fp8)
    run(f"{p}-r32", 8192, 32, 128, 16384, 1024, fp8)
