"""Inputs and oracles shared by tests/test_ffa_fp16_cpu.py and
tests/test_ffa_fp16_gpu.py (no test in here; CPU only).

Inputs are randn * 0.5 from a seeded CPU generator, rounded to the grid k/64
and clamped to |x| <= 3.96875 = 254/64: at most 8 significant bits, so every
value is exact in bf16 and in fp16. Both dtypes therefore see identical
numbers, the quantisation of the inputs is no part of any error, and one fp64
oracle serves both. scale_qk multiplies q and k by a power of two, which keeps
that property (8 -> grid k/8, |x| <= 31.75).

Oracles per (case, d, ...), computed once and never modified:
  hi    fp64 on the exact values (not rounded to a 16-bit dtype)
  lo16  fp32, fp16 inputs, P rounded to fp16 before PV - the budget reference
        of every fp16 parity check (tests/util.assert_close_to_ref)
  lobf  fp32, bf16 inputs, P rounded to bf16 - what the bf16 kernels get
Each is the tuple of oracle.ref_attn_with_grads: (out, lse, dq, dk, dv[,
dsink])."""
import functools

import torch

from oracle import make_attn_mask, ref_attn_with_grads
from tests.test_ffa_fp8_edges_gpu import CASES as EDGE_CASES

FP16, BF16 = torch.float16, torch.bfloat16
S_SINK = 3

# the geometries of test 1 of tests/test_ffa_fp16_gpu.py, by their names in
# tests/test_ffa_fp8_edges_gpu.py CASES
PARITY_CASES = (
    "causal_unaligned", "causal_tq_gt_tk", "bicausal_192x224",
    "offset_ranges_t2", "overlap_q", "empty_k", "gqa_8_2",
)
# the two cases the fp16-vs-bf16 error ratio is taken on, at d 128
RATIO_CASES = ("causal_unaligned", "overlap_q")

CASES = dict(EDGE_CASES)
CASES.update(
    # D=192 and the padded d=160
    causal_200=dict(tq=200, tk=200, hq=2, hk=2,
                    qr=[[0, 200]], kr=[[0, 200]], ty=[1]),
    # q and k times 8: logit std about 16 after the softmax scale
    range_96=dict(tq=96, tk=96, hq=2, hk=2,
                  qr=[[0, 96]], kr=[[0, 96]], ty=[1]),
    # auto_range_merge: two unique q ranges with three k segments each, the
    # rows listed out of order so the merge has to sort them
    merge_3seg=dict(tq=230, tk=384, hq=2, hk=2,
                    qr=[[0, 100], [100, 230], [0, 100],
                        [100, 230], [0, 100], [100, 230]],
                    kr=[[200, 300], [10, 90], [0, 64],
                        [250, 384], [64, 200], [90, 250]],
                    ty=[1, 0, 0, 1, 0, 2]),
)


def grid_randn(shape, g, scale=1):
    x = (torch.randn(*shape, generator=g) * 32.0).round().clamp(-254, 254)
    return x * (scale / 64.0)


class Ref:
    """Inputs and oracles of one key; read-only."""


@functools.lru_cache(maxsize=None)
def reference(name, d, scale_qk=1, softcap=0.0) -> Ref:
    c = CASES[name]
    tq, tk, hq, hk = c["tq"], c["tk"], c["hq"], c["hk"]
    g = torch.Generator().manual_seed(16)
    r = Ref()
    r.name, r.d, r.case, r.softcap = f"{name}-d{d}", d, c, softcap
    r.q = grid_randn((tq, hq, d), g, scale_qk)
    r.k = grid_randn((tk, hk, d), g, scale_qk)
    r.v = grid_randn((tk, hk, d), g)
    r.dout = grid_randn((tq, hq, d), g)
    for t in (r.q, r.k, r.v, r.dout):
        assert torch.equal(t.to(FP16).float(), t)
        assert torch.equal(t.to(BF16).float(), t)
    r.layout = c.get("sink")
    r.sink = None
    kw = dict(softcap=softcap)
    if r.layout:
        shape = (S_SINK, hq) if r.layout == "sh" else (tq, S_SINK, hq)
        r.sink = (torch.randn(*shape, generator=g) * 2.0).float()
        kw.update(sink=r.sink, sink_layout=r.layout)
    r.mask = make_attn_mask(tq, tk, c["qr"], c["kr"], c["ty"])

    def oracle(dtype, **okw):
        return ref_attn_with_grads(
            r.q.to(dtype), r.k.to(dtype), r.v.to(dtype), r.mask,
            r.dout.to(dtype), **kw, **okw,
        )

    r.hi = oracle(torch.float64)
    r.lo16 = oracle(FP16, high_precision=False, p_dtype=FP16)
    r.lobf = oracle(BF16, high_precision=False, p_dtype=BF16)
    r.dead = torch.isinf(r.hi[1]) & (r.hi[1] < 0)       # [tq, hq]
    return r


def rel_l2(x, ref) -> float:
    x, ref = x.double(), ref.double()
    return ((x - ref).norm() / ref.norm().clamp_min(1e-300)).item()
