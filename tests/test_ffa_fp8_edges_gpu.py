"""Edge-shape parity of the dense fp8 (e4m3) forward, csrc/ffa_fwd_fp8.hip.

Inputs are randn * 0.5 from a seeded CPU generator cast to float8_e4m3fn; the
oracle (oracle.ref_attn over make_attn_mask) runs in fp64 on the dequantised
values, so the quantisation is the input and not part of the error. Every
parity case goes through check_parity, which asserts four things.

a. lse, tight. The finite / -inf pattern equals the oracle's and finite values
   are within ATOL_LSE of it. The lse never sees the rounded P, and S is an
   fp32 accumulation of exact fp8 products, so its only error is that
   accumulation, the hardware exp2 / log2 (at magnitude 8..16 because of the
   MAX_OFFSET shift) and the summation order. ATOL_LSE is four times the
   largest lse error measured over all cases of this file on an MI355X
   (profiles/fp8_dense_edges.md). The tolerance must be able to see ONE key:
   dropping or adding a key of probability p moves the lse by at least p, so
   the helper computes p_min, the smallest fp64 probability of any allowed key
   of the case, and asserts ATOL_LSE <= 0.5 * p_min.

b. out, per element, against a derived envelope. The kernel normalises by the
   unrounded fp32 row sum and rounds only P, scaled to [0, 256], to e4m3: a
   relative error of at most 2^-4 in the normal range, and an absolute error of
   at most 2^-10 in the subnormal range on a scale where the row maximum is
   2^8. The running-max rescale and the merge across ranges are convex
   combinations, so the bound survives both. With p the fp64 softmax over all
   allowed keys of the row (sink logits in the denominator where given):

     |out - ref| <= 1.01 * (2^-4 * sum_j p_j |v_j,c|
                            + 2^-18 * sum_{j allowed} |v_j,c|)
                    + 2^-8 * |ref| + 1e-6

   2^-8 covers the bf16 output cast; 1.01 and 1e-6 cover fp32 accumulation.
   No element may exceed it. tests/test_ffa_fp8_edges_cpu.py checks without a
   GPU that an fp32 emulation of the kernel's rounding stays inside it.

c. Rows with no allowed key have out exactly 0.

d. The global rel-L2 criterion of tests/test_ffa_fp8_gpu.py
   (assert_close_to_ref, floor 1e-2) holds as well.

max_logits is held to ATOL_MAX_LOGITS, four times its measured error, never
above 1e-3: a missing ln 2 or a missed head is orders of magnitude larger."""
import functools
import math

import pytest
import torch

from oracle import make_attn_mask, ref_attn
from tests.util import assert_close_to_ref

# measured on an MI355X over every case below (profiles/fp8_dense_edges.md):
# largest |lse - oracle| 8.06e-6 (causal_tq_gt_tk, d 128), largest
# |max_logits - oracle| 1.53e-5 (d 64); each tolerance is four times that
ATOL_LSE = 3.2e-5
ATOL_MAX_LOGITS = 6.1e-5

FP8 = torch.float8_e4m3fn
DIMS = (64, 128)

_OVERLAP_Q = dict(
    tq=256, tk=512, hq=2, hk=2,
    qr=[[0, 256], [64, 192], [0, 128]],
    kr=[[0, 128], [128, 384], [384, 512]],
    ty=[1, 0, 2],
)

# name -> geometry (the head dim is the second parameter of every test)
CASES = {
    "causal_unaligned": dict(tq=173, tk=211, hq=2, hk=1,
                             qr=[[0, 173]], kr=[[0, 211]], ty=[1]),
    # first 38 rows have no key: n_hi < n_lo for their waves
    "causal_tq_gt_tk": dict(tq=211, tk=173, hq=2, hk=1,
                            qr=[[0, 211]], kr=[[0, 173]], ty=[1]),
    "invcausal_160x96": dict(tq=160, tk=96, hq=2, hk=2,
                             qr=[[0, 160]], kr=[[0, 96]], ty=[2]),
    "bicausal_192x224": dict(tq=192, tk=224, hq=3, hk=1,
                             qr=[[0, 192]], kr=[[0, 224]], ty=[3]),
    # two live rows per head, one of them a single key with P exactly 256:
    # the global rel-L2 check then rests on ONE rounding per head, and with
    # one head a correct emulation misses its 1e-2 floor on that single draw
    # (1.16e-2 at d 64). Four heads give it four draws to average.
    "tiny_5x2": dict(tq=5, tk=2, hq=4, hk=2,
                     qr=[[0, 5]], kr=[[0, 2]], ty=[1]),
    # the second K tile has one live key; loads clamp to ke - 1
    "tk33_full": dict(tq=40, tk=33, hq=2, hk=2,
                      qr=[[0, 40]], kr=[[0, 33]], ty=[0]),
    "tk33_causal": dict(tq=40, tk=33, hq=2, hk=2,
                        qr=[[0, 40]], kr=[[0, 33]], ty=[1]),
    # q start 37: the first block straddles two lock slots, the last wave is
    # partial, b_lo is unaligned for types 2 and 3; rows outside stay empty
    **{
        f"offset_ranges_t{t}": dict(tq=320, tk=192, hq=2, hk=2,
                                    qr=[[37, 300]], kr=[[19, 150]], ty=[t])
        for t in (0, 1, 2, 3)
    },
    # with 263 rows on 131 keys type 3 above allows nothing at all; this one
    # keeps a 28-wide band alive at the same unaligned starts
    "offset_bicausal_band": dict(tq=320, tk=192, hq=2, hk=2,
                                 qr=[[37, 140]], kr=[[19, 150]], ty=[3]),
    "overlap_q": _OVERLAP_Q,
    # the first range's grid has blocks that return early
    "short_and_long": dict(tq=330, tk=330, hq=2, hk=2,
                           qr=[[0, 40], [40, 330]], kr=[[0, 40], [40, 330]],
                           ty=[1, 1]),
    # range 0 has ks == ke: rows 0..59 stay empty, 60..119 live off range 1
    "empty_k": dict(tq=200, tk=96, hq=2, hk=1,
                    qr=[[0, 120], [60, 200]], kr=[[40, 40], [0, 96]],
                    ty=[1, 0]),
    "gqa_4_2": dict(tq=96, tk=96, hq=4, hk=2,
                    qr=[[0, 96]], kr=[[0, 96]], ty=[1]),
    "gqa_8_2": dict(tq=96, tk=96, hq=8, hk=2,
                    qr=[[0, 96]], kr=[[0, 96]], ty=[1]),
    # one launch per K part into the same (out, lse); oracle over the union
    "accumulate": dict(tq=173, tk=211, hq=2, hk=2,
                       qr=[[0, 173], [0, 173]], kr=[[0, 83], [83, 211]],
                       ty=[0, 1]),
    "max_logits": dict(tq=320, tk=320, hq=4, hk=2,
                       qr=[[0, 192], [192, 320]], kr=[[0, 256], [64, 320]],
                       ty=[1, 3]),
    # rows 190..255 are in no q range: sink only
    "sink_sh": dict(tq=256, tk=256, hq=4, hk=2,
                    qr=[[0, 100], [100, 190]], kr=[[0, 150], [33, 256]],
                    ty=[1, 0], sink="sh"),
    "sink_ssh": dict(tq=256, tk=256, hq=4, hk=2,
                     qr=[[0, 100], [100, 190]], kr=[[0, 150], [33, 256]],
                     ty=[1, 0], sink="ssh"),
}
S_SINK = 3

PLAIN = [
    n for n in CASES
    if n not in ("accumulate", "max_logits", "sink_sh", "sink_ssh",
                 "gqa_4_2", "gqa_8_2")
]


class Ref:
    """Inputs and fp64 reference of one (case, d); computed once, read-only."""


def _fp64_softmax(qq, kk, vv, mask, sink, layout, k_head_of):
    """fp64 lse, p over the real keys, out; heads of K/V picked by k_head_of"""
    tq, hq, d = qq.shape
    qd = qq.double().permute(1, 0, 2)
    kd = kk.double()[:, k_head_of].permute(1, 0, 2)
    vd = vv.double()[:, k_head_of].permute(1, 0, 2)
    s = torch.matmul(qd, kd.transpose(-1, -2)) * d ** -0.5
    s = s.masked_fill(~mask.unsqueeze(0), float("-inf"))
    if sink is None:
        lse = torch.logsumexp(s, dim=-1)
    else:
        sf = sink.double()
        extra = (sf.permute(1, 0).unsqueeze(1).expand(hq, tq, sf.shape[0])
                 if layout == "sh" else sf.permute(2, 0, 1))
        lse = torch.logsumexp(torch.cat([s, extra], dim=-1), dim=-1)
    p = torch.nan_to_num(torch.exp(s - lse.unsqueeze(-1)), nan=0.0)
    return s, lse, p, torch.matmul(p, vd), vd


@functools.lru_cache(maxsize=None)
def reference(name: str, d: int) -> Ref:
    c = CASES[name]
    tq, tk, hq, hk = c["tq"], c["tk"], c["hq"], c["hk"]
    g = torch.Generator().manual_seed(11)
    r = Ref()
    r.name, r.d, r.case = f"{name}-d{d}", d, c
    r.q8 = (torch.randn(tq, hq, d, generator=g) * 0.5).to(FP8)
    r.k8 = (torch.randn(tk, hk, d, generator=g) * 0.5).to(FP8)
    r.v8 = (torch.randn(tk, hk, d, generator=g) * 0.5).to(FP8)
    r.layout = c.get("sink")
    r.sink = None
    if r.layout:
        shape = (S_SINK, hq) if r.layout == "sh" else (tq, S_SINK, hq)
        r.sink = (torch.randn(*shape, generator=g) * 2.0).float()
    r.mask = make_attn_mask(tq, tk, c["qr"], c["kr"], c["ty"])
    qq, kk, vv = r.q8.float(), r.k8.float(), r.v8.float()
    kw = dict(sink=r.sink, sink_layout=r.layout) if r.layout else {}
    r.o_hi, r.lse_hi = ref_attn(qq, kk, vv, r.mask, **kw)
    r.o_lo, _ = ref_attn(qq, kk, vv, r.mask, high_precision=False,
                         p_dtype=FP8, **kw)

    # the same oracle kept in fp64, with the softmax itself: p gives the
    # envelope and p_min, and ref_attn's fp32 results must be its rounding
    heads = [h // (hq // hk) for h in range(hq)]
    r.s, lse, p, out, vd = _fp64_softmax(qq, kk, vv, r.mask, r.sink,
                                         r.layout, heads)
    r.lse64 = lse.permute(1, 0).contiguous()
    r.out64 = out.permute(1, 0, 2).contiguous()
    fin = torch.isfinite(r.lse64)
    assert torch.equal(fin, torch.isfinite(r.lse_hi))
    torch.testing.assert_close(r.lse_hi[fin].double(), r.lse64[fin],
                               atol=2e-6, rtol=0)
    torch.testing.assert_close(r.o_hi.double(), r.out64, atol=1e-6, rtol=0)
    mk = r.mask.double().unsqueeze(0)
    env = 1.01 * (2.0 ** -4 * torch.matmul(p, vd.abs())
                  + 2.0 ** -18 * torch.matmul(mk, vd.abs()))
    r.bound = (env.permute(1, 0, 2) + 2.0 ** -8 * r.out64.abs()
               + 1e-6).contiguous()
    r.has_key = r.mask.any(dim=1)                       # [tq]
    allowed = r.mask.unsqueeze(0).expand_as(p)
    r.p_min = p[allowed].min().item() if r.mask.any() else math.inf
    return r


def lse_errors(lse, r: Ref):
    fin = torch.isfinite(r.lse64)
    if not fin.any():
        return 0.0
    return (lse.double()[fin] - r.lse64[fin]).abs().max().item()


def out_ratio(out, r: Ref):
    """largest |out - ref| / bound over all elements"""
    return ((out.double() - r.out64).abs() / r.bound).max().item()


def check_parity(out, lse, r: Ref, what: str = ""):
    """a-d of the module docstring; prints each figure before it asserts"""
    out, lse = out.detach().cpu().float(), lse.detach().cpu().float()
    tag = f"fp8edge:{r.name}{what}"
    fin = torch.isfinite(r.lse64)
    e_lse = lse_errors(lse, r) if torch.equal(torch.isfinite(lse), fin) \
        else math.inf
    ratio = out_ratio(out, r)
    print(f"    [{tag}] lse_err={e_lse:.3e} out_ratio={ratio:.3f} "
          f"p_min={r.p_min:.3e}")
    # a. lse
    assert ATOL_LSE <= 0.5 * r.p_min, (
        f"{tag}: atol_lse {ATOL_LSE:.1e} cannot see one key "
        f"(p_min {r.p_min:.3e})")
    assert torch.equal(torch.isfinite(lse), fin), f"{tag}: lse -inf pattern"
    assert not torch.isnan(lse).any(), f"{tag}: NaN lse"
    assert torch.equal(lse[~fin], r.lse64[~fin].float()), f"{tag}: empty lse"
    assert e_lse <= ATOL_LSE, f"{tag}: lse error {e_lse:.3e} > {ATOL_LSE:.1e}"
    # b. out inside the envelope, element by element
    assert ratio <= 1.0, (
        f"{tag}: |out - ref| reaches {ratio:.3f} x the e4m3 envelope")
    # c. rows with no allowed key
    empty = ~r.has_key
    assert torch.equal(out[empty], torch.zeros_like(out[empty])), (
        f"{tag}: a row with no allowed key has non-zero out")
    # d. the criterion of tests/test_ffa_fp8_gpu.py
    assert_close_to_ref(out, r.o_hi.float(), r.o_lo.float(), f"{tag}:out",
                        floor=1e-2)


def emulate(r: Ref):
    """fp32 restatement of the kernel's rounding: per range, P = exp(s - max)
    scaled to [0, 256] and rounded to e4m3, normalised by the UNROUNDED row
    sum; ranges merged by their lse; sink folded last. Returns (out, lse) as
    flex_flash_attn_func does: out through bf16."""
    from oracle.ref_attn import merge_out_lse

    c = r.case
    tq, tk, hq, hk = c["tq"], c["tk"], c["hq"], c["hk"]
    heads = [h // (hq // hk) for h in range(hq)]
    qf = r.q8.float().permute(1, 0, 2)
    kf = r.k8.float()[:, heads].permute(1, 0, 2)
    vf = r.v8.float()[:, heads].permute(1, 0, 2)
    s_all = torch.matmul(qf, kf.transpose(-1, -2)) * r.d ** -0.5
    outs, lses = [], []
    for qr, kr, ty in zip(c["qr"], c["kr"], c["ty"]):
        m = make_attn_mask(tq, tk, [qr], [kr], [ty])
        s = s_all.masked_fill(~m.unsqueeze(0), float("-inf"))
        mx = s.amax(dim=-1, keepdim=True)
        mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
        pr = torch.exp(s - mx) * 256.0
        l_ = pr.sum(dim=-1, keepdim=True)
        o = torch.matmul(pr.to(FP8).float(), vf)
        o = torch.where(l_ > 0, o / l_, torch.zeros_like(o))
        lse = torch.where(l_ > 0, mx + torch.log(l_) - math.log(256.0),
                          torch.full_like(l_, float("-inf"))).squeeze(-1)
        outs.append(o.permute(1, 0, 2))
        lses.append(lse.permute(1, 0))
    out, lse = merge_out_lse(outs, lses)
    if r.sink is not None:
        sf = r.sink.double()
        lse_s = torch.logsumexp(sf, dim=0 if r.layout == "sh" else 1)
        tot = torch.logaddexp(lse, lse_s.expand_as(lse))
        out = out * torch.nan_to_num(torch.exp(lse - tot), nan=0.0).unsqueeze(-1)
        lse = tot
    return out.float().bfloat16().float(), lse.float()


# ───────────────────────── GPU tests ─────────────────────────

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


def _dev(r: Ref):
    c = r.case
    i32 = dict(dtype=torch.int32, device="cuda")
    return (r.q8.cuda(), r.k8.cuda(), r.v8.cuda(),
            torch.tensor(c["qr"], **i32), torch.tensor(c["kr"], **i32),
            torch.tensor(c["ty"], **i32))


def _run(r: Ref, **kw):
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, qr, kr, tm = _dev(r)
    out, meta = flex_flash_attn_func(q, k, v, qr, kr, tm, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and meta.lse.dtype == torch.float32
    return out, meta


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", PLAIN)
def test_fp8_edge_parity(name, d):
    r = reference(name, d)
    out, meta = _run(r)
    check_parity(out, meta.lse, r)


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", ["gqa_4_2", "gqa_8_2"])
def test_fp8_edge_gqa(name, d):
    """1 < hk < hq, forward only: kh = h / gqa and kh = h % hk differ. First
    shown on the CPU: the wrong-head reference is far outside every bound."""
    r = reference(name, d)
    hq, hk = r.case["hq"], r.case["hk"]
    wrong = [h % hk for h in range(hq)]
    _, lse_w, _, out_w, _ = _fp64_softmax(
        r.q8.float(), r.k8.float(), r.v8.float(), r.mask, None, None, wrong)
    lse_w = lse_w.permute(1, 0).float()
    out_w = out_w.permute(1, 0, 2).float()
    assert lse_errors(lse_w, r) > 100 * ATOL_LSE
    assert out_ratio(out_w, r) > 10.0
    denom = r.out64.norm()
    budget = max(3.0 * ((r.o_lo.double() - r.out64).norm() / denom).item(),
                 1e-2)
    assert ((out_w.double() - r.out64).norm() / denom).item() > 3 * budget

    out, meta = _run(r)
    check_parity(out, meta.lse, r)


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
def test_fp8_edge_accumulate(d):
    """Two launches, K split at 83, into one caller-owned fp32 (out, lse), as
    the CP runtime does: lse_prev is finite for every row of the second."""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
    )

    r = reference("accumulate", d)
    c = r.case
    q, k, v, qr, kr, tm = _dev(r)
    out = torch.zeros(c["tq"], c["hq"], d, dtype=torch.float32, device="cuda")
    lse = torch.full((c["tq"], c["hq"]), float("-inf"), dtype=torch.float32,
                     device="cuda")
    for i in range(2):
        o2, meta = _flex_flash_attn_forward(
            q=q, k=k, v=v, sink=None, sink_layout="sh", out=out, lse=lse,
            q_ranges=qr[i:i + 1], k_ranges=kr[i:i + 1],
            attn_type_map=tm[i:i + 1], softmax_scale=d ** -0.5, softcap=0.0,
            out_type=None, disable_fwd_atomic_reduction=False,
            deterministic=False, sm_margin=0,
        )
        assert o2 is out and meta.lse is lse
    torch.cuda.synchronize()
    check_parity(out, lse, r)


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
def test_fp8_edge_deterministic(d):
    """deterministic=True with three overlapping ranges: one launch per
    q-disjoint group. Bitwise repeatable, and as exact as the default mode."""
    r = reference("overlap_q", d)
    o1, m1 = _run(r, deterministic=True)
    o2, m2 = _run(r, deterministic=True)
    assert torch.equal(o1, o2)
    assert torch.equal(m1.lse, m2.lse)
    check_parity(o1, m1.lse, r, ":det")


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
def test_fp8_edge_max_logits(d):
    r = reference("max_logits", d)
    out, meta = _run(r, return_max_logits=True)
    check_parity(out, meta.lse, r)
    ml = meta.max_logits
    assert ml is not None and ml.shape == (r.case["hq"],)
    assert ml.dtype == torch.float32
    ref = r.s.amax(dim=(-1, -2))          # fp64, masked, scaled; [hq]
    err = (ml.cpu().double() - ref).abs().max().item()
    print(f"    [fp8edge:{r.name}] max_logits_err={err:.3e}")
    assert ATOL_MAX_LOGITS <= 1e-3
    assert err <= ATOL_MAX_LOGITS, f"max_logits error {err:.3e}"


@gpu
@requires_gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("layout", ["sh", "ssh"])
def test_fp8_edge_sink(layout, d):
    """Sink logits folded after the fp8 merge, forward only; rows in no q
    range get lse = lse_sink and out exactly 0."""
    r = reference(f"sink_{layout}", d)
    out, meta = _run(r, sink=r.sink.cuda(), sink_layout=layout)
    assert torch.isfinite(meta.lse).all()
    check_parity(out, meta.lse, r)


@gpu
@requires_gpu
def test_fp8_rejects_auto_range_merge():
    """fp8 + auto_range_merge is refused before the attention launch."""
    from magi_attention.functional import flex_flash_attn_func

    r = reference("overlap_q", 64)
    q, k, v, qr, kr, tm = _dev(r)
    with pytest.raises(AssertionError, match=r"fp8 \+ auto_range_merge"):
        flex_flash_attn_func(q, k, v, qr, kr, tm, auto_range_merge=True)
    torch.cuda.synchronize()
