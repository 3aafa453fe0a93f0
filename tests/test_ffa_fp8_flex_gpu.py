"""Dense fp8 forward through magi_ffa_fwd_fp8_flex: merged tables
(auto_range_merge), the direct bf16 store and softcap. Softcap and the direct
store are reached through flex_flash_attn_func; merged tables through
FlexFlashAttnFunc.apply, the autograd function it ends in, because
flex_flash_attn_func itself still refuses fp8 + auto_range_merge. Oracle, envelope and check_parity are those of
tests/test_ffa_fp8_edges_gpu.py; the in-kernel carry across the k segments of
a q range is the running-max rescale its envelope already covers.

Softcap: tanhf adds error to the lse, so ATOL_LSE is not assumed. Measured on
an MI355X against the fp64 softcapped oracle over the three cases and both
head dims (profiles/fp8_dense_flex.md): largest |lse - oracle| 2.77e-6
(bicausal_192x224, d 64), largest |max_logits - oracle| 5.01e-6
(merged_segments, d 64); each tolerance is four times that, the lse one
checked against 0.5 * p_min of every case and the max_logits one against
1e-3."""
import copy
import functools

import pytest
import torch

from oracle import make_attn_mask, ref_attn, ref_attn_with_grads
from tests import test_ffa_fp8_edges_gpu as E
from tests.util import assert_close_to_ref

CAP = 2.0
ATOL_LSE_CAP = 1.11e-5         # 4 x 2.77e-6
ATOL_MAX_LOGITS_CAP = 2.0e-5   # 4 x 5.01e-6

# two unique q ranges, out of table order. [60, 100) has six k segments: 33
# rows from an unaligned start, 11 rows, an empty one and one each of types
# 1, 2, 3; [0, 60) has two, and its causal one leaves rows 0..9 to the other.
# The segments of a q range are k-disjoint, as the oracle's mask is a union.
MERGED = dict(
    tq=100, tk=200, hq=4, hk=2,
    qr=[[60, 100], [0, 60], [60, 100], [60, 100], [60, 100], [0, 60],
        [60, 100], [60, 100]],
    kr=[[100, 133], [0, 50], [5, 16], [70, 70], [150, 200], [133, 150],
        [16, 56], [56, 100]],
    ty=[0, 1, 0, 0, 1, 0, 2, 3],
)


@functools.lru_cache(maxsize=None)
def ref(name: str, d: int) -> E.Ref:
    """E.reference, which also knows the geometry above"""
    if name != "merged_segments":
        return E.reference(name, d)
    E.CASES[name] = MERGED
    try:
        return E.reference.__wrapped__(name, d)
    finally:
        del E.CASES[name]


@functools.lru_cache(maxsize=None)
def softcap_ref(name: str, d: int) -> E.Ref:
    """ref(name, d) with s -> CAP * tanh(s / CAP): fp64 lse, out, envelope and
    p_min as E.reference derives them; oracle.ref_attn(softcap=) must agree"""
    b = ref(name, d)
    r = copy.copy(b)
    r.name = b.name + "-cap"
    hq, hk = b.case["hq"], b.case["hk"]
    vd = b.v8.double()[:, [h // (hq // hk) for h in range(hq)]].permute(1, 0, 2)
    dead = ~b.mask.unsqueeze(0)
    r.s = (CAP * torch.tanh(b.s / CAP)).masked_fill(dead, float("-inf"))
    lse = torch.logsumexp(r.s, dim=-1)
    p = torch.nan_to_num(torch.exp(r.s - lse.unsqueeze(-1)), nan=0.0)
    r.lse64 = lse.permute(1, 0).contiguous()
    r.out64 = torch.matmul(p, vd).permute(1, 0, 2).contiguous()
    o_hi, lse_hi = ref_attn(b.q8.float(), b.k8.float(), b.v8.float(), b.mask,
                            softcap=CAP)
    fin = torch.isfinite(r.lse64)
    torch.testing.assert_close(lse_hi[fin].double(), r.lse64[fin], atol=2e-6,
                               rtol=0)
    torch.testing.assert_close(o_hi.double(), r.out64, atol=1e-6, rtol=0)
    env = 1.01 * (2.0 ** -4 * torch.matmul(p, vd.abs()) + 2.0 ** -18
                  * torch.matmul(b.mask.double().unsqueeze(0), vd.abs()))
    r.bound = (env.permute(1, 0, 2) + 2.0 ** -8 * r.out64.abs()
               + 1e-6).contiguous()
    r.p_min = p[~dead.expand_as(p)].min().item()
    return r


def check_softcap(out, lse, r: E.Ref):
    """check_parity's a-c with the softcap lse tolerance"""
    out, lse = out.detach().cpu().float(), lse.detach().cpu().float()
    fin = torch.isfinite(r.lse64)
    assert ATOL_LSE_CAP <= 0.5 * r.p_min, (r.name, r.p_min)
    assert torch.equal(torch.isfinite(lse), fin) and not torch.isnan(lse).any()
    e_lse, ratio = E.lse_errors(lse, r), E.out_ratio(out, r)
    print(f"    [fp8flex:{r.name}] lse_err={e_lse:.3e} out_ratio={ratio:.3f} "
          f"p_min={r.p_min:.3e}")
    assert e_lse <= ATOL_LSE_CAP, f"{r.name}: lse error {e_lse:.3e}"
    assert ratio <= 1.0, f"{r.name}: {ratio:.3f} x the e4m3 envelope"
    assert torch.equal(out[~r.has_key], torch.zeros_like(out[~r.has_key]))


def max_logits_error(ml, r: E.Ref) -> float:
    assert ml is not None and ml.shape == (r.case["hq"],)
    err = (ml.cpu().double() - r.s.amax(dim=(-1, -2))).abs().max().item()
    print(f"    [fp8flex:{r.name}] max_logits_err={err:.3e}")
    return err


def merged_apply(q, k, v, qr, kr, tm, *, softcap=0.0,
                 disable_fwd_atomic_reduction=False, return_max_logits=False):
    """FlexFlashAttnFunc with auto_range_merge=True, the autograd function
    flex_flash_attn_func ends in; returns (out, lse, max_logits)"""
    from magi_attention.functional.flex_flash_attn import FlexFlashAttnFunc

    return FlexFlashAttnFunc.apply(
        q, k, v, None, "sh", qr, kr, tm, None, softcap, False, 0,
        disable_fwd_atomic_reduction, False, None, None, True, False, False,
        False, False, False, False, return_max_logits)


def run(r: E.Ref, merge=False, **kw):
    """(out, lse, max_logits) of the case; out is bf16 either way"""
    if not merge:
        out, meta = E._run(r, **kw)
        return out, meta.lse, meta.max_logits
    out, lse, ml = merged_apply(*E._dev(r), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    return out, lse, ml


pytestmark = [pytest.mark.gpu, E.requires_gpu, pytest.mark.parametrize("d", E.DIMS)]


@pytest.mark.parametrize("name", ["accumulate", "overlap_q", "empty_k",
                                  "short_and_long", "max_logits",
                                  "merged_segments"])
def test_merged_tables(name, d):
    r = ref(name, d)
    out, lse, ml = run(r, True, return_max_logits=name == "max_logits")
    E.check_parity(out, lse, r, ":merge")
    if name == "max_logits":
        assert max_logits_error(ml, r) <= E.ATOL_MAX_LOGITS


@pytest.mark.parametrize("name,merge", [
    ("causal_unaligned", False), ("causal_tq_gt_tk", False),
    ("offset_ranges_t3", False), ("short_and_long", False),
    ("sink_sh", False), ("gqa_8_2", False), ("accumulate", True)])
def test_direct_bf16_store(name, merge, d):
    """no lock, no f32 out, no cast: out is bf16; rows in no range keep
    out == 0 and lse == -inf (the sink's lse with a sink), which check_parity
    holds them to"""
    r = ref(name, d)
    kw = dict(sink=r.sink.cuda(), sink_layout=r.layout) if r.layout else {}
    out, lse, _ = run(r, merge, disable_fwd_atomic_reduction=True, **kw)
    E.check_parity(out, lse, r, ":direct")


@pytest.mark.parametrize("name", ["causal_unaligned", "bicausal_192x224",
                                  "merged_segments"])
def test_softcap(name, d):
    r = softcap_ref(name, d)
    out, lse, ml = run(r, name == "merged_segments", softcap=CAP,
                       return_max_logits=True)
    check_softcap(out, lse, r)
    assert ATOL_MAX_LOGITS_CAP <= 1e-3
    assert max_logits_error(ml, r) <= ATOL_MAX_LOGITS_CAP


def test_softcap_merged_backward(d):
    """fp8 forward with softcap over a merged table, bf16-upcast backward;
    ratios and floors of test_fp8_fwd_bwd_oracle_parity"""
    t, hq, hk = 256, 4, 2
    g = torch.Generator().manual_seed(21)
    q8, k8, v8 = ((torch.randn(t, h, d, generator=g) * 0.5).to(E.FP8)
                  for h in (hq, hk, hk))
    dout = (torch.randn(t, hq, d, generator=g) * 0.5).bfloat16()
    qr, kr, ty = ([[0, 128], [128, 256], [128, 256]],
                  [[0, 128], [0, 128], [128, 256]], [1, 0, 1])
    q, k, v = (x.cuda().requires_grad_(True) for x in (q8, k8, v8))
    i32 = dict(dtype=torch.int32, device="cuda")
    out, _, _ = merged_apply(q, k, v, torch.tensor(qr, **i32),
                             torch.tensor(kr, **i32), torch.tensor(ty, **i32),
                             softcap=CAP)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    args = (q8.float(), k8.float(), v8.float(),
            make_attn_mask(t, t, qr, kr, ty), dout.float())
    hi = ref_attn_with_grads(*args, softcap=CAP)
    lo = ref_attn_with_grads(*args, softcap=CAP, high_precision=False,
                             p_dtype=torch.bfloat16)
    got = (out, None, q.grad, k.grad, v.grad)
    for i, what, ratio, floor in ((0, "out", 8.0, 3.5e-2), (2, "dq", 4.5, 9e-2),
                                  (3, "dk", 4.5, 9e-2), (4, "dv", 4.5, 9e-2)):
        assert_close_to_ref(got[i].detach().cpu().float(), hi[i].float(),
                            lo[i].float(), f"fp8flex:{what}", ratio=ratio,
                            floor=floor)

