"""The softcap cases of tests/test_ffa_dense_paths_gpu.py can tell a kernel
that applies softcap from one that does not. No GPU needed: this is a
condition on the inputs, checked with the oracle alone.

For the inputs of every softcap case two wrong "implementations" are
evaluated in fp64:

  * softcap ignored altogether (the oracle at softcap=0): each of out, dq, dk
    and dv must miss the assert_close_to_ref budget of the GPU test by at
    least 3x;
  * forward softcapped, but the tanh derivative (1 - tanh^2) left out of dS
    in the backward: dq must miss its budget by at least 3x.

The dense softcap tests that came first ran at s / cap of about 0.015, where
tanh is the identity to within the budget and both of these pass. If a table
ever fails here, change its cap or scale, not the factor."""
import pytest
import torch

from oracle import ref_attn_with_grads
from tests.test_ffa_dense_paths_gpu import (
    SOFTCAP_CASES,
    SOFTCAP_D192,
    softcap_inputs,
)
from tests.util import FLOOR, MISMATCH_RATIO

POWER = 3.0

CASES = [c + (d,) for c in SOFTCAP_CASES for d in (64, 128)]
CASES.append(SOFTCAP_D192 + (192,))


def _miss(wrong, hi, lo):
    """rel-L2 error of `wrong` over the budget assert_close_to_ref grants."""
    hi, lo, wrong = hi.double(), lo.double(), wrong.double()
    denom = hi.norm().clamp_min(1e-8)
    budget = max(MISMATCH_RATIO * ((lo - hi).norm() / denom).item(), FLOOR)
    return ((wrong - hi).norm() / denom).item() / budget


def _dq_by_hand(q, k, v, dout, mask, scale, cap, keep_dtanh):
    """dq from the oracle's own steps in fp64: s = cap * tanh(q k^T scale /
    cap), p = softmax(s), dS = p * (dP - rowsum(dP * p)), then the chain
    through the cap: dS * (1 - tanh^2) when keep_dtanh, dS alone when not."""
    hq, hk = q.shape[1], k.shape[1]
    g = hq // hk
    qf = q.double().permute(1, 0, 2)
    kf = k.double().repeat_interleave(g, dim=1).permute(1, 0, 2)
    vf = v.double().repeat_interleave(g, dim=1).permute(1, 0, 2)
    do = dout.double().permute(1, 0, 2)
    th = torch.tanh(torch.matmul(qf, kf.transpose(-1, -2)) * scale / cap)
    s = torch.where(mask.unsqueeze(0), cap * th, torch.full_like(th, -torch.inf))
    p = torch.nan_to_num(torch.exp(s - torch.logsumexp(s, -1, keepdim=True)))
    dp = torch.matmul(do, vf.transpose(-1, -2))
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    if keep_dtanh:
        ds = ds * (1 - th * th)
    return (torch.matmul(ds, kf) * scale).permute(1, 0, 2)


@pytest.mark.parametrize(
    "case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-h{c[3]}{c[4]}-d{c[5]}"
)
def test_softcap_cases_tell_softcap_apart(case):
    table, tname, regime, hq, hk, d = case
    (q, k, v, dout, _, _, _), mask, scale, cap, _ = softcap_inputs(
        table, tname, regime, hq, hk, d
    )
    kw = dict(softmax_scale=scale)
    hi = ref_attn_with_grads(q, k, v, mask, dout, softcap=cap, **kw)
    lo = ref_attn_with_grads(
        q, k, v, mask, dout, softcap=cap, high_precision=False,
        p_dtype=torch.bfloat16, **kw,
    )
    uncapped = ref_attn_with_grads(q, k, v, mask, dout, softcap=0.0, **kw)
    for i, n in ((0, "out"), (2, "dq"), (3, "dk"), (4, "dv")):
        miss = _miss(uncapped[i], hi[i], lo[i])
        print(f"    [no softcap:{n}] misses the budget by {miss:.1f}x")
        assert miss >= POWER, (
            f"{n}: a kernel without softcap misses the budget by only "
            f"{miss:.2f}x on these inputs"
        )

    sc = d ** -0.5 if scale is None else scale
    # the hand-built dq is the oracle's when the derivative is kept
    # (hi holds the fp64 gradient rounded to bf16)
    same = _dq_by_hand(q, k, v, dout, mask, sc, cap, True)
    torch.testing.assert_close(
        same.to(torch.bfloat16), hi[2], atol=0, rtol=2 ** -7
    )
    flat = _dq_by_hand(q, k, v, dout, mask, sc, cap, False)
    miss = _miss(flat, hi[2], lo[2])
    print(f"    [no (1 - tanh^2):dq] misses the budget by {miss:.1f}x")
    assert miss >= POWER, (
        f"dq: a backward without (1 - tanh^2) misses the budget by only "
        f"{miss:.2f}x on these inputs"
    )
