"""The yardstick of tests/test_ffa_fp8_edges_gpu.py, checked without a GPU.

For every case and head dim of that file:
- the lse tolerance can see one key: ATOL_LSE <= 0.5 * p_min;
- an fp32 emulation of the kernel's rounding (P scaled to [0, 256], rounded to
  e4m3, normalised by the unrounded row sum, ranges merged by lse, sink folded
  last, out through bf16) stays inside the per-element envelope, has exact
  zeros on rows without a key, the oracle's -inf pattern, and meets the global
  rel-L2 criterion. If it did not, the derivation of the envelope would be
  wrong, not the kernel;
- the envelope is not slack: the emulation uses a real share of it."""
import math

import pytest
import torch

from tests import test_ffa_fp8_edges_gpu as E
from tests.util import assert_close_to_ref

ALL = [(n, d) for n in E.CASES for d in E.DIMS]


@pytest.mark.parametrize("name,d", ALL, ids=[f"{n}-d{d}" for n, d in ALL])
def test_emulation_inside_envelope(name, d):
    r = E.reference(name, d)
    assert E.ATOL_LSE <= 0.5 * r.p_min, (name, d, r.p_min)
    out, lse = E.emulate(r)
    fin = torch.isfinite(r.lse64)
    assert torch.equal(torch.isfinite(lse), fin)
    # the emulation's lse is plain fp32 torch, not the kernel's: held only to
    # the one-key cap, which no correct fp32 evaluation comes near
    assert E.lse_errors(lse, r) <= 0.5 * r.p_min
    ratio = E.out_ratio(out, r)
    print(f"    [{r.name}] emulation out_ratio={ratio:.3f} "
          f"p_min={r.p_min:.3e}")
    assert ratio <= 1.0
    assert torch.equal(out[~r.has_key], torch.zeros_like(out[~r.has_key]))
    assert_close_to_ref(out, r.o_hi.float(), r.o_lo.float(), r.name,
                        floor=1e-2)


def test_envelope_is_not_slack():
    """The bound is a worst case (every rounding at its limit, all of one
    sign), so rows with many keys sit well inside it; rows with few keys come
    close. Over the cases the emulation uses more than half of it: a kernel
    with twice the rounding error would leave it."""
    worst = max(E.out_ratio(E.emulate(E.reference(n, 64))[0],
                            E.reference(n, 64)) for n in E.CASES)
    assert 0.5 < worst <= 1.0, worst


def test_empty_case_has_no_key():
    """offset_ranges_t3: 263 rows on 131 keys, bi-causal allows nothing."""
    r = E.reference("offset_ranges_t3", 64)
    assert not r.mask.any() and r.p_min == math.inf
    assert not torch.isfinite(r.lse64).any()
    assert E.reference("offset_bicausal_band", 64).mask.any()


@pytest.mark.parametrize("name", ["gqa_4_2", "gqa_8_2"])
def test_wrong_head_reference_is_far_outside(name):
    r = E.reference(name, 64)
    hq, hk = r.case["hq"], r.case["hk"]
    assert [h // (hq // hk) for h in range(hq)] != [h % hk for h in range(hq)]
    _, lse_w, _, out_w, _ = E._fp64_softmax(
        r.q8.float(), r.k8.float(), r.v8.float(), r.mask, None, None,
        [h % hk for h in range(hq)])
    assert E.lse_errors(lse_w.permute(1, 0).float(), r) > 100 * E.ATOL_LSE
    assert E.out_ratio(out_w.permute(1, 0, 2).float(), r) > 10.0
