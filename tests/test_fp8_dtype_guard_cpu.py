"""The dense forward picks its kernel from q.dtype alone, so q, k and v must
share a dtype: bf16 q with fp8 k/v would make the bf16 kernel read K and V at
two bytes per element, past the end of both buffers. The guard sits at the top
of _flex_flash_attn_forward, before anything is allocated or launched, so CPU
tensors are enough to check it.

Every call here passes an EMPTY range table: even with the guard missing, both
C entries return on n_ranges == 0 before any launch, so this file can never
start a mixed-dtype kernel."""
import itertools
import re

import pytest
import torch

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn

MIXED = [
    c for c in itertools.product((BF16, FP8), repeat=3) if len(set(c)) > 1
]


def _tensors(dq, dk, dv, d=64):
    q = torch.zeros(4, 2, d).to(dq)
    k = torch.zeros(6, 2, d).to(dk)
    v = torch.zeros(6, 2, d).to(dv)
    empty = torch.zeros(0, 2, dtype=torch.int32)
    return q, k, v, empty


def _names(dq, dk, dv):
    return f"q={dq}.*k={dk}.*v={dv}".replace("torch.", r"torch\.")


def test_mixed_combinations_are_all_six():
    assert len(MIXED) == 6


@pytest.mark.parametrize("dq,dk,dv", MIXED, ids=lambda t: str(t)[6:])
def test_forward_rejects_mixed_dtypes(dq, dk, dv):
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
    )

    q, k, v, empty = _tensors(dq, dk, dv)
    with pytest.raises(AssertionError, match=_names(dq, dk, dv)) as ei:
        _flex_flash_attn_forward(
            q=q, k=k, v=v, sink=None, sink_layout="sh", out=None, lse=None,
            q_ranges=empty, k_ranges=empty.clone(), attn_type_map=None,
            softmax_scale=1.0, softcap=0.0, out_type=None,
            disable_fwd_atomic_reduction=False, deterministic=False,
            sm_margin=0, max_seqlen_q=0,
        )
    # same wording as the index path's guard
    assert re.search("must all be fp8-e4m3 or all be bf16", str(ei.value))


@pytest.mark.parametrize("dq,dk,dv", MIXED, ids=lambda t: str(t)[6:])
def test_public_entry_rejects_mixed_dtypes(dq, dk, dv):
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, empty = _tensors(dq, dk, dv)
    with pytest.raises(AssertionError, match=_names(dq, dk, dv)):
        flex_flash_attn_func(q, k, v, empty, empty.clone(), None,
                             max_seqlen_q=0)
