"""Parity of the fused dK/dV backward with register-prefetched lse/dpsum, and
of the dQ pass with its causal blocks handed out last-first.

The fused kernel (8 waves, chosen from max_seqlen_k >= 1024) carries each
staged tile's lse/dpsum in lane registers loaded one tile ahead. The shapes
are the smallest at which a carried value can go wrong: a q loop that starts
off a 32-row boundary, a partial last subtile whose rows clamp to qe - 1, two
subtiles per staged tile (D=64), a second q segment behind a first one that
ends mid-tile, band masks that cut a tile, rows with lse = -inf, and a full
mask that never leaves the fast path.

Every case compares against the fp64 oracle on the same bf16 inputs, budgeted
by the bf16 oracle's own error (tests/util.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

H = 2  # hq = hk

# name, tq, tk, d, q_ranges, k_ranges, types, auto_range_merge, max_seqlen_k
DKV_CASES = [
    # ke - qe = 11: every block's q loop starts at nblk0 - 11, off the 32-row
    # grid; 1061 rows leave a partial last subtile
    ("causal_d128", 1061, 1072, 128, [[0, 1061]], [[0, 1072]], [1], False, None),
    ("causal_d64", 1061, 1072, 64, [[0, 1061]], [[0, 1072]], [1], False, None),
    # one k range, two q segments: segment 0 ends at row 301, mid-tile, so a
    # value prefetched past its end would be a row of the gap, not of segment 1
    ("two_qseg_merge_d128", 1061, 1100, 128,
     [[0, 301], [512, 1061]], [[0, 1100], [0, 1100]], [0, 1], True, None),
    ("two_qseg_merge_d64", 1061, 1100, 64,
     [[0, 301], [512, 1061]], [[0, 1100], [0, 1100]], [0, 1], True, None),
    # band masks: qs = 7 puts every wave's wq_hi = n0 + 32 + 7 inside a tile
    ("bicausal_d128", 520, 1100, 128, [[7, 507]], [[0, 1100]], [3], False, None),
    ("invcausal_d128", 1061, 1061, 128, [[7, 1061]], [[0, 1061]], [2], False,
     None),
    # 400 q rows on 261 keys under bottom-right causal: rows 0..138 see no key
    # (lse = -inf); rows 400..699 belong to no range at all
    ("masked_rows_d128", 1200, 1061, 128,
     [[0, 400], [700, 1200]], [[0, 261], [0, 1061]], [1, 1], False, None),
    ("full_d128", 1061, 1061, 128, [[0, 1061]], [[0, 1061]], [0], False, None),
]

# dQ pass, block order only: 2 x 256 + 5 rows on the 8-wave kernel (taken
# from max_seqlen_k >= 8192: the launcher reads the bound, not the tensors),
# and a 600-row range on the 4-wave kernel
DQ_CASES = [
    ("dq_w8_517", 517, 517, 128, [[0, 517]], [[0, 517]], [1], False, 8192),
    ("dq_w4_600", 600, 600, 128, [[0, 600]], [[0, 600]], [1], False, None),
]


def _run_case(case):
    from magi_attention.functional import flex_flash_attn_func

    name, tq, tk, d, qr_l, kr_l, ty_l, merge, msk = case
    q, k, v, dout, qr, kr, tm = make_flex_case(tq, tk, H, H, d, qr_l, kr_l, ty_l)
    q.requires_grad_(True)
    k.requires_grad_(True)
    v.requires_grad_(True)
    out, _ = flex_flash_attn_func(
        q, k, v, qr, kr, tm, auto_range_merge=merge, max_seqlen_k=msk
    )
    out.backward(dout)
    torch.cuda.synchronize()

    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    qc, kc, vc, doc = [t.detach().cpu() for t in (q, k, v, dout)]
    hi = ref_attn_with_grads(qc, kc, vc, mask, doc)
    lo = ref_attn_with_grads(
        qc, kc, vc, mask, doc, high_precision=False, p_dtype=torch.bfloat16
    )
    got = {"dq": q.grad, "dk": k.grad, "dv": v.grad}
    ref = {"dq": (hi[2], lo[2]), "dk": (hi[3], lo[3]), "dv": (hi[4], lo[4])}
    return name, got, ref


def _check(name, got, ref, which):
    for g in which:
        assert torch.isfinite(got[g]).all(), f"{name}:{g} not finite"
        assert_close_to_ref(
            got[g].cpu().float(), ref[g][0].float(), ref[g][1].float(),
            f"{name}:{g}",
        )


@requires_gpu
@pytest.mark.parametrize("case", DKV_CASES, ids=[c[0] for c in DKV_CASES])
def test_fused_dkv_prefetch_parity(case):
    name, got, ref = _run_case(case)
    _check(name, got, ref, ("dk", "dv", "dq"))


@requires_gpu
@pytest.mark.parametrize("case", DQ_CASES, ids=[c[0] for c in DQ_CASES])
def test_dq_descending_blocks_parity(case):
    name, got, ref = _run_case(case)
    _check(name, got, ref, ("dq", "dk", "dv"))
