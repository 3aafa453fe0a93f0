"""Parity of the dK/dV backward kernels whose dV/dK fragment reads run one
step ahead of their MFMAs.

The fused kernel (8 waves, chosen from max_seqlen_k >= 1024; shorter ranges
go to the split kernels) issues the transposed read of step j + 1 before the
MFMA of step j, across the dV/dK alternation and across the 32-column d
tiles, inside one 32-row subtile. The shapes are the smallest at
which a fragment consumed one step early or late, a fragment carried over a
skipped subtile, or a stage load the ring did not wait for gives a wrong
number: a q loop that starts off the 32-row grid and ends in a partial
subtile, two subtiles per staged tile (d = 64), a k block whose last waves
are not live, waves whose subtile is skipped by a band mask, a second q
segment behind one that ends mid-tile, a q segment shorter than a subtile,
an empty q segment, a GQA group walked by one workgroup (cat_gqa), the direct
16-bit epilogue, and - for the split kernels, which loop over work items - a
CU margin that leaves one workgroup several work items.

Every case compares dq, dk and dv against the fp64 oracle on the same 16-bit
inputs, budgeted by the 16-bit oracle's own error (tests/util.py, DESIGN
section 5b)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

BF16, FP16 = torch.bfloat16, torch.float16

# name -> tq, tk, q_ranges, k_ranges, types, auto_range_merge
# Long tables: k ranges of 1061..1100 keys = 5 blocks of 256 (8 waves); the
# last block has 1 to 3 live waves of 8.
# Short tables (_s): k ranges under 1024 keys, 4-wave kernels (128-key
# blocks, 64-row staged tiles).
SEGS = {
    # ke - qe = 11: every block's q loop starts at nblk0 - 11, off the 32-row
    # grid; 1061 rows leave a partial last subtile; waves with n0 >= 1072 idle
    "causal": (1061, 1072, [[0, 1061]], [[0, 1072]], [1], False),
    # one k range, two q segments, the first ending at row 301, mid-tile
    "two_qseg": (1061, 1100, [[0, 301], [512, 1061]],
                 [[0, 1100], [0, 1100]], [0, 1], True),
    # a 19-row q segment: one partial subtile, then a long segment
    "short_qseg": (1061, 1100, [[0, 19], [40, 1061]],
                   [[0, 1100], [0, 1100]], [0, 1], True),
    # an empty q segment between two live ones
    "empty_qseg": (1061, 1100, [[0, 301], [400, 400], [512, 1061]],
                   [[0, 1100], [0, 1100], [0, 1100]], [0, 0, 1], True),
    # band masks: qs = 7 puts every wave's wq_hi = n0 + 32 + 7 inside a tile,
    # so within one staged tile some waves compute and others skip
    "bicausal": (520, 1100, [[7, 507]], [[0, 1100]], [3], False),
    "invcausal": (1061, 1061, [[7, 1061]], [[0, 1061]], [2], False),
    "full": (1061, 1061, [[0, 1061]], [[0, 1061]], [0], False),
    # two disjoint k ranges: more work items for the CU-margin walk
    "two_krange": (1061, 2200, [[0, 530], [530, 1061]],
                   [[0, 1100], [1100, 2200]], [1, 0], False),
    "causal_s": (517, 528, [[0, 517]], [[0, 528]], [1], False),
    "empty_qseg_s": (600, 700, [[0, 301], [400, 400], [512, 600]],
                     [[0, 700], [0, 700], [0, 700]], [0, 0, 1], True),
    "short_qseg_s": (600, 700, [[0, 19], [40, 600]],
                     [[0, 700], [0, 700]], [0, 1], True),
    "bicausal_s": (420, 700, [[7, 407]], [[0, 700]], [3], False),
}


def _case(seg, d, path, dtype=BF16, hq=2, hk=2, **kw):
    tag = f"{path}-{seg}-d{d}-{'bf16' if dtype == BF16 else 'fp16'}"
    if hq != hk:
        tag += f"-h{hq}{hk}"
    tag += "".join(f"-{k}" for k in sorted(kw))
    return pytest.param((seg, d, path, dtype, hq, hk, kw), id=tag)


# path: "fused" (8 waves), "fused4" (MAGI_BWD_FUSED_DKV=1 on k ranges under
# 1024 keys: 4 waves), "split8" (MAGI_BWD_SPLIT_DKV=1, 8 waves, 3-slot ring),
# "split4" (k ranges under 1024 keys or D = 192: 4 waves, 2 slots)
FUSED_CASES = [
    _case("causal", 128, "fused"),
    _case("causal", 64, "fused"),
    _case("causal", 128, "fused", FP16),
    _case("causal", 64, "fused", FP16),
    _case("two_qseg", 128, "fused"),
    _case("two_qseg", 64, "fused"),
    _case("short_qseg", 128, "fused"),
    _case("short_qseg", 64, "fused"),
    _case("empty_qseg", 128, "fused"),
    _case("bicausal", 128, "fused"),
    _case("bicausal", 64, "fused"),
    _case("invcausal", 128, "fused"),
    _case("full", 128, "fused"),
    _case("causal", 128, "fused", hq=4, hk=2, cat_gqa=True),
    _case("two_qseg", 64, "fused", hq=4, hk=2, cat_gqa=True),
    _case("causal", 128, "fused", hq=4, hk=2, cat_gqa=True, direct=True),
    _case("causal", 128, "fused", direct=True),
    _case("causal", 128, "fused", FP16, direct=True),
    _case("bicausal", 64, "fused", direct=True),
    _case("causal", 128, "fused", softcap=0.5),
    # the 4-wave fused builds (two subtiles per staged tile at both d)
    _case("causal_s", 128, "fused4"),
    _case("empty_qseg_s", 64, "fused4"),
    _case("bicausal_s", 128, "fused4", FP16),
]

SPLIT_CASES = [
    _case("causal", 128, "split8"),
    _case("causal", 128, "split8", FP16),
    _case("causal", 64, "split8"),
    _case("two_qseg", 128, "split8"),
    _case("short_qseg", 128, "split8"),
    _case("empty_qseg", 128, "split8"),
    _case("bicausal", 128, "split8"),
    _case("invcausal", 128, "split8"),
    _case("two_krange", 128, "split8", margin=254),
    _case("two_qseg", 128, "split8", hq=4, hk=2, cat_gqa=True, margin=254),
    _case("causal", 128, "split8", softcap=0.5),
    _case("causal_s", 128, "split4"),
    _case("causal_s", 128, "split4", FP16),
    _case("empty_qseg_s", 128, "split4"),
    _case("short_qseg_s", 64, "split4"),
    _case("bicausal_s", 128, "split4"),
    _case("empty_qseg_s", 128, "split4", margin=254),
    _case("causal_s", 128, "split4", softcap=0.5),
    _case("causal_s", 192, "split4"),
    _case("empty_qseg_s", 192, "split4"),
    _case("bicausal_s", 192, "split4", margin=254),
    _case("two_qseg", 192, "split4"),
]

_REF = {}


def _reference(key, q, k, v, dout, mask, dtype, softcap):
    """fp64 and 16-bit oracle results, computed once per key, read-only."""
    if key not in _REF:
        qc, kc, vc, doc = [t.detach().cpu() for t in (q, k, v, dout)]
        hi = ref_attn_with_grads(qc, kc, vc, mask, doc, softcap=softcap)
        lo = ref_attn_with_grads(
            qc, kc, vc, mask, doc, softcap=softcap,
            high_precision=False, p_dtype=dtype,
        )
        _REF[key] = (hi, lo)
    return _REF[key]


def _run_and_check(monkeypatch, case):
    from magi_attention.functional import flex_flash_attn_func

    seg, d, path, dtype, hq, hk, kw = case
    tq, tk, qr_l, kr_l, ty_l, merge = SEGS[seg]
    softcap = kw.get("softcap", 0.0)
    longest = max(e - s for s, e in kr_l)
    for name in ("MAGI_BWD_SPLIT_DKV", "MAGI_BWD_FUSED_DKV", "MAGI_BWD_BIGSEQ",
                 "MAGI_BWD_HEAD_MAJOR", "MAGI_BWD_COSCHED"):
        monkeypatch.delenv(name, raising=False)
    if path == "split8":
        monkeypatch.setenv("MAGI_BWD_SPLIT_DKV", "1")
    if path == "fused4":
        monkeypatch.setenv("MAGI_BWD_FUSED_DKV", "1")
    # the launcher picks the kernels from the bound max_seqlen_k, which
    # defaults to the longest k range
    if path == "split4":
        assert longest < 1024 or d == 192
    elif path == "fused4":
        assert longest < 1024 and d != 192
    else:
        assert longest >= 1024 and d != 192

    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l, dtype=dtype
    )
    for t in (q, k, v):
        t.requires_grad_(True)
    out, _ = flex_flash_attn_func(
        q, k, v, qr, kr, tm, auto_range_merge=merge, softcap=softcap,
        sm_margin=kw.get("margin", 0), cat_gqa=kw.get("cat_gqa", False),
        disable_bwd_dkv_atomic_reduction=kw.get("direct", False),
    )
    out.backward(dout)
    torch.cuda.synchronize()
    if kw.get("direct"):
        assert k.grad.dtype == dtype and v.grad.dtype == dtype

    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    hi, lo = _reference(
        (seg, d, dtype, hq, hk, softcap), q, k, v, dout, mask, dtype, softcap
    )
    tag = f"{path}:{seg}:d{d}"
    for i, (n, g) in enumerate((("dq", q.grad), ("dk", k.grad), ("dv", v.grad))):
        assert torch.isfinite(g).all(), f"{tag}:{n} not finite"
        assert_close_to_ref(
            g.cpu().float(), hi[2 + i].float(), lo[2 + i].float(), f"{tag}:{n}"
        )


@requires_gpu
@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_dkv_fragment_pipeline_parity(monkeypatch, case):
    _run_and_check(monkeypatch, case)


@requires_gpu
@pytest.mark.parametrize("case", SPLIT_CASES)
def test_split_dkv_parity(monkeypatch, case):
    _run_and_check(monkeypatch, case)
