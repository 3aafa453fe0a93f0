"""Parity of the forward and dQ kernels with hand-ordered K/V staging.

Both kernels issue their K/V stage loads outside the compiler's wait
bookkeeping: the counted wait at the loop barrier is all that orders the
staging ring, and an explicit drain ends every k segment. The forward also
hands a causal range's q blocks out last-first. The shapes sit where that
ordering can go wrong, not at workload size:

  * k ranges of 33, 64, 65, 129, 193 and 257 rows: less than one 64-row stage,
    exactly one, a ring wrap (3 slots = 192 rows), and prefetches whose rows
    clamp past the end of the range; the same lengths as q ranges;
  * auto_range_merge tables with three or more k segments per q range, of
    unequal and sub-stage length (a drain and a restage between segments);
  * a CU margin that leaves two workgroups to walk all work items, so LDS is
    restaged across items, compared bit for bit with margin 0;
  * two launches accumulating into one out/lse and one dq buffer;
  * GQA, tq > tk and tq < tk under causal with several q blocks per range;
  * the same inputs twice: identical out, lse and dq.

Each shape runs on both kernel widths. "wide": the forward's default 8-wave
3-slot build and the dQ pass's 8-wave build (taken from max_seqlen_k >= 8192:
the launcher reads the bound, not the tensors). "narrow": the 4-wave 2-slot
builds (forward via MAGI_FWD_WAVES=4, dQ below the bound).

Every case compares against the fp64 oracle on the same bf16 inputs, budgeted
by the bf16 oracle's own error (tests/util.py); lse uses
the bound of tests/test_ffa_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

LENS = [33, 64, 65, 129, 193, 257]
TYPES = {"full": 0, "causal": 1, "inv_causal": 2, "bi_causal": 3}


def _packed(lens_q, lens_k):
    """Disjoint back-to-back ranges of the given lengths."""
    qr, kr, q0, k0 = [], [], 0, 0
    for lq, lk in zip(lens_q, lens_k):
        qr.append([q0, q0 + lq])
        kr.append([k0, k0 + lk])
        q0 += lq
        k0 += lk
    return q0, k0, qr, kr


def _table(name, atype):
    """(tq, tk, q_ranges, k_ranges, types, merge) of a named table."""
    if name == "klens":    # 70-row q ranges (3 waves, the last partial)
        tq, tk, qr, kr = _packed([70] * len(LENS), LENS)
        return tq, tk, qr, kr, [atype] * len(LENS), False
    if name == "qlens":    # 100-row k ranges: one stage + a clamped second
        tq, tk, qr, kr = _packed(LENS, [100] * len(LENS))
        return tq, tk, qr, kr, [atype] * len(LENS), False
    if name == "merge":
        # q range A: 4 k segments (17, 100, 257 and 64 rows); q range B: 3
        # (33, 65, 193). Segments of one q range are disjoint; the k range
        # [40, 140) serves both q ranges, so the dkv pass sees two q segments
        qr = [[0, 200], [0, 200], [0, 200], [0, 200],
              [200, 330], [200, 330], [200, 330]]
        kr = [[0, 17], [40, 140], [150, 407], [420, 484],
              [40, 140], [500, 565], [570, 763]]
        ty = [0, atype, atype, 0, atype, 0, atype]
        return 330, 763, qr, kr, ty, True
    if name == "tall":     # tq > tk: rows 0..299 see no key under causal
        return 600, 300, [[0, 600]], [[0, 300]], [atype], False
    if name == "wide_k":   # tq < tk
        return 300, 600, [[0, 300]], [[0, 600]], [atype], False
    if name == "one_517":  # 2 x 256 + 5 rows, one range
        return 517, 517, [[0, 517]], [[0, 517]], [atype], False
    raise KeyError(name)


_REF = {}


def _reference(key, q, k, v, dout, mask):
    """fp64 and bf16 oracle results, computed once per (table, shape)."""
    if key not in _REF:
        qc, kc, vc, doc = [t.detach().cpu() for t in (q, k, v, dout)]
        hi = ref_attn_with_grads(qc, kc, vc, mask, doc)
        lo = ref_attn_with_grads(
            qc, kc, vc, mask, doc, high_precision=False, p_dtype=torch.bfloat16
        )
        _REF[key] = (hi, lo)
    return _REF[key]


def _set_width(monkeypatch, wide):
    if wide:
        monkeypatch.delenv("MAGI_FWD_WAVES", raising=False)
    else:
        monkeypatch.setenv("MAGI_FWD_WAVES", "4")
    monkeypatch.delenv("MAGI_FWD_NBUF", raising=False)
    return 8192 if wide else None


def _run(monkeypatch, name, atype, d, wide, hq=2, hk=2, sm_margin=0):
    from magi_attention.functional import flex_flash_attn_func

    msk = _set_width(monkeypatch, wide)
    tq, tk, qr_l, kr_l, ty_l, merge = _table(name, atype)
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l
    )
    q.requires_grad_(True)
    k.requires_grad_(True)
    v.requires_grad_(True)
    out, meta = flex_flash_attn_func(
        q, k, v, qr, kr, tm, auto_range_merge=merge, max_seqlen_k=msk,
        sm_margin=sm_margin,
    )
    out.backward(dout)
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    hi, lo = _reference((name, atype, d, hq, hk), q, k, v, dout, mask)
    got = {"out": out.detach(), "lse": meta.lse.detach(), "dq": q.grad,
           "dk": k.grad, "dv": v.grad}
    return got, hi, lo


def _check(tag, got, hi, lo):
    names = ("out", "lse", "dq", "dk", "dv")
    for i, n in enumerate(names):
        g = got[n].cpu().float()
        if n == "lse":
            dead = torch.isinf(hi[1])
            assert torch.equal(torch.isinf(g) & (g < 0), dead), (
                f"{tag}: rows without a key must have lse = -inf"
            )
            torch.testing.assert_close(
                g[~dead], hi[1][~dead].float(), atol=5e-3, rtol=1e-3
            )
            continue
        assert torch.isfinite(g).all(), f"{tag}:{n} not finite"
        assert_close_to_ref(g, hi[i].float(), lo[i].float(), f"{tag}:{n}")


def _bit_equal(tag, a, b, which):
    for n in which:
        assert torch.equal(a[n], b[n]), f"{tag}: {n} differs bit for bit"


WIDTHS = [pytest.param(True, id="wide"), pytest.param(False, id="narrow")]


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("table", ["klens", "qlens"])
def test_range_lengths(monkeypatch, table, tname, d, wide):
    got, hi, lo = _run(monkeypatch, table, TYPES[tname], d, wide)
    _check(f"{table}:{tname}:d{d}", got, hi, lo)


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("tname", ["causal", "bi_causal"])
def test_merged_k_segments(monkeypatch, tname, d, wide):
    got, hi, lo = _run(monkeypatch, "merge", TYPES[tname], d, wide)
    _check(f"merge:{tname}:d{d}", got, hi, lo)


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("table", ["klens", "merge"])
def test_cu_margin_walk_matches_exact_grid(monkeypatch, table, wide):
    """margin 254 leaves 2 (8 waves) or 4 (4 waves) workgroups for 12+ work
    items. q ranges are disjoint, so every out/lse/dq element is written by
    one workgroup once: the strided walk must reproduce the exact grid bit
    for bit. dk/dv come from the untouched dkv kernels' atomics and are
    checked against the oracle only."""
    base, hi, lo = _run(monkeypatch, table, 1, 128, wide)
    walk, _, _ = _run(monkeypatch, table, 1, 128, wide, sm_margin=254)
    _check(f"margin:{table}", walk, hi, lo)
    _bit_equal(f"margin:{table}", base, walk, ("out", "lse", "dq"))


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
def test_gqa(monkeypatch, d, wide):
    got, hi, lo = _run(monkeypatch, "klens", 1, d, wide, hq=4, hk=2)
    _check(f"gqa:d{d}", got, hi, lo)


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("table", ["tall", "wide_k"])
def test_causal_rectangles_reversed_blocks(monkeypatch, table, d, wide):
    got, hi, lo = _run(monkeypatch, table, 1, d, wide)
    _check(f"{table}:d{d}", got, hi, lo)


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
def test_bitwise_repeat(monkeypatch, d, wide):
    """One range: every out, lse and dq element has a single writer."""
    a, hi, lo = _run(monkeypatch, "one_517", 1, d, wide)
    b, _, _ = _run(monkeypatch, "one_517", 1, d, wide)
    _check(f"repeat:d{d}", a, hi, lo)
    _bit_equal(f"repeat:d{d}", a, b, ("out", "lse", "dq"))


@requires_gpu
@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
def test_two_launches_accumulate(monkeypatch, d, wide):
    """K split at row 129 over two forward launches into one (out, lse) and
    two backward launches into one (dq, dk, dv) equals one call on the
    union."""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_backward,
        _flex_flash_attn_forward,
    )

    msk = _set_width(monkeypatch, wide)
    tq, tk, h = 300, 386, 2
    q, k, v, dout, _, _, _ = make_flex_case(
        tq, tk, h, h, d, [[0, tq]], [[0, tk]], [0]
    )
    out = torch.zeros(tq, h, d, dtype=torch.float32, device="cuda")
    lse = torch.full((tq, h), float("-inf"), dtype=torch.float32, device="cuda")
    dq = torch.zeros(tq, h, d, dtype=torch.float32, device="cuda")
    dk = torch.zeros(tk, h, d, dtype=torch.float32, device="cuda")
    dv = torch.zeros(tk, h, d, dtype=torch.float32, device="cuda")
    scale = d ** -0.5
    qr = torch.tensor([[0, tq]], dtype=torch.int32, device="cuda")
    parts = [
        torch.tensor([[a, b]], dtype=torch.int32, device="cuda")
        for a, b in ((0, 129), (129, tk))
    ]
    tm = torch.zeros(1, dtype=torch.int32, device="cuda")
    for kr in parts:
        _flex_flash_attn_forward(
            q=q, k=k, v=v, sink=None, sink_layout="sh", out=out, lse=lse,
            q_ranges=qr, k_ranges=kr, attn_type_map=tm, softmax_scale=scale,
            softcap=0.0, out_type=None, disable_fwd_atomic_reduction=False,
            deterministic=False, sm_margin=0,
        )
    for kr in parts:
        _flex_flash_attn_backward(
            dout=dout, q=q, k=k, v=v, sink=None, sink_layout="sh", out=out,
            lse=lse, dq=dq, dk=dk, dv=dv, dsink=None, q_ranges=qr,
            k_ranges=kr, attn_type_map=tm, softmax_scale=scale, softcap=0.0,
            dq_type=None, dk_type=None, dv_type=None,
            disable_bwd_dkv_atomic_reduction=False, deterministic=False,
            sm_margin=0, max_seqlen_k=msk,
        )
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, [[0, tq]], [[0, tk]], [0])
    hi, lo = _reference(("acc", d), q, k, v, dout, mask)
    got = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    _check(f"acc:d{d}", got, hi, lo)
