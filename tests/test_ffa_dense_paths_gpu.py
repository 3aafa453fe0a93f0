"""Parity of the dense bf16 kernels on the launch paths no other test takes.

  A. softcap where tanh bends: softcap=0.5 at the default scale (s / cap of
     order one half) and softmax_scale=1, softcap=2 (|s| / cap past one, tanh
     saturating). tests/test_softcap_power_cpu.py proves on the CPU that an
     implementation which drops the tanh, or its derivative, misses every
     budget used here by 3x or more. Every softcap build runs: forward 8 and
     4 waves, dQ 4 and 8 waves, dK/dV split 4 waves, split 8 waves and fused
     8 waves, and the D=192 builds.
  B. the work-major grid order (MAGI_FWD_HEADMAJOR=0, MAGI_BWD_HEAD_MAJOR=0),
     which the launchers pick on their own only past 32k keys: against the
     oracle, bit for bit against head-major, and under a CU margin.
  C. the direct-store forward epilogue (disable_fwd_atomic_reduction), bf16
     and fp32 out: rows of no range and rows without a key are left alone.
  D. deterministic backward against the oracle: overlapping q and k ranges
     off the 128 grid, GQA sub-launches checked per kv head, split and fused
     dK/dV, both grid orders.
  E. D=192 (and d=160 padded into it) on partial tiles, band masks and rows
     without a key.

Builds are reached the way the launchers choose them: forward 4 waves by
MAGI_FWD_WAVES=4; dQ 8 waves by max_seqlen_k=8192 (the launcher reads the
bound, not the tensors); fused 8-wave dK/dV by max_seqlen_k >= 1024; split
8-wave dK/dV by MAGI_BWD_SPLIT_DKV=1 with that bound; split 4-wave dK/dV by
passing no bound.

Every case compares against the fp64 oracle on the same bf16 inputs, budgeted
by the bf16 oracle's own error (tests/util.py); lse uses
the bound of tests/test_fwd_dq_prefetch_gpu.py. Measured errors are in
profiles/dense_launch_paths.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.test_fwd_dq_prefetch_gpu import TYPES, _table  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

NAMES = ("out", "lse", "dq", "dk", "dv")

# (softmax_scale, softcap); None = the default d ** -0.5
REGIMES = {"half": (None, 0.5), "sat": (1.0, 2.0)}

# kernel builds taken by one forward + backward call:
#   name -> (forward waves, max_seqlen_k bound, force split dK/dV)
BUILDS = {
    "narrow": (4, None, False),      # fwd 4, dQ 4, split 4-wave dK/dV
    "wide_fused": (8, 8192, False),  # fwd 8, dQ 8, fused 8-wave dK/dV
    "wide_split": (8, 8192, True),   # fwd 8, dQ 8, split 8-wave dK/dV
}

# the softcap cases: (table, mask type, regime, hq, hk). Each runs at d = 64
# and 128 on every build; tests/test_softcap_power_cpu.py walks the same list.
SOFTCAP_CASES = (
    [("klens", t, "half", 2, 2) for t in TYPES]
    + [(tb, t, "half", 2, 2)
       for tb in ("qlens", "merge") for t in ("causal", "bi_causal")]
    # tall has more q rows than keys: bi-causal masks all of it, causal
    # leaves rows 0..299 without a key
    + [("tall", "causal", "half", 2, 2)]
    + [("klens", "causal", "half", 4, 2)]
    + [("klens", t, "sat", 2, 2) for t in TYPES]
    + [("merge", "causal", "sat", 2, 2), ("tall", "causal", "sat", 2, 2)]
)
SOFTCAP_D192 = ("klens", "causal", "half", 2, 2)


def softcap_inputs(table, tname, regime, hq, hk, d, device="cpu"):
    """Inputs, mask and (scale, cap) of one softcap case."""
    tq, tk, qr_l, kr_l, ty_l, merge = _table(table, TYPES[tname])
    tensors = make_flex_case(tq, tk, hq, hk, d, qr_l, kr_l, ty_l, device=device)
    scale, cap = REGIMES[regime]
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    return tensors, mask, scale, cap, merge


_REF = {}


def _reference(key, q, k, v, dout, mask, scale=None, cap=0.0):
    """fp64 and bf16 oracle results, computed once per key."""
    if key not in _REF:
        qc, kc, vc, doc = [t.detach().cpu() for t in (q, k, v, dout)]
        hi = ref_attn_with_grads(
            qc, kc, vc, mask, doc, softmax_scale=scale, softcap=cap
        )
        lo = ref_attn_with_grads(
            qc, kc, vc, mask, doc, softmax_scale=scale, softcap=cap,
            high_precision=False, p_dtype=torch.bfloat16,
        )
        _REF[key] = (hi, lo)
    return _REF[key]


def _set_build(monkeypatch, build):
    """Select the kernel builds; returns the max_seqlen_k bound to pass."""
    waves, bound, split = BUILDS[build]
    if waves == 4:
        monkeypatch.setenv("MAGI_FWD_WAVES", "4")
    else:
        monkeypatch.delenv("MAGI_FWD_WAVES", raising=False)
    if split:
        monkeypatch.setenv("MAGI_BWD_SPLIT_DKV", "1")
    else:
        monkeypatch.delenv("MAGI_BWD_SPLIT_DKV", raising=False)
    for name in ("MAGI_FWD_NBUF", "MAGI_BWD_FUSED_DKV", "MAGI_BWD_BIGSEQ",
                 "MAGI_BWD_DQ_BIGSEQ"):
        monkeypatch.delenv(name, raising=False)
    return bound


def _set_grid_order(monkeypatch, head_major):
    """None leaves the launchers' own choice (head-major at these sizes)."""
    for name in ("MAGI_FWD_HEADMAJOR", "MAGI_BWD_HEAD_MAJOR"):
        if head_major is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "1" if head_major else "0")


def _run(monkeypatch, table, tname, d, build, hq=2, hk=2, regime=None,
         head_major=None, sm_margin=0, deterministic=False, ranges=None,
         bound=None, **kw):
    """One forward + backward through flex_flash_attn_func and its oracle.
    ranges = (tq, tk, q_ranges, k_ranges, types, merge) replaces the table."""
    from magi_attention.functional import flex_flash_attn_func

    msk = _set_build(monkeypatch, build)
    if bound is not None:
        msk = bound
    _set_grid_order(monkeypatch, head_major)
    tq, tk, qr_l, kr_l, ty_l, merge = ranges or _table(table, TYPES[tname])
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l
    )
    scale, cap = REGIMES[regime] if regime else (None, 0.0)
    q.requires_grad_(True)
    k.requires_grad_(True)
    v.requires_grad_(True)
    out, meta = flex_flash_attn_func(
        q, k, v, qr, kr, tm, auto_range_merge=merge, max_seqlen_k=msk,
        sm_margin=sm_margin, softmax_scale=scale, softcap=cap,
        deterministic=deterministic, **kw,
    )
    out.backward(dout)
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    hi, lo = _reference(
        (table, tname, d, hq, hk, regime), q, k, v, dout, mask, scale, cap
    )
    got = {"out": out.detach(), "lse": meta.lse.detach(), "dq": q.grad,
           "dk": k.grad, "dv": v.grad}
    return got, hi, lo


def _check(tag, got, hi, lo, grad_ratio=3.0, rows=None):
    """Oracle parity of whichever of out, lse, dq, dk, dv `got` holds. Rows
    without a key must have lse = -inf and out = 0 exactly. rows (a bool
    vector over q rows) restricts the out/lse comparison to those rows."""
    dead = torch.isinf(hi[1])
    for i, n in enumerate(NAMES):
        if n not in got:
            continue
        g = got[n].cpu().float()
        h, l = hi[i].float(), lo[i].float()
        if n == "lse":
            if rows is None:
                assert torch.equal(torch.isinf(g) & (g < 0), dead), (
                    f"{tag}: rows without a key must have lse = -inf"
                )
            live = ~dead if rows is None else (~dead & rows[:, None])
            if live.any():
                worst = (g[live] - h[live]).abs().max().item()
                print(f"    [{tag}:lse] max abs err={worst:.3e}")
            torch.testing.assert_close(
                g[live], h[live], atol=5e-3, rtol=1e-3
            )
            continue
        assert torch.isfinite(g).all(), f"{tag}:{n} not finite"
        if n == "out":
            if rows is None:
                assert (g[dead] == 0).all(), (
                    f"{tag}: rows without a key must have out = 0"
                )
            else:
                g, h, l = g[rows], h[rows], l[rows]
            assert_close_to_ref(g, h, l, f"{tag}:out")
        else:
            assert_close_to_ref(g, h, l, f"{tag}:{n}", ratio=grad_ratio)


def _bit_equal(tag, a, b, which):
    for n in which:
        assert torch.equal(a[n], b[n]), f"{tag}: {n} differs bit for bit"


# --------------------------------------------------------------------------
# A. softcap where it matters
# --------------------------------------------------------------------------

def _case_id(c):
    table, tname, regime, hq, hk = c
    return f"{table}-{tname}-{regime}-h{hq}{hk}"


@requires_gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("case", SOFTCAP_CASES, ids=_case_id)
def test_softcap(monkeypatch, case, d, build):
    table, tname, regime, hq, hk = case
    got, hi, lo = _run(
        monkeypatch, table, tname, d, build, hq=hq, hk=hk, regime=regime
    )
    _check(f"softcap:{_case_id(case)}:d{d}:{build}", got, hi, lo)


# largest dq/dk/dv error over budget measured on the MI355X at ratio 3.0 is
# in profiles/dense_launch_paths.md; the ceiling the project allows D=192
# gradients is the 4.5 of test_ffa_gpu.test_head_dim_192_bucket
D192_GRAD_RATIO = 3.0


@requires_gpu
def test_softcap_d192(monkeypatch):
    """D=192 has 4-wave builds only: forward, dQ and split dK/dV."""
    table, tname, regime, hq, hk = SOFTCAP_D192
    got, hi, lo = _run(
        monkeypatch, table, tname, 192, "narrow", hq=hq, hk=hk, regime=regime
    )
    _check("softcap:d192", got, hi, lo, grad_ratio=D192_GRAD_RATIO)


# --------------------------------------------------------------------------
# B. work-major grid
# --------------------------------------------------------------------------

WIDTHS = [pytest.param("wide_fused", id="wide"),
          pytest.param("narrow", id="narrow")]


def _both_orders(monkeypatch, tag, table, d, build, **kw):
    """head-major then work-major; the q ranges of these tables are disjoint
    (or merge to disjoint ones), so every out, lse and dq element has one
    writer and the two grid orders must agree bit for bit. dk and dv come
    from atomics and are checked against the oracle only."""
    head, hi, lo = _run(
        monkeypatch, table, "causal", d, build, head_major=True, **kw
    )
    work, _, _ = _run(
        monkeypatch, table, "causal", d, build, head_major=False, **kw
    )
    _check(tag, work, hi, lo)
    _bit_equal(tag, head, work, ("out", "lse", "dq"))
    return work, hi, lo


@requires_gpu
@pytest.mark.parametrize("build", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("table", ["klens", "merge", "one_517"])
def test_work_major(monkeypatch, table, d, build):
    _both_orders(monkeypatch, f"workmajor:{table}:d{d}", table, d, build)


@requires_gpu
@pytest.mark.parametrize("build", WIDTHS)
@pytest.mark.parametrize("d", [64, 128])
def test_work_major_gqa(monkeypatch, d, build):
    _both_orders(
        monkeypatch, f"workmajor:gqa:d{d}", "klens", d, build, hq=4, hk=2
    )


@requires_gpu
@pytest.mark.parametrize("build", WIDTHS)
def test_work_major_cu_margin(monkeypatch, build):
    """margin 254 leaves 2 (8 waves) or 4 (4 waves) workgroups to walk the
    work-major work space; it must reproduce the exact work-major grid."""
    exact, hi, lo = _run(
        monkeypatch, "klens", "causal", 128, build, head_major=False
    )
    walk, _, _ = _run(
        monkeypatch, "klens", "causal", 128, build, head_major=False,
        sm_margin=254,
    )
    _check("workmajor:margin", walk, hi, lo)
    _bit_equal("workmajor:margin", exact, walk, ("out", "lse", "dq"))


# --------------------------------------------------------------------------
# C. direct-store forward
# --------------------------------------------------------------------------

# rows 70..106 and 500..516 belong to no range; the causal range is taller
# than its keys (300 x 150), so its first 150 rows, 107..256, see no key, and
# so do the last 28 rows, 472..499, of the inv-causal range (93 x 65)
GAP_TQ, GAP_TK = 517, 344
GAP_Q = [[0, 70], [107, 407], [407, 500]]
GAP_K = [[0, 129], [129, 279], [279, 344]]
GAP_T = [0, 1, 2]
OUT_SENTINEL, LSE_SENTINEL = 7.25, 123.0   # exact in bf16


def _gap_rows():
    inside = torch.zeros(GAP_TQ, dtype=torch.bool)
    for a, b in GAP_Q:
        inside[a:b] = True
    return inside


def _forward_only(monkeypatch, key, waves, d, tq, tk, qr_l, kr_l, ty_l,
                  direct, out_dtype, merge=False):
    """_flex_flash_attn_forward into caller-owned out / lse. Direct stores
    start from the sentinels, the atomic path from its own zero / -inf."""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
        _seg_starts,
        merge_ranges,
    )

    _set_build(monkeypatch, "wide_fused" if waves == 8 else "narrow")
    _set_grid_order(monkeypatch, None)
    hq = hk = 2
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l
    )
    if direct:
        out = torch.full((tq, hq, d), OUT_SENTINEL, dtype=out_dtype,
                         device="cuda")
        lse = torch.full((tq, hq), LSE_SENTINEL, dtype=torch.float32,
                         device="cuda")
    else:
        out = torch.zeros(tq, hq, d, dtype=torch.float32, device="cuda")
        lse = torch.full((tq, hq), float("-inf"), dtype=torch.float32,
                         device="cuda")
    starts = None
    if merge:
        qr, _, kr, tm, inv_q, _ = merge_ranges(qr, kr, tm)
        starts = _seg_starts(inv_q, qr.shape[0])
    _flex_flash_attn_forward(
        q=q, k=k, v=v, sink=None, sink_layout="sh", out=out, lse=lse,
        q_ranges=qr, k_ranges=kr, attn_type_map=tm, softmax_scale=d ** -0.5,
        softcap=0.0, out_type=None, disable_fwd_atomic_reduction=direct,
        deterministic=False, sm_margin=0, qk_starts=starts,
    )
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    hi, lo = _reference((key, d), q, k, v, dout, mask)
    return out, lse, hi, lo


def _check_direct(tag, out, lse, hi, lo, inside):
    """Rows of no range and rows without a key keep the sentinels exactly;
    the rest match the oracle."""
    dead = torch.isinf(hi[1]).all(dim=1)        # per q row, every head
    assert torch.equal(torch.isinf(hi[1]).any(dim=1), dead)
    assert (dead & inside).any() and (~inside).any() and (~dead).any()
    o, s = out.cpu().float(), lse.cpu()
    assert (o[dead] == OUT_SENTINEL).all(), (
        f"{tag}: out written on a row of no range or without a key"
    )
    assert (s[dead] == LSE_SENTINEL).all(), (
        f"{tag}: lse written on a row of no range or without a key"
    )
    _check(tag, {"out": o, "lse": s}, hi, lo, rows=~dead)


@requires_gpu
@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize(
    "out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"]
)
def test_direct_store(monkeypatch, out_dtype, d, waves):
    out, lse, hi, lo = _forward_only(
        monkeypatch, "gap", waves, d, GAP_TQ, GAP_TK, GAP_Q, GAP_K, GAP_T,
        True, out_dtype,
    )
    _check_direct(f"direct:d{d}:w{waves}", out, lse, hi, lo, _gap_rows())


@requires_gpu
@pytest.mark.parametrize("waves", [8, 4])
def test_direct_store_merged_segments(monkeypatch, waves):
    """The merge table's k segments iterate in-kernel, so each q range still
    has one writer and the store stays direct. 20 extra q rows belong to no
    range; under causal the 200-row range's first rows see keys only through
    its full segments, so no row of a range is without a key here."""
    _, tk, qr_l, kr_l, ty_l, _ = _table("merge", 1)
    tq = 350
    out, lse, hi, lo = _forward_only(
        monkeypatch, "gap_merge", waves, 128, tq, tk, qr_l, kr_l, ty_l, True,
        torch.float32, merge=True,
    )
    dead = torch.isinf(hi[1]).all(dim=1)
    assert torch.equal(dead, torch.arange(tq) >= 330)
    o, s = out.cpu().float(), lse.cpu()
    assert (o[dead] == OUT_SENTINEL).all() and (s[dead] == LSE_SENTINEL).all()
    _check(f"direct:merge:w{waves}", {"out": o, "lse": s}, hi, lo, rows=~dead)


# Largest element-wise relative difference between the fp32 direct store and
# the atomic path of the same call, measured on the MI355X: 0.0 at every d
# and width. That is what the code says: on a first write the merge sees
# lse_prev = -inf, so lse_m = lse_new + log1p(exp(-inf)) = lse_new, its
# weight is exp(0) * (1 / l) = 1 / l and it stores 0 + (1 / l) * acc, the
# direct store's acc * (1 / l). Four times the measured figure is the bound.
DIRECT_VS_ATOMIC_MEASURED = 0.0


@requires_gpu
@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("d", [64, 128])
def test_direct_store_matches_atomic(monkeypatch, d, waves):
    args = ("gap", waves, d, GAP_TQ, GAP_TK, GAP_Q, GAP_K, GAP_T)
    f32, lse_d, hi, _ = _forward_only(monkeypatch, *args, True, torch.float32)
    b16, _, _, _ = _forward_only(monkeypatch, *args, True, torch.bfloat16)
    ato, lse_a, _, _ = _forward_only(monkeypatch, *args, False, torch.float32)
    live = ~torch.isinf(hi[1]).all(dim=1)
    a, b = f32.cpu()[live].double(), ato.cpu()[live].double()
    rel = ((a - b).abs() / b.abs().clamp_min(1e-30)).max().item()
    print(f"    [direct-vs-atomic d{d} w{waves}] max rel diff = {rel:.3e}")
    assert rel <= 4 * DIRECT_VS_ATOMIC_MEASURED
    assert torch.equal(lse_d.cpu()[live], lse_a.cpu()[live])
    assert torch.equal(b16, f32.to(torch.bfloat16)), (
        "bf16 direct store is not the fp32 direct store rounded to bf16"
    )


@requires_gpu
@pytest.mark.parametrize("build", WIDTHS)
def test_direct_store_end_to_end(monkeypatch, build):
    """flex_flash_attn_func with the direct store; the backward reads the
    bf16 out it wrote."""
    got, hi, lo = _run(
        monkeypatch, "gap", "mixed", 128, build,
        ranges=(GAP_TQ, GAP_TK, GAP_Q, GAP_K, GAP_T, False),
        disable_fwd_atomic_reduction=True,
    )
    assert got["out"].dtype == torch.bfloat16
    _check(f"direct:e2e:{build}", got, hi, lo)


# --------------------------------------------------------------------------
# D. deterministic backward against the oracle
# --------------------------------------------------------------------------

# q ranges overlap each other and so do k ranges, off the 128 grid; the
# (q, k) rectangles stay disjoint, as the kernels require. All four types.
DET_RANGES = (
    517, 517,
    [[0, 301], [150, 517], [0, 150], [401, 517]],
    [[0, 129], [129, 386], [300, 517], [386, 517]],
    [1, 0, 2, 3],
    False,
)


def _deterministic(monkeypatch, hq, hk, d, fused, head_major=None):
    kw = dict(hq=hq, hk=hk, ranges=DET_RANGES, deterministic=True,
              head_major=head_major, bound=1024 if fused else None)
    build = "wide_fused" if fused else "narrow"
    a, hi, lo = _run(monkeypatch, "det", "mixed", d, build, **kw)
    b, _, _ = _run(monkeypatch, "det", "mixed", d, build, **kw)
    tag = f"det:h{hq}{hk}:d{d}:{'fused' if fused else 'split'}"
    _check(tag, a, hi, lo)
    _bit_equal(tag, a, b, NAMES)
    # a sub-launch over the wrong q heads can hide in a whole-tensor norm
    for i, n in ((3, "dk"), (4, "dv")):
        for j in range(hk):
            assert_close_to_ref(
                a[n][:, j].cpu().float(), hi[i][:, j].float(),
                lo[i][:, j].float(), f"{tag}:{n}[:, {j}]",
            )


@requires_gpu
@pytest.mark.parametrize("fused", [False, True], ids=["split4", "fused8"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hq", [2, 4, 8])
def test_deterministic_vs_oracle(monkeypatch, hq, d, fused):
    _deterministic(monkeypatch, hq, 2, d, fused)


@requires_gpu
@pytest.mark.parametrize("fused", [False, True], ids=["split4", "fused8"])
def test_deterministic_work_major(monkeypatch, fused):
    _deterministic(monkeypatch, 8, 2, 128, fused, head_major=False)


# --------------------------------------------------------------------------
# E. D=192 edges
# --------------------------------------------------------------------------

D192_CASES = (
    [(tb, t, 2, 2) for tb in ("klens", "qlens") for t in TYPES]
    + [("tall", "causal", 2, 2)]
)


@requires_gpu
@pytest.mark.parametrize("d", [192, 160])
@pytest.mark.parametrize(
    "case", D192_CASES, ids=lambda c: f"{c[0]}-{c[1]}-h{c[2]}{c[3]}"
)
def test_d192_edges(monkeypatch, case, d):
    table, tname, hq, hk = case
    got, hi, lo = _run(monkeypatch, table, tname, d, "narrow", hq=hq, hk=hk)
    _check(f"d{d}:{table}:{tname}", got, hi, lo, grad_ratio=D192_GRAD_RATIO)


@requires_gpu
def test_d192_gqa(monkeypatch):
    got, hi, lo = _run(monkeypatch, "klens", "causal", 192, "narrow", 4, 2)
    _check("d192:gqa", got, hi, lo, grad_ratio=D192_GRAD_RATIO)
