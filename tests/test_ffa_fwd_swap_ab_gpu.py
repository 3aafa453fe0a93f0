"""swap_ab of the dense forward on the GPU: the four waves of a workgroup
split the k loop of QT = 1 or 2 32-row q tiles (KS = 4 / QT waves per tile,
32 * KS k rows per stage) and merge their softmax states in LDS.

_flex_flash_attn_forward(swap_ab=True) against the fp64 oracle, budgets as
tests/test_ffa_fwd_pack_gpu.py. Geometries, each with QT forced to 1 and 2:
  odd      11 q x 40 k: a partial q tile; the stage is longer than the range,
           so the last waves merge an empty (-inf) partial
  tail     32 q x 200 k: the second 128-row stage holds 72 rows
  two      53 q x 150 k: at QT = 2 the second tile is partial and the tiles'
           k bounds differ (a sub-tile dead for one tile, live for the other)
  docs     causal documents of 11 and 53 tokens; 13 tokens have no key
  blocks   q blocks of 16 with 2-3 k blocks of 32, full and causal, merged
           tables: wave 0's state carried across segments, the rest empty
  wide     q blocks of 16 with two k blocks of 80, full and causal, merged
           tables: every wave's partial is live and carried across segments
  overlap  q ranges [0,48) twice and [24,72), merge mode: locks
  long     150 q x 200 k: several blocks per range, lock slot 128"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from magi_attention.functional._ffa_launch import (  # noqa: E402
    new_max_logits, swap_ab_active)
from oracle import make_attn_mask, ref_attn, ref_attn_with_grads  # noqa: E402
from tests.test_ffa_fwd_pack_gpu import _check  # noqa: E402  (same budgets)
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
_BLK = [(i, (i + j) % 4, (i + j) % 2) for i in range(6) for j in range(2 + i % 2)]
_WIDE = [(i, (i + j) % 3) for i in range(3) for j in range(2)]
GEOM = {  # tq, tk, q ranges, k ranges, types (None: the test's own)
    "odd": (11, 40, [[0, 11]], [[0, 40]], None),
    "tail": (32, 200, [[0, 32]], [[0, 200]], None),
    "two": (53, 150, [[0, 53]], [[0, 150]], None),
    "docs": (64, 64, [[0, 11], [11, 64]], [[0, 11], [20, 60]], [1, 1]),
    "blocks": (96, 128, [[16 * i, 16 * i + 16] for i, _, _ in _BLK],
               [[32 * b, 32 * b + 32] for _, b, _ in _BLK],
               [t for _, _, t in _BLK]),
    "wide": (48, 240, [[16 * i, 16 * i + 16] for i, _ in _WIDE],
             [[80 * b, 80 * b + 80] for _, b in _WIDE], [0, 1] * 3),
    "overlap": (80, 160, [[0, 48], [0, 48], [24, 72]],  # no (q, k) pair twice
                [[0, 32], [32, 96], [96, 160]], [0, 1, 0]),
    "long": (150, 200, [[0, 150]], [[0, 200]], None),
}
DEAD = {"docs": 13, "overlap": 8}  # tokens without a key
ALL = [("odd", 0), ("odd", 1), ("odd", 2), ("odd", 3), ("tail", 0), ("tail", 1),
       ("two", 1), ("two", 3), ("docs", 1), ("blocks", 0), ("wide", 0),
       ("overlap", 0), ("long", 2), ("long", 3)]
SOME = [("odd", 1), ("two", 3), ("docs", 1), ("wide", 0)]  # disjoint q ranges
VARIANTS = {"d64": dict(d=64), "fp16": dict(dtype=FP16),
            "softcap": dict(softcap=0.5), "margin": dict(sm_margin=200),
            "workmajor": dict(MAGI_FWD_HEADMAJOR=0), "gqa": dict(hq=4, hk=2),
            "sink": dict(sink=True), "direct16": dict(direct=BF16),
            "directf32": dict(direct=F32)}


@functools.lru_cache(maxsize=None)
def _case(name, atype, hq=2, hk=2, d=128, dtype=BF16, softcap=0.0, sink=False):
    """Inputs on the GPU and the two oracles, after checking on the CPU that
    the geometry holds what the table claims and that the oracle is sound."""
    tq, tk, qr_l, kr_l, ty_l = GEOM[name]
    ty_l = ty_l or [atype]
    c = type("Case", (), {})()
    c.name, c.softcap, c.scale = name, softcap, d ** -0.5
    c.tag = f"{name}{atype}-{hq}:{hk}-d{d}-{str(dtype)[6:]}"
    c.q, c.k, c.v, c.dout, c.qr, c.kr, c.tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l, dtype=dtype)
    c.mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    assert int((~c.mask.any(1)).sum()) == DEAD.get(name, 0), name
    g = torch.Generator().manual_seed(7)
    c.sink = torch.randn(2, hq, generator=g).cuda() if sink else None
    qc, kc, vc = c.q.cpu(), c.k.cpu(), c.v.cpu()
    kw = dict(softcap=softcap, sink=None if c.sink is None else c.sink.cpu())
    c.hi = ref_attn(qc.double(), kc.double(), vc.double(), c.mask, **kw)
    c.lo = ref_attn(qc, kc, vc, c.mask, high_precision=False, p_dtype=dtype, **kw)
    assert torch.isfinite(c.hi[0]).all() and c.hi[0].norm() > 0
    assert torch.isfinite(c.lo[0].float()).all()
    return c


def _run(c, swap_ab=True, **kw):
    from magi_attention.functional import flex_flash_attn as ffa

    tabs = (c.qr, c.kr, c.tm, None)
    if c.name in ("blocks", "wide"):
        tabs = ffa._merged_tables(c.qr, c.kr, c.tm)
    args = dict(q=c.q, k=c.k, v=c.v, sink=c.sink, sink_layout="sh", out=None,
                lse=None, q_ranges=tabs[0], k_ranges=tabs[1],
                attn_type_map=tabs[2], qk_starts=tabs[3],
                softmax_scale=c.scale, softcap=c.softcap, out_type=None,
                disable_fwd_atomic_reduction=False, deterministic=False,
                sm_margin=0, swap_ab=swap_ab)
    args.update(kw)
    out, meta = ffa._flex_flash_attn_forward(**args)
    torch.cuda.synchronize()
    return out, meta


@pytest.fixture
def knobs(monkeypatch):
    for knob in ("MAGI_FWD_WAVES", "MAGI_FWD_HEADMAJOR", "MAGI_FWD_NBUF",
                 "MAGI_FWD_SPLITK_QT"):
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


@requires_gpu
@pytest.mark.parametrize("qt", [1, 2])
@pytest.mark.parametrize("name,atype", ALL)
def test_parity(knobs, name, atype, qt):
    knobs.setenv("MAGI_FWD_SPLITK_QT", str(qt))
    c = _case(name, atype)
    _check(c, *_run(c), what=f"qt{qt}")


@requires_gpu
@pytest.mark.parametrize("qt", [0, 1], ids=["qt-unset", "qt1"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,atype", SOME)
def test_variants(knobs, name, atype, variant, qt):
    if qt:
        knobs.setenv("MAGI_FWD_SPLITK_QT", str(qt))
    kw = dict(VARIANTS[variant])
    for knob in [k for k in kw if k.startswith("MAGI_")]:
        knobs.setenv(knob, str(kw.pop(knob)))
    run_kw = dict(sm_margin=kw.pop("sm_margin", 0))
    direct = kw.pop("direct", None)
    if direct is not None:
        run_kw.update(disable_fwd_atomic_reduction=True, out_type=direct)
    c = _case(name, atype, **kw)
    out, meta = _run(c, **run_kw)
    assert out.dtype == (direct or F32)
    _check(c, out, meta, what=variant)


@requires_gpu
def test_deterministic_overlap(knobs):
    c = _case("overlap", 0)
    a, b = _run(c, deterministic=True), _run(c, deterministic=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].lse, b[1].lse)
    _check(c, *a, what="det")


@requires_gpu
@pytest.mark.parametrize("softcap", [0.0, 0.5])
@pytest.mark.parametrize("name,atype", [("tail", 1), ("two", 3), ("wide", 0)])
def test_max_logits(knobs, name, atype, softcap):
    c = _case(name, atype, softcap=softcap)
    out, meta = _run(c, max_logits=new_max_logits(2, c.q.device))
    _check(c, out, meta, "max_logits")
    s = torch.matmul(c.q.cpu().double().permute(1, 0, 2),
                     c.k.cpu().double().permute(1, 2, 0)) * c.scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    ref = s.masked_fill(~c.mask, float("-inf")).amax(dim=(-1, -2)).float()
    torch.testing.assert_close(meta.max_logits.cpu(), ref, atol=1e-4, rtol=1e-4)


@requires_gpu
@pytest.mark.parametrize("what", ["d192", "pack_gqa", "sparse_load"])
def test_fallbacks_equal_the_flag_off(knobs, what):
    """Where swap_ab_active says no, the flag changes nothing, bit for bit."""
    assert swap_ab_active(True, BF16, 128, False, False)
    c = _case("blocks", 0, 4, 2, d=192 if what == "d192" else 128)
    # merged tables: unique q ranges, here disjoint, so one writer per row
    kw = dict(pack_gqa=what == "pack_gqa", sparse_load=what == "sparse_load")
    if what == "sparse_load":  # full blocks only
        kw.update(attn_type_map=torch.zeros_like(c.tm))
    assert not swap_ab_active(True, BF16, c.q.shape[2], kw["pack_gqa"],
                              kw["sparse_load"])
    on, off = _run(c, True, **kw), _run(c, False, **kw)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1].lse, off[1].lse)
    assert torch.isfinite(on[0]).all() and on[0].abs().sum() > 0


@requires_gpu
def test_public_entry_padded_head_dim_with_grads(knobs):
    from magi_attention.functional import flex_flash_attn_func

    tq, tk, qr_l, kr_l, ty_l = GEOM["wide"]
    q, k, v, dout, qr, kr, tm = make_flex_case(tq, tk, 2, 2, 96, qr_l, kr_l, ty_l)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out, meta = flex_flash_attn_func(*leaves, qr, kr, tm, swap_ab=True,
                                     auto_range_merge=True)
    out.backward(dout)
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    cpu = [t.cpu() for t in (q, k, v)]
    hi = ref_attn_with_grads(*(t.double() for t in cpu), mask, dout.cpu().double())
    lo = ref_attn_with_grads(*cpu, mask, dout.cpu(), high_precision=False,
                             p_dtype=BF16)
    assert torch.isfinite(hi[0]).all() and hi[0].norm() > 0
    torch.testing.assert_close(meta.lse.cpu(), hi[1].float(), atol=5e-3, rtol=1e-3)
    got = [out.detach()] + [t.grad for t in leaves]
    for g, i, n in zip(got, (0, 2, 3, 4), ("out", "dq", "dk", "dv")):
        assert g.shape[-1] == 96
        assert_close_to_ref(g.cpu(), hi[i], lo[i], f"public:d96:{n}")
