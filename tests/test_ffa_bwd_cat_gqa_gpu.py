"""cat_gqa of the dense backward on the GPU: a dK/dV workgroup owns a KV head
and walks the q heads of its GQA group into one register tile.

What is asked of it:
  1. oracle parity of dq, dk and dv with cat_gqa=True on every dK/dV launch
     path (fused / split, 4 / 8 waves, head-major / work-major, D = 64 / 128 /
     192, softcap, fp16, a CU margin), at g = 2, 3 and 8 (MQA), within the
     usual budget (tests/util.assert_close_to_ref, ratio 3, lo = the 16-bit
     oracle with P rounded to the element type; D=192 at D192_GRAD_RATIO). The
     dq pass is untouched: dq is bit-equal to the cat-off dq.
  2. hq == hk: cat_gqa is the cat-off launch, bit for bit.
  3. the direct 16-bit dK/dV store under GQA. The argument for exact equality
     is the one of tests/test_ffa_bwd_direct_gpu.py: with cat_gqa and disjoint
     k ranges a dK/dV element has ONE register tile and ONE owner; the f32
     path adds that value into a zeroed buffer (0 + x = x) and the test casts
     it, the direct path rounds the same value the same way and stores it.
  4. deterministic: on k-disjoint tables each element is written once either
     way, so deterministic == not deterministic, bit for bit; with overlapping
     k ranges two deterministic runs agree bit for bit.
  5. the public entry, plain and with a padded head dim.
  6. the context-parallel runtime at cp = 1 with MAGI_ATTENTION_CATGQA=1.

Geometries, inputs (tests/util.make_flex_case, seed 42, randn * 0.5) and knob
handling are those of tests/test_ffa_bwd_direct_gpu.py; "gap" adds k rows that
are in no range at all. Each case runs ONE forward; every backward goes
through _flex_flash_attn_backward. Before a kernel result is held to a
budget, the 16-bit oracle itself is (a NaN or an all-zero oracle would make
the budget meaningless)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.test_ffa_bwd_direct_gpu import GEOM as _DIRECT_GEOM  # noqa: E402
from tests.test_ffa_bwd_direct_gpu import _knobs  # noqa: E402
from tests.test_ffa_dense_paths_gpu import D192_GRAD_RATIO  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
NAMES = ("dq", "dk", "dv")
HEADS = [pytest.param(4, 2, id="g2"), pytest.param(6, 2, id="g3"),
         pytest.param(8, 1, id="mqa")]
DKV = [pytest.param("MAGI_BWD_FUSED_DKV", id="fused"),
       pytest.param("MAGI_BWD_SPLIT_DKV", id="split")]

GEOM = dict(_DIRECT_GEOM)
# two causal documents; k rows 96..127 belong to no range
GEOM["gap"] = (224, 256, [[0, 96], [96, 224]], [[0, 96], [128, 256]], [1, 1])
# which tables run under auto_range_merge
MERGED = {"merge"}
# k rows that must come back exactly zero
ZERO_ROWS = {"docs": slice(224, 256), "gap": slice(96, 128)}


class _Case:
    """Inputs on the GPU, one forward (out, lse) and the two oracles."""


@functools.lru_cache(maxsize=None)
def _case(name, d, dtype, hq, hk, softcap=0.0) -> _Case:
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
    )

    tq, tk, qr_l, kr_l, ty_l = GEOM[name]
    c = _Case()
    c.name = name
    c.tag = (f"{name}-d{d}-{str(dtype)[6:]}-{hq}:{hk}"
             + (f"-cap{softcap}" if softcap else ""))
    c.q, c.k, c.v, c.dout, c.qr, c.kr, c.tm = make_flex_case(
        tq, tk, hq, hk, d, qr_l, kr_l, ty_l, dtype=dtype
    )
    c.softcap, c.scale = softcap, d ** -0.5
    out, meta = _flex_flash_attn_forward(
        q=c.q, k=c.k, v=c.v, sink=None, sink_layout="sh", out=None, lse=None,
        q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
        softmax_scale=c.scale, softcap=softcap, out_type=None,
        disable_fwd_atomic_reduction=False, deterministic=False, sm_margin=0,
    )
    c.out, c.lse = out.to(dtype), meta.lse
    torch.cuda.synchronize()
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    qc, kc, vc, doc = (t.cpu() for t in (c.q, c.k, c.v, c.dout))
    c.hi = ref_attn_with_grads(qc.double(), kc.double(), vc.double(), mask,
                               doc.double(), softcap=softcap)
    c.lo = ref_attn_with_grads(qc, kc, vc, mask, doc, softcap=softcap,
                               high_precision=False, p_dtype=dtype)
    return c


def _backward(c, cat, dkv_direct=False, sm_margin=0, **kw):
    """(dq, dk, dv) of one backward over the case's forward"""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_backward,
    )

    kw.setdefault("auto_range_merge", c.name in MERGED)
    got = _flex_flash_attn_backward(
        dout=c.dout, q=c.q, k=c.k, v=c.v, sink=None, sink_layout="sh",
        out=c.out, lse=c.lse, dq=None, dk=None, dv=None, dsink=None,
        q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
        softmax_scale=c.scale, softcap=c.softcap,
        dq_type=None, dk_type=None, dv_type=None,
        disable_bwd_dkv_atomic_reduction=dkv_direct,
        deterministic=kw.pop("deterministic", False), sm_margin=sm_margin,
        cat_gqa=cat, **kw,
    )[:3]
    torch.cuda.synchronize()
    return got


def _oracle_is_sound(c, ratio):
    """on the CPU: the 16-bit oracle is finite, non-zero and inside the budget
    the kernel is about to be held to"""
    for i, n in enumerate(NAMES):
        hi, lo = c.hi[2 + i], c.lo[2 + i]
        assert torch.isfinite(hi).all() and torch.isfinite(lo.float()).all()
        assert hi.norm() > 0, f"{c.tag}:{n}: the oracle gradient is all zero"
        assert_close_to_ref(lo, hi, lo, f"{c.tag}:oracle:{n}", ratio=ratio)


def _check_oracle(c, got, what, ratio=3.0):
    dtype = c.q.dtype
    for i, n in enumerate(NAMES):
        assert_close_to_ref(got[i].to(dtype).cpu(), c.hi[2 + i], c.lo[2 + i],
                            f"{c.tag}:{what}:{n}", ratio=ratio)


def _check_zero_rows(c, dk, dv):
    rows = ZERO_ROWS.get(c.name)
    if rows is not None:
        assert (dk[rows] == 0).all() and (dv[rows] == 0).all(), (
            f"{c.tag}: k rows no query attends must come back exactly zero")


def _parity(c, ratio=3.0, **kw):
    """cat off, then cat on: dq bit-equal, everything within the oracle
    budget. Returns the cat-on gradients."""
    _oracle_is_sound(c, ratio)
    off = _backward(c, False, **kw)
    on = _backward(c, True, **kw)
    assert [t.dtype for t in on] == [F32] * 3
    same = torch.equal(off[0], on[0])
    print(f"    [{c.tag}:dq] cat on bit-equal to cat off: {same}")
    assert same, f"{c.tag}: the dq pass must not see cat_gqa"
    _check_oracle(c, on, "cat", ratio)
    _check_zero_rows(c, on[1], on[2])
    return on


# 1 - oracle parity
@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkv", DKV)
@pytest.mark.parametrize(
    "name", ["full160", "docs", "inv_causal", "bi_causal", "merge"])
def test_parity(monkeypatch, name, dkv, d, hq, hk):
    _knobs(monkeypatch, **{dkv: 1})
    _parity(_case(name, d, BF16, hq, hk))


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("name", ["full160", "docs"])
def test_parity_d192(monkeypatch, name, hq, hk):
    _knobs(monkeypatch, MAGI_BWD_SPLIT_DKV=1)
    _parity(_case(name, 192, BF16, hq, hk), ratio=D192_GRAD_RATIO)


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkv", DKV)
def test_parity_eight_waves(monkeypatch, dkv, d, hq, hk):
    _knobs(monkeypatch, MAGI_BWD_BIGSEQ=256, MAGI_BWD_DQ_BIGSEQ=256,
           **{dkv: 1})
    _parity(_case("full320", d, BF16, hq, hk))


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("head_major", [0, 1])
@pytest.mark.parametrize("dkv", DKV)
def test_parity_grid_order(monkeypatch, dkv, head_major, hq, hk):
    _knobs(monkeypatch, MAGI_BWD_HEAD_MAJOR=head_major, **{dkv: 1})
    _parity(_case("docs", 128, BF16, hq, hk))
    # more than one k block per range: the block index is not always 0
    _knobs(monkeypatch, MAGI_BWD_HEAD_MAJOR=head_major, MAGI_BWD_BIGSEQ=256,
           **{dkv: 1})
    _parity(_case("full320", 64, BF16, hq, hk))


@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkv", DKV)
def test_parity_softcap(monkeypatch, dkv, d):
    """softcap 0.5 at the default scale: s / cap of order one, tanh bends"""
    _knobs(monkeypatch, **{dkv: 1})
    _parity(_case("docs", d, BF16, 6, 2, softcap=0.5))


@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkv", DKV)
def test_parity_fp16(monkeypatch, dkv, d):
    _knobs(monkeypatch, **{dkv: 1})
    _parity(_case("docs", d, FP16, 4, 2))


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("waves", [4, 8])
def test_parity_split_cu_margin(monkeypatch, waves, hq, hk):
    """sm_margin = 250 leaves 6 CUs: the split kernels' workgroups walk the
    flattened (kv head, k block, range) space with a stride"""
    _knobs(monkeypatch, MAGI_BWD_SPLIT_DKV=1,
           MAGI_BWD_BIGSEQ=256 if waves == 8 else 1 << 30)
    _parity(_case("full320" if waves == 8 else "docs", 64, BF16, hq, hk),
            sm_margin=250)


# 2 - a group of one head
@requires_gpu
@pytest.mark.parametrize("dkv", DKV)
def test_degenerate_group(monkeypatch, dkv):
    _knobs(monkeypatch, **{dkv: 1})
    c = _case("docs", 128, BF16, 2, 2)
    off = _backward(c, False)
    on = _backward(c, True)
    for a, b, n in zip(off, on, NAMES):
        assert torch.equal(a, b), f"{c.tag}: {n} differs with hq == hk"
    _check_oracle(c, on, "hq==hk")


# 3 - direct store under GQA: fails on the parent (raises or returns f32)
@requires_gpu
@pytest.mark.parametrize("hq,hk", [pytest.param(4, 2, id="g2"),
                                   pytest.param(8, 1, id="mqa")])
@pytest.mark.parametrize("dtype", [pytest.param(BF16, id="bf16"),
                                   pytest.param(FP16, id="fp16")])
@pytest.mark.parametrize("dkv", DKV)
@pytest.mark.parametrize("name", ["docs", "gap", "full160", "merge"])
def test_direct_store_under_gqa(monkeypatch, name, dkv, dtype, hq, hk):
    _knobs(monkeypatch, **{dkv: 1})
    c = _case(name, 128, dtype, hq, hk)
    _oracle_is_sound(c, 3.0)
    f32 = _backward(c, True, dkv_direct=False)
    on = _backward(c, True, dkv_direct=True)
    assert [t.dtype for t in f32] == [F32] * 3
    assert [t.dtype for t in on] == [F32, dtype, dtype], (
        "flag + cat_gqa must store dK/dV in the input dtype")
    for i in (1, 2):
        a, b = f32[i].to(dtype), on[i]
        same = torch.equal(a, b)
        diff = (a.float() - b.float()).abs()
        print(f"    [{c.tag}:{NAMES[i]}] bit-equal={same} differing="
              f"{int((diff != 0).sum())} max abs diff={diff.max().item():.3e}")
        assert same, f"{c.tag}: direct {NAMES[i]} differs from the f32 cast"
    _check_oracle(c, on, "cat+direct")
    _check_zero_rows(c, on[1], on[2])


@requires_gpu
def test_direct_store_under_gqa_eight_waves_d64(monkeypatch):
    _knobs(monkeypatch, MAGI_BWD_BIGSEQ=256, MAGI_BWD_SPLIT_DKV=1)
    c = _case("full320", 64, BF16, 6, 2)
    f32 = _backward(c, True)
    on = _backward(c, True, dkv_direct=True)
    assert [t.dtype for t in on] == [F32, BF16, BF16]
    for i in (1, 2):
        assert torch.equal(f32[i].to(BF16), on[i]), NAMES[i]
    _check_oracle(c, on, "cat+direct")


# 4 - deterministic
@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("dkv", DKV)
@pytest.mark.parametrize("name", ["docs", "full160"])
def test_deterministic_k_disjoint(monkeypatch, name, dkv, hq, hk):
    _knobs(monkeypatch, **{dkv: 1})
    c = _case(name, 128, BF16, hq, hk)
    _oracle_is_sound(c, 3.0)
    plain = _backward(c, True)
    det = _backward(c, True, deterministic=True)
    for i in (1, 2):
        same = torch.equal(plain[i], det[i])
        print(f"    [{c.tag}:{NAMES[i]}] deterministic bit-equal={same}")
        assert same, f"{c.tag}: deterministic {NAMES[i]} differs"
    _check_oracle(c, det, "cat+det")


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("dkv", DKV)
def test_deterministic_overlapping_k(monkeypatch, dkv, hq, hk):
    """merge without auto_range_merge: slices 0 and 1 share k rows 0..99 and
    colour into two k groups, launched one after the other"""
    _knobs(monkeypatch, **{dkv: 1})
    c = _case("merge", 64, BF16, hq, hk)
    _oracle_is_sound(c, 3.0)
    one = _backward(c, True, deterministic=True, auto_range_merge=False)
    two = _backward(c, True, deterministic=True, auto_range_merge=False)
    for a, b, n in zip(one, two, NAMES):
        assert torch.equal(a, b), f"{c.tag}: two deterministic {n} differ"
    _check_oracle(c, one, "cat+det+overlap")


# 5 - the public entry
@requires_gpu
@pytest.mark.parametrize("d", [128, 96], ids=["d128", "d96_padded"])
@pytest.mark.parametrize("direct", [False, True], ids=["f32", "direct"])
def test_public_entry(monkeypatch, direct, d):
    from magi_attention.functional import flex_flash_attn as ffa
    from magi_attention.functional import flex_flash_attn_func

    _knobs(monkeypatch)
    seen = []
    inner = ffa._flex_flash_attn_backward

    def spy(*a, **kw):
        got = inner(*a, **kw)
        seen.append((kw.get("cat_gqa"), got[1].dtype, got[2].dtype))
        return got

    monkeypatch.setattr(ffa, "_flex_flash_attn_backward", spy)
    tq, tk, qr_l, kr_l, ty_l = GEOM["docs"]
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, 4, 2, d, qr_l, kr_l, ty_l)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out, _ = flex_flash_attn_func(
        *leaves, qr, kr, tm, cat_gqa=True,
        disable_bwd_dkv_atomic_reduction=direct)
    out.backward(dout)
    torch.cuda.synchronize()
    # what _flex_flash_attn_backward handed back, before autograd's own cast
    assert seen == [(True, BF16, BF16) if direct else (True, F32, F32)]
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    qc, kc, vc, doc = (t.cpu() for t in (q, k, v, dout))
    hi = ref_attn_with_grads(qc.double(), kc.double(), vc.double(), mask,
                             doc.double())
    lo = ref_attn_with_grads(qc, kc, vc, mask, doc, high_precision=False,
                             p_dtype=BF16)
    for i, n in enumerate(NAMES):
        g = leaves[i].grad
        assert g.dtype == BF16 and g.shape[-1] == d
        assert_close_to_ref(g.cpu(), hi[2 + i], lo[2 + i], f"public:d{d}:{n}")


# 6 - the context-parallel runtime at cp = 1
@requires_gpu
def test_cp1_env_flag(monkeypatch):
    from magi_attention.api import calc_attn, dispatch, magi_attn_flex_key
    from magi_attention.common.ranges import AttnRanges
    from magi_attention.config import DispatchConfig, DistAttnConfig
    from magi_attention.functional import _ffa_launch
    from tests.test_dist_attn_gpu import _init_pg

    _knobs(monkeypatch)
    group = _init_pg()
    total, hq, hk, d = 1536, 4, 2, 128
    ranges = [[0, 512], [512, 1280], [1280, 1536]]
    types = [1, 1, 0]
    g = torch.Generator().manual_seed(3)
    q, k, v, dout = (
        (torch.randn(total, h, d, generator=g) * 0.5).bfloat16().cuda()
        for h in (hq, hk, hk, hq))
    seen = []
    inner = _ffa_launch.bwd_args

    def spy(*a, **kw):
        seen.append(bool(kw.get("cat_gqa")))
        return inner(*a, **kw)

    monkeypatch.setattr(_ffa_launch, "bwd_args", spy)

    def run(flag):
        if flag:
            monkeypatch.setenv("MAGI_ATTENTION_CATGQA", "1")
        else:
            monkeypatch.delenv("MAGI_ATTENTION_CATGQA", raising=False)
        key = magi_attn_flex_key(
            AttnRanges.from_ranges(ranges), AttnRanges.from_ranges(ranges),
            types, total, total, hq, hk, d, cp_group_or_mesh=group,
            dist_attn_config=DistAttnConfig(
                dispatch_config=DispatchConfig(chunk_size=256)),
        )
        leaves = [dispatch(t, key).requires_grad_(True) for t in (q, k, v)]
        out_l, _ = calc_attn(*leaves, key)
        del seen[:]
        out_l.backward(dispatch(dout, key))
        torch.cuda.synchronize()
        # dpsum-only structs aside, every backward struct carries the flag
        assert seen and any(seen) == flag, seen
        return [t.grad for t in leaves], key

    off, key = run(False)
    on, _ = run(True)
    # budget: the 16-bit oracle's own error against fp64, in dispatched order
    from magi_attention.api import get_position_ids

    mask = make_attn_mask(total, total, ranges, ranges, types)
    qc, kc, vc, doc = (t.cpu() for t in (q, k, v, dout))
    hi = ref_attn_with_grads(qc, kc, vc, mask, doc)
    lo = ref_attn_with_grads(qc, kc, vc, mask, doc, high_precision=False,
                             p_dtype=BF16)
    pos = get_position_ids(key).cpu()

    def padded(t):
        pad = torch.zeros(key.pad_size, *t.shape[1:], dtype=t.dtype)
        return torch.cat([t, pad]).float()[pos]

    for i, n in enumerate(NAMES):
        assert_close_to_ref(on[i].cpu().float(), padded(hi[2 + i]),
                            padded(lo[2 + i]), f"cp1:cat:{n}")
        # and against the same call with the flag unset, at that same budget
        assert_close_to_ref(on[i].cpu().float(), off[i].cpu().float(),
                            off[i].cpu().float()
                            + (padded(lo[2 + i]) - padded(hi[2 + i])),
                            f"cp1:cat-vs-off:{n}")
