"""pack_gqa of the dense forward on the GPU: a workgroup owns a KV head and
packs the (token, q head) pairs of its GQA group into its 32-row q tiles.

_flex_flash_attn_forward(pack_gqa=True) against the fp64 oracle: out within
tests/util.assert_close_to_ref (ratio 3, floor 3e-3, lo = the 16-bit oracle
with P rounded to the element type), lse as tests/test_fwd_dq_prefetch_gpu.py
(-inf pattern equal, then atol=5e-3, rtol=1e-3); rows in no range or with no
key keep out = 0 and lse = -inf. No bit-equality with the unpacked launch is
claimed when hq != hk. Geometries (smallest shapes that reach each seam):
  odd      11 tokens x 40 keys: at G=3 R=33, wave 1 has one live row and
           token 10's heads split across waves
  docs     causal documents of 11 and 53 tokens; the second has 40 keys, so
           its first 13 tokens have none; k rows 11..19 are in no range
  blocks   tq=96 in q blocks of 16 with 2-3 disjoint k blocks of 32, full and
           causal mixed, under auto_range_merge: the segment loop
  overlap  q ranges [0,48) twice and [24,72) in merge mode (locks over
           several heads); tokens 72..79 are in no range
  long     150 tokens: more than one block at 4 and 8 waves, lock slot 128
max_logits is an exact maximum of fp32-accumulated bf16 products: 1e-4."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn, ref_attn_with_grads  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
HEADS = [pytest.param(4, 2, id="g2"), pytest.param(6, 2, id="g3"),
         pytest.param(8, 1, id="mqa")]
_BLK = [(i, (i + j) % 4, (i + j) % 2) for i in range(6) for j in range(2 + i % 2)]
GEOM = {  # tq, tk, q ranges, k ranges, types (None: the test's own)
    "odd": (11, 40, [[0, 11]], [[0, 40]], None),
    "docs": (64, 64, [[0, 11], [11, 64]], [[0, 11], [20, 60]], [1, 1]),
    "blocks": (96, 128, [[16 * i, 16 * i + 16] for i, _, _ in _BLK],
               [[32 * b, 32 * b + 32] for _, b, _ in _BLK],
               [t for _, _, t in _BLK]),
    "overlap": (80, 160, [[0, 48], [0, 48], [24, 72]],  # no (q, k) pair twice
                [[0, 32], [32, 96], [96, 160]], [0, 1, 0]),
    "long": (150, 200, [[0, 150]], [[0, 200]], None),
}
DEAD = {"docs": 13, "overlap": 8}  # tokens without a key
ALL = [("odd", 0), ("odd", 1), ("odd", 2), ("odd", 3), ("docs", 1),
       ("blocks", 0), ("overlap", 0), ("long", 2), ("long", 3)]
SOME = [("odd", 1), ("blocks", 0), ("long", 3)]
VARIANTS = {"d64": dict(d=64), "d192": dict(d=192), "fp16": dict(dtype=FP16),
            "softcap": dict(softcap=0.5), "w4": dict(MAGI_FWD_WAVES=4),
            "w8": dict(MAGI_FWD_WAVES=8), "workmajor": dict(MAGI_FWD_HEADMAJOR=0),
            "margin": dict(sm_margin=200)}


@functools.lru_cache(maxsize=None)
def _case(name, atype, hq, hk, d=128, dtype=BF16, softcap=0.0, sink=False):
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


def _run(c, pack=True, **kw):
    from magi_attention.functional import flex_flash_attn as ffa

    tabs = (c.qr, c.kr, c.tm, None)
    if c.name == "blocks":
        tabs = ffa._merged_tables(c.qr, c.kr, c.tm)
    args = dict(q=c.q, k=c.k, v=c.v, sink=c.sink, sink_layout="sh", out=None,
                lse=None, q_ranges=tabs[0], k_ranges=tabs[1],
                attn_type_map=tabs[2], qk_starts=tabs[3],
                softmax_scale=c.scale, softcap=c.softcap, out_type=None,
                disable_fwd_atomic_reduction=False, deterministic=False,
                sm_margin=0, pack_gqa=pack)
    args.update(kw)
    out, meta = ffa._flex_flash_attn_forward(**args)
    torch.cuda.synchronize()
    return out, meta


def _check(c, out, meta, what="pack"):
    out, lse = out.cpu(), meta.lse.cpu()
    dead = torch.isinf(c.hi[1])
    if c.sink is None:  # with a sink a row without a key has lse = lse_sink
        assert dead.sum() == DEAD.get(c.name, 0) * lse.shape[1]
        assert (out[dead] == 0).all(), f"{c.tag}: rows without a key: out"
    assert torch.equal(torch.isinf(lse) & (lse < 0), dead), f"{c.tag}: -inf"
    torch.testing.assert_close(lse[~dead], c.hi[1][~dead], atol=5e-3, rtol=1e-3)
    assert torch.isfinite(out).all()
    assert_close_to_ref(out.to(c.q.dtype), c.hi[0], c.lo[0], f"{c.tag}:{what}")


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
@pytest.mark.parametrize("name,atype", ALL)
def test_parity(monkeypatch, name, atype, hq, hk):
    for knob in ("MAGI_FWD_WAVES", "MAGI_FWD_HEADMAJOR", "MAGI_FWD_NBUF"):
        monkeypatch.delenv(knob, raising=False)
    c = _case(name, atype, hq, hk)
    _check(c, *_run(c))


@requires_gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,atype", SOME)
def test_variants(monkeypatch, name, atype, variant):
    kw = dict(VARIANTS[variant])
    for knob in [k for k in kw if k.startswith("MAGI_")]:
        monkeypatch.setenv(knob, str(kw.pop(knob)))
    margin = kw.pop("sm_margin", 0)
    c = _case(name, atype, 6, 2, **kw)
    _check(c, *_run(c, sm_margin=margin), what=variant)


@requires_gpu
@pytest.mark.parametrize("out16", [True, False], ids=["16bit", "f32"])
@pytest.mark.parametrize("name", ["docs", "blocks"])
def test_direct_store(name, out16):
    c = _case(name, 1, 6, 2)
    out, meta = _run(c, disable_fwd_atomic_reduction=True,
                     out_type=BF16 if out16 else F32)
    assert out.dtype == (BF16 if out16 else F32)
    _check(c, out, meta, "direct")


@requires_gpu
@pytest.mark.parametrize("hq,hk", HEADS)
def test_deterministic_overlap(hq, hk):
    c = _case("overlap", 0, hq, hk)
    a, b = _run(c, deterministic=True), _run(c, deterministic=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].lse, b[1].lse)
    _check(c, *a, what="det")


@requires_gpu
@pytest.mark.parametrize("softcap", [0.0, 0.5])
@pytest.mark.parametrize("name,atype", [("odd", 1), ("blocks", 0), ("overlap", 0)])
def test_max_logits(name, atype, softcap):
    from magi_attention.functional import _ffa_launch

    c = _case(name, atype, 6, 2, softcap=softcap)
    out, meta = _run(c, max_logits=_ffa_launch.new_max_logits(6, c.q.device))
    _check(c, out, meta, "max_logits")
    kk = c.k.cpu().double().repeat_interleave(3, dim=1).permute(1, 2, 0)
    s = torch.matmul(c.q.cpu().double().permute(1, 0, 2), kk) * c.scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    ref = s.masked_fill(~c.mask, float("-inf")).amax(dim=(-1, -2)).float()
    torch.testing.assert_close(meta.max_logits.cpu(), ref, atol=1e-4, rtol=1e-4)


@requires_gpu
def test_sink():
    c = _case("docs", 1, 6, 2, sink=True)
    _check(c, *_run(c), what="sink")


@requires_gpu
def test_direct_launch():
    """_ffa_launch.fwd(pack_gqa=True): a TypeError on the parent commit"""
    from magi_attention.functional import _ffa_launch
    from magi_attention.functional.flex_flash_attn import _get_locks

    c = _case("long", 3, 6, 2)
    out = torch.zeros(150, 6, 128, dtype=F32, device="cuda")
    lse = torch.full((150, 6), float("-inf"), device="cuda")
    _ffa_launch.fwd(
        c.q, c.k, c.v, out, lse, c.qr, c.kr, c.tm,
        locks=_get_locks(150, 6, out.device), max_logits=None, qk_starts=None,
        max_seqlen_q=150, softmax_scale=c.scale, softcap=0.0,
        disable_fwd_atomic_reduction=False, sm_margin=0, deterministic=False,
        pack_gqa=True)
    torch.cuda.synchronize()
    _check(c, out, type("Meta", (), {"lse": lse}), "launch")


@requires_gpu
def test_group_of_one_head_is_the_unpacked_launch():
    c = _case("overlap", 0, 2, 2)
    on, off = _run(c, deterministic=True), _run(c, False, deterministic=True)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1].lse, off[1].lse)
    _check(c, *on, what="hq==hk")


@requires_gpu
def test_public_entry_padded_head_dim_with_grads():
    from magi_attention.functional import flex_flash_attn_func

    tq, tk, qr_l, kr_l, ty_l = GEOM["blocks"]
    q, k, v, dout, qr, kr, tm = make_flex_case(tq, tk, 6, 2, 96, qr_l, kr_l, ty_l)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out, meta = flex_flash_attn_func(*leaves, qr, kr, tm, pack_gqa=True,
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
