"""Direct 16-bit dQ/dK/dV stores of the dense backward on the GPU.

Why exact equality: both backward kernels accumulate a tile in registers over
their whole loop and write it once. With disjoint outer ranges every dQ
element has one owner, and with hq == hk every dK/dV element too. The default
path then adds that one f32 value into a zeroed f32 buffer (0 + x = x) and
the host casts the buffer to 16 bit, round to nearest even; the direct path
rounds the same f32 value the same way and stores it. So each case runs ONE
forward, then the backward twice on its result - flags off, then flags on -
and asks torch.equal of dq, dk and dv. Two equal wrong answers must not pass:
the flags-off gradients are also held to the fp64 oracle within the usual
budget (tests/util.assert_close_to_ref, lo = the 16-bit oracle with P rounded
to the element type; D=192 gradients at D192_GRAD_RATIO).

Inputs: tests/util.make_flex_case, seed 42, randn * 0.5, hq = hk = 2. The
16-bit buffers are reached through the Python layer only."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import make_attn_mask, ref_attn_with_grads  # noqa: E402
from tests.test_ffa_dense_paths_gpu import D192_GRAD_RATIO  # noqa: E402
from tests.util import assert_close_to_ref, make_flex_case  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP16, id="fp16")]
KNOBS = ("MAGI_BWD_BIGSEQ", "MAGI_BWD_DQ_BIGSEQ", "MAGI_BWD_FUSED_DKV",
         "MAGI_BWD_SPLIT_DKV", "MAGI_BWD_HEAD_MAJOR", "MAGI_BWD_COSCHED")

# name -> (tq, tk, q_ranges, k_ranges, types)
GEOM = {
    # 1: ragged last tiles in both passes
    "full160": (160, 160, [[0, 160]], [[0, 160]], [0]),
    # 2: two causal documents; k rows 224..255 are in no range with a query:
    #    the third slice has an empty q range over them
    "docs": (224, 256, [[0, 96], [96, 224], [224, 224]],
             [[0, 96], [96, 224], [224, 256]], [1, 1, 0]),
    # 3: inv-causal and bi-causal
    "inv_causal": (64, 128, [[0, 64]], [[0, 128]], [2]),
    "bi_causal": (64, 128, [[0, 64]], [[0, 128]], [3]),
    # 5: the distinct k ranges are disjoint, the q ranges overlap
    "merge": (128, 200, [[0, 64], [64, 128], [0, 128]],
              [[0, 100], [0, 100], [100, 200]], [0, 0, 0]),
    # 6: long enough for the 8-wave kernels once the knobs say 256
    "full320": (320, 320, [[0, 320]], [[0, 320]], [0]),
}


def _knobs(monkeypatch, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, str(val))


class _Case:
    """Inputs on the GPU, one forward (out, lse) and the two oracles."""


@functools.lru_cache(maxsize=None)
def _case(name, d, dtype, softcap=0.0, hq=2, hk=2) -> _Case:
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
    )

    tq, tk, qr_l, kr_l, ty_l = GEOM[name]
    c = _Case()
    c.tag = f"{name}-d{d}-{str(dtype)[6:]}" + (f"-cap{softcap}" if softcap else "")
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


def _backward(c, dq_direct, dkv_direct, dq=None, dk=None, dv=None,
              grad_type=None, **kw):
    """(dq, dk, dv) of one backward over the case's forward; grad_type names
    dq_type, dk_type and dv_type at once."""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_backward,
    )

    got = _flex_flash_attn_backward(
        dout=c.dout, q=c.q, k=c.k, v=c.v, sink=None, sink_layout="sh",
        out=c.out, lse=c.lse, dq=dq, dk=dk, dv=dv, dsink=None,
        q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
        softmax_scale=c.scale, softcap=c.softcap,
        dq_type=grad_type, dk_type=grad_type, dv_type=grad_type,
        disable_bwd_dkv_atomic_reduction=dkv_direct,
        disable_bwd_dq_atomic_reduction=dq_direct,
        deterministic=kw.pop("deterministic", False), sm_margin=0, **kw,
    )[:3]
    torch.cuda.synchronize()
    return got


def _off_then_on(c, dq_direct=True, dkv_direct=True, grad_ratio=3.0, **kw):
    """The backward with flags off, then on; bit equality of the two and
    oracle parity of the first. Returns the direct (dq, dk, dv)."""
    dtype = c.q.dtype
    off = _backward(c, False, False, **kw)
    on = _backward(c, dq_direct, dkv_direct, **kw)
    assert [t.dtype for t in off] == [F32] * 3
    assert [t.dtype for t in on] == [
        dtype if dq_direct else F32, *([dtype if dkv_direct else F32] * 2)
    ]
    for i, n in enumerate(("dq", "dk", "dv")):
        a, b = off[i].to(dtype), on[i].to(dtype)
        same = torch.equal(a, b)
        diff = (a.float() - b.float()).abs()
        print(f"    [{c.tag}:{n}] bit-equal={same} differing="
              f"{int((diff != 0).sum())} max abs diff={diff.max().item():.3e}")
        assert same, f"{c.tag}: direct {n} differs from the f32 path's cast"
        assert_close_to_ref(a.cpu(), c.hi[2 + i], c.lo[2 + i],
                            f"{c.tag}:{n}", ratio=grad_ratio)
    return on


# 1 - one full range, ragged last tiles
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_full_ragged(monkeypatch, d, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case("full160", d, dtype))


# the same at D=192: 4-wave dQ and the split dV / dK kernels
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_full_ragged_d192(monkeypatch, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case("full160", 192, dtype), grad_ratio=D192_GRAD_RATIO)


# 2 - two causal documents, uncovered k rows, an empty q range
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_causal_docs(monkeypatch, d, dtype):
    _knobs(monkeypatch)
    _, dk, dv = _off_then_on(_case("docs", d, dtype))
    assert (dk[224:] == 0).all() and (dv[224:] == 0).all(), (
        "k rows no query attends must come back exactly zero")


# 3 - inv-causal and bi-causal
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["inv_causal", "bi_causal"])
def test_mask_types(monkeypatch, name, d, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case(name, d, dtype))


# 4 - softcap
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_softcap(monkeypatch, d, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case("docs", d, dtype, softcap=15.0))


# 5 - auto_range_merge: dK/dV direct, dQ not (its ranges overlap)
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_auto_range_merge(monkeypatch, d, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case("merge", d, dtype), dq_direct=False,
                 auto_range_merge=True)


# 6 - the 8-wave kernels at small size, fused and split dK/dV; and the fused
#     4-wave kernel, which only an override reaches
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dkv", ["MAGI_BWD_FUSED_DKV", "MAGI_BWD_SPLIT_DKV"])
def test_eight_waves(monkeypatch, dkv, d, dtype):
    _knobs(monkeypatch, MAGI_BWD_BIGSEQ=256, MAGI_BWD_DQ_BIGSEQ=256,
           **{dkv: 1})
    _off_then_on(_case("full320", d, dtype))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_fused_four_waves(monkeypatch, d, dtype):
    _knobs(monkeypatch, MAGI_BWD_FUSED_DKV=1)
    _off_then_on(_case("full160", d, dtype))


# 7 - deterministic: disjoint ranges colour into one group, MHA has one split
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_deterministic(monkeypatch, d, dtype):
    _knobs(monkeypatch)
    _off_then_on(_case("docs", d, dtype), deterministic=True)


# 8 - a padded head dim through the public entry, both flags set
@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_head_dim_public_entry(monkeypatch, dtype):
    from magi_attention.functional import flex_flash_attn_func

    _knobs(monkeypatch)
    tq, tk, qr_l, kr_l, ty_l = GEOM["docs"]
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, 2, 2, 96, qr_l, kr_l, ty_l, dtype=dtype)
    grads = []
    for flag in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, _ = flex_flash_attn_func(
            *leaves, qr, kr, tm, disable_fwd_atomic_reduction=flag,
            disable_bwd_dkv_atomic_reduction=flag)
        out.backward(dout)
        torch.cuda.synchronize()
        grads.append([t.grad for t in leaves])
    mask = make_attn_mask(tq, tk, qr_l, kr_l, ty_l)
    qc, kc, vc, doc = (t.cpu() for t in (q, k, v, dout))
    hi = ref_attn_with_grads(qc.double(), kc.double(), vc.double(), mask,
                             doc.double())
    lo = ref_attn_with_grads(qc, kc, vc, mask, doc, high_precision=False,
                             p_dtype=dtype)
    for i, n in enumerate(("dq", "dk", "dv")):
        off, on = grads[0][i], grads[1][i]
        assert off.dtype == on.dtype == dtype and on.shape[-1] == 96
        assert torch.equal(off, on), f"d96:{n} differs bit for bit"
        assert_close_to_ref(off.cpu(), hi[2 + i], lo[2 + i], f"d96:{n}")


# ───────────── semantics: these fail on the parent commit ─────────────

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_flags_pick_the_gradient_dtypes(monkeypatch, dtype):
    _knobs(monkeypatch)
    c = _case("docs", 64, dtype)
    dq, dk, dv = _backward(c, False, True)
    assert (dq.dtype, dk.dtype, dv.dtype) == (F32, dtype, dtype)
    dq, dk, dv = _backward(c, True, False)
    assert (dq.dtype, dk.dtype, dv.dtype) == (dtype, F32, F32)
    # float32 asked for by name keeps the atomic path whatever the flags say
    dq, dk, dv = _backward(c, True, True, grad_type=F32)
    assert (dq.dtype, dk.dtype, dv.dtype) == (F32, F32, F32)
    dq, dk, dv = _backward(c, True, True, grad_type=dtype)
    assert (dq.dtype, dk.dtype, dv.dtype) == (dtype, dtype, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_callers_buffers_come_back(monkeypatch, dtype):
    _knobs(monkeypatch)
    c = _case("docs", 64, dtype)
    ref = _backward(c, True, True)
    mine = [torch.zeros_like(t) for t in (c.q, c.k, c.v)]
    got = _backward(c, True, True, dq=mine[0], dk=mine[1], dv=mine[2])
    for a, b, r in zip(got, mine, ref):
        assert a is b and a.dtype == dtype
        assert torch.equal(a, r)
    assert any(bool((t != 0).any()) for t in mine)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gqa_falls_back_to_f32(monkeypatch, dtype):
    """hq = 4, hk = 2: two q heads add into each dK/dV row, so the flag runs
    the f32 atomic path - accepted as before, f32 back. Two f32 values per
    element add up the same in either order, so the runs agree bit for bit."""
    _knobs(monkeypatch)
    c = _case("docs", 64, dtype, hq=4, hk=2)
    off = _backward(c, False, False)
    on = _backward(c, False, True)
    assert [t.dtype for t in on] == [F32] * 3
    for a, b, n in zip(off, on, ("dq", "dk", "dv")):
        assert torch.equal(a, b), n
    for i, n in enumerate(("dq", "dk", "dv")):
        assert_close_to_ref(off[i].to(dtype).cpu(), c.hi[2 + i], c.lo[2 + i],
                            f"{c.tag}:gqa:{n}")


@requires_gpu
def test_fp8_keeps_f32_accumulators(monkeypatch):
    """fp8 gradients are cast f32 -> fp8 once; the flag must not put a bf16
    rounding in between."""
    from magi_attention.functional import flex_flash_attn_func

    _knobs(monkeypatch)
    tq, tk, qr_l, kr_l, ty_l = GEOM["docs"]
    q, k, v, dout, qr, kr, tm = make_flex_case(
        tq, tk, 2, 2, 128, qr_l, kr_l, ty_l)
    fp8 = torch.float8_e4m3fn
    grads = []
    for flag in (False, True):
        leaves = [t.to(fp8).requires_grad_(True) for t in (q, k, v)]
        out, _ = flex_flash_attn_func(
            *leaves, qr, kr, tm, disable_bwd_dkv_atomic_reduction=flag)
        out.backward(dout)
        torch.cuda.synchronize()
        grads.append([t.grad for t in leaves])
    for a, b, n in zip(grads[0], grads[1], ("dq", "dk", "dv")):
        assert a.dtype == b.dtype == fp8
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), n
        assert bool((a.float() != 0).any()), n
