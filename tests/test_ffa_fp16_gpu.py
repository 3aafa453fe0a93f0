"""fp16 q/k/v through the dense forward and backward kernels on the GPU.

Inputs and oracles come from tests/fp16_cases.py: values exact in bf16 and
fp16, one fp64 oracle for both. Every parity check is
tests/util.assert_close_to_ref with its default ratio and floor against the
fp16-P oracle (lo16); D=192 gradients use D192_GRAD_RATIO of
tests/test_ffa_dense_paths_gpu.py. Rows with no key must have out exactly 0,
lse -inf and a zero dq.

lse, every case: the finite / -inf pattern equals the oracle's, and
max |lse - oracle| <= 2 x the bf16 kernels' lse error on the same case and
launch path + 1e-6. Both runs share inputs and all fp32 math; only the
accumulation inside the MFMA may differ.

Test 9 shows the kernels really compute in fp16: their rel-L2 error against
fp64 is at most half the bf16 kernels' on the same values. Three more
mantissa bits predict 1/8; tests/test_ffa_fp16_cpu.py asserts that the
fp16-P and bf16-P oracles are at least 4x apart. The ratios it and test 9
print, measured once, are in profiles/fp16_dense.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.fp16_cases import (  # noqa: E402
    BF16, FP16, PARITY_CASES, RATIO_CASES, reference, rel_l2,
)
from tests.test_ffa_dense_paths_gpu import (  # noqa: E402
    BUILDS, D192_GRAD_RATIO, _set_build,
)
from tests.util import assert_close_to_ref  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
NAMES = ("out", "lse", "dq", "dk", "dv")


def _tables(r):
    c = r.case
    i32 = dict(dtype=torch.int32, device="cuda")
    return (torch.tensor(c["qr"], **i32), torch.tensor(c["kr"], **i32),
            torch.tensor(c["ty"], **i32))


def _run(r, dtype=FP16, grad=True, with_sink=True, **kw):
    """flex_flash_attn_func on the case's values in dtype; returns out, lse,
    dq, dk, dv (and dsink, max_logits where asked for) on the CPU."""
    from magi_attention.functional import flex_flash_attn_func

    q, k, v = (t.to(dtype).cuda().requires_grad_(grad)
               for t in (r.q, r.k, r.v))
    sink = None
    if r.sink is not None and with_sink:
        sink = r.sink.cuda().requires_grad_(grad)
        kw.update(sink=sink, sink_layout=r.layout)
    if r.softcap:
        kw["softcap"] = r.softcap
    qr, kr, tm = _tables(r)
    with torch.set_grad_enabled(grad):
        out, meta = flex_flash_attn_func(q, k, v, qr, kr, tm, **kw)
    assert out.dtype == dtype and meta.lse.dtype == torch.float32
    got = {"out": out.detach().cpu(), "lse": meta.lse.detach().cpu()}
    if meta.max_logits is not None:
        got["max_logits"] = meta.max_logits.cpu()
    if grad:
        out.backward(r.dout.to(dtype).cuda())
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            assert t.grad.dtype == dtype
            got[n] = t.grad.cpu()
        if sink is not None:
            got["dsink"] = sink.grad.cpu()
    torch.cuda.synchronize()
    return got


def _check_lse(tag, lse, r, lse_bf16):
    hi = r.hi[1]
    fin = torch.isfinite(hi)
    assert torch.equal(torch.isfinite(lse), fin), f"{tag}: lse pattern"
    assert torch.equal(lse[~fin], hi[~fin]), f"{tag}: empty rows' lse"
    assert torch.equal(torch.isfinite(lse_bf16), fin)
    if not fin.any():
        return
    e16 = (lse[fin].double() - hi[fin].double()).abs().max().item()
    ebf = (lse_bf16[fin].double() - hi[fin].double()).abs().max().item()
    print(f"    [{tag}:lse] fp16 err={e16:.3e} bf16 err={ebf:.3e}")
    assert e16 <= 2 * ebf + 1e-6, f"{tag}: lse {e16:.3e} vs bf16 {ebf:.3e}"


def _check(tag, got, r, grad_ratio=3.0, **bf16_kw):
    """Parity of out, lse and whichever gradients got holds; the bf16 forward
    for the lse rule runs with the same arguments on the same launch path."""
    lse_bf16 = _run(r, BF16, grad=False, **bf16_kw)["lse"]
    _check_lse(tag, got["lse"], r, lse_bf16)
    dead_rows = r.dead
    for i, n in enumerate(NAMES):
        if n == "lse" or n not in got:
            continue
        g = got[n].float()
        assert torch.isfinite(g).all(), f"{tag}:{n} not finite"
        if n in ("out", "dq") and r.sink is None:
            assert (g[dead_rows] == 0).all(), (
                f"{tag}: rows without a key must have {n} = 0")
        assert_close_to_ref(g, r.hi[i], r.lo16[i], f"{tag}:{n}",
                            ratio=3.0 if n == "out" else grad_ratio)


# 1 ─ forward + backward parity on the edge geometries
@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", PARITY_CASES)
def test_fp16_parity(name, d):
    r = reference(name, d)
    _check(f"fp16:{r.name}", _run(r), r)


# 2 ─ D=192 and the padded d=160
@requires_gpu
@pytest.mark.parametrize("d", [192, 160])
def test_fp16_d192(d):
    r = reference("causal_200", d)
    _check(f"fp16:{r.name}", _run(r), r, grad_ratio=D192_GRAD_RATIO)


# 3 ─ the launch shapes: forward 4/8 waves, dQ 4/8 waves, fused and split
#     dK/dV (the builds of tests/test_ffa_dense_paths_gpu.py), and below the
#     8-wave forward on its 2-slot ring. Softcap (test 4) and the direct store
#     (test 5) run on the 4- and 8-wave builds too. Not reached: the fused
#     4-wave dK/dV and the D=192 8-wave forward, which no launcher picks
#     without an A/B override.
@requires_gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["overlap_q", "causal_unaligned"])
def test_fp16_launch_paths(monkeypatch, name, d, build):
    r = reference(name, d)
    bound = _set_build(monkeypatch, build)
    got = _run(r, max_seqlen_k=bound)
    _check(f"fp16:{r.name}:{build}", got, r, max_seqlen_k=bound)


@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_fwd_two_slot_ring(monkeypatch, d):
    """MAGI_FWD_NBUF=2: the 8-wave forward with the 2-slot staging ring."""
    r = reference("causal_unaligned", d)
    bound = _set_build(monkeypatch, "wide_fused")
    monkeypatch.setenv("MAGI_FWD_NBUF", "2")
    got = _run(r, max_seqlen_k=bound)
    _check(f"fp16:{r.name}:ring2", got, r, max_seqlen_k=bound)


# 4 ─ softcap
@requires_gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_fp16_softcap(monkeypatch, build):
    r = reference("causal_unaligned", 128, softcap=2.0)
    bound = _set_build(monkeypatch, build)
    got = _run(r, max_seqlen_k=bound)
    _check(f"fp16:{r.name}:softcap2:{build}", got, r, max_seqlen_k=bound)


# 5 ─ direct store
@requires_gpu
@pytest.mark.parametrize("build", ["wide_fused", "narrow"])
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_direct_store(monkeypatch, d, build):
    """short_and_long has disjoint q ranges: the kernel stores fp16 itself,
    bit-equal to the f32 merge path cast to fp16."""
    r = reference("short_and_long", d)
    bound = _set_build(monkeypatch, build)
    direct = _run(r, disable_fwd_atomic_reduction=True, max_seqlen_k=bound)
    merged = _run(r, grad=False, max_seqlen_k=bound)
    assert direct["out"].dtype == FP16
    assert torch.equal(direct["out"], merged["out"])
    assert torch.equal(direct["lse"], merged["lse"])
    _check(f"fp16:{r.name}:direct:{build}", direct, r,
           disable_fwd_atomic_reduction=True, max_seqlen_k=bound)


@requires_gpu
@pytest.mark.parametrize("layout", ["sh", "ssh"])
def test_fp16_direct_store_sink(layout):
    """Direct store + sink: the sink postprocess never sees fp16 (f32 out,
    cast once). Rows 190..255 are in no q range: out 0, lse = lse_sink."""
    r = reference(f"sink_{layout}", 128)
    direct = _run(r, disable_fwd_atomic_reduction=True)
    merged = _run(r, grad=False)
    assert direct["out"].dtype == FP16
    assert torch.equal(direct["out"], merged["out"])
    assert torch.equal(direct["lse"], merged["lse"])
    assert (direct["out"][190:] == 0).all()
    # f32 logsumexp of three logits of magnitude <= 8: a few ulp of 1e-6
    lse_sink = torch.logsumexp(r.sink.double(), dim=0 if layout == "sh" else 1)
    torch.testing.assert_close(
        direct["lse"][190:].double(), lse_sink.expand(256, -1)[190:],
        atol=1e-5, rtol=0)
    _check(f"fp16:{r.name}:direct", direct, r,
           disable_fwd_atomic_reduction=True)
    assert_close_to_ref(direct["dsink"], r.hi[5], r.lo16[5],
                        f"fp16:{r.name}:dsink")


# 6 ─ auto_range_merge
@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_auto_range_merge(d):
    r = reference("merge_3seg", d)
    _check(f"fp16:{r.name}:merge", _run(r, auto_range_merge=True), r,
           auto_range_merge=True)


# 7 ─ deterministic
@requires_gpu
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_deterministic(d):
    r = reference("overlap_q", d)
    a = _run(r, deterministic=True)
    b = _run(r, deterministic=True)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), f"{n} differs between two runs"
    _check(f"fp16:{r.name}:det", a, r, deterministic=True)


# 8 ─ max_logits, at the tolerance of tests/test_ffa_gpu.py test_max_logits
@requires_gpu
def test_fp16_max_logits():
    r = reference("max_logits", 128)
    got = _run(r, grad=False, return_max_logits=True)
    ml = got["max_logits"]
    assert ml.dtype == torch.float32 and ml.shape == (r.case["hq"],)
    c = r.case
    g = c["hq"] // c["hk"]
    kk = r.k.double().repeat_interleave(g, dim=1).permute(1, 0, 2)
    s = torch.matmul(r.q.double().permute(1, 0, 2), kk.transpose(-1, -2))
    s = (s * r.d ** -0.5).masked_fill(~r.mask.unsqueeze(0), float("-inf"))
    torch.testing.assert_close(ml, s.amax(dim=(-1, -2)).float(), atol=2e-2,
                               rtol=2e-2)


# 9 ─ really fp16
@requires_gpu
@pytest.mark.parametrize("name", RATIO_CASES)
def test_fp16_is_more_exact_than_bf16(name):
    r = reference(name, 128)
    f16, bf = _run(r, FP16), _run(r, BF16)
    for i, n in enumerate(NAMES):
        if n == "lse":
            continue
        e16, ebf = rel_l2(f16[n], r.hi[i]), rel_l2(bf[n], r.hi[i])
        print(f"    [fp16ratio:{r.name}:{n}] fp16={e16:.3e} bf16={ebf:.3e} "
              f"ratio={e16 / ebf:.3f}")
        assert e16 <= 0.5 * ebf, (n, e16, ebf)


# 10 ─ range: logits of std about 16
@requires_gpu
def test_fp16_large_logits():
    r = reference("range_96", 128, scale_qk=8)
    assert r.q.abs().max() > 8 and r.k.abs().max() > 8
    _check(f"fp16:{r.name}:x8", _run(r), r)


# 11 ─ the CP runtime at cp = 1
@requires_gpu
def test_fp16_calc_attn_cp1():
    """tests/test_dist_attn_gpu.py's sliding-window case with fp16 q/k/v."""
    from magi_attention.api import (
        calc_attn, dispatch, get_position_ids,
        infer_attn_mask_from_sliding_window, magi_attn_flex_key, undispatch,
    )
    from magi_attention.common.range import AttnRange
    from magi_attention.common.ranges import AttnRanges
    from magi_attention.config import DispatchConfig, DistAttnConfig
    from oracle import make_attn_mask, ref_attn_with_grads
    from tests.fp16_cases import grid_randn
    from tests.test_dist_attn_gpu import _init_pg

    total, hq, hk, d = 1024, 4, 2, 128
    group = _init_pg()
    qr, kr, tt = infer_attn_mask_from_sliding_window(
        AttnRange(0, total), AttnRange(0, total), (255, 0)
    )
    qranges = [[x.start, x.end] for x in qr]
    kranges = [[x.start, x.end] for x in kr]
    types = [t.to_int_type() for t in tt]
    key = magi_attn_flex_key(
        AttnRanges.from_ranges(qranges), AttnRanges.from_ranges(kranges),
        types, total, total, hq, hk, d, cp_group_or_mesh=group,
        dist_attn_config=DistAttnConfig(
            dispatch_config=DispatchConfig(chunk_size=256)
        ),
    )
    g = torch.Generator().manual_seed(3)
    q, k, v, dout = (grid_randn((total, h, d), g) for h in (hq, hk, hk, hq))
    ql, kl, vl = (dispatch(t.to(FP16).cuda(), key).requires_grad_(True)
                  for t in (q, k, v))
    out_l, meta_l = calc_attn(ql, kl, vl, key)
    out = undispatch(out_l, key)
    out_l.backward(dispatch(dout.to(FP16).cuda(), key))
    torch.cuda.synchronize()
    assert out.dtype == FP16 and meta_l.lse.dtype == torch.float32
    assert ql.grad.dtype == kl.grad.dtype == vl.grad.dtype == FP16

    mask = make_attn_mask(total, total, qranges, kranges, types)
    hi = ref_attn_with_grads(q.double(), k.double(), v.double(), mask,
                             dout.double())
    lo = ref_attn_with_grads(q.to(FP16), k.to(FP16), v.to(FP16), mask,
                             dout.to(FP16), high_precision=False,
                             p_dtype=FP16)
    assert_close_to_ref(out.cpu(), hi[0], lo[0], "fp16:cp1:out")
    pos = get_position_ids(key).cpu()

    def padded(t):
        return torch.cat(
            [t, torch.zeros(key.pad_size, *t.shape[1:], dtype=t.dtype)])[pos]

    for n, t, i in (("dq", ql, 2), ("dk", kl, 3), ("dv", vl, 4)):
        assert_close_to_ref(t.grad.cpu(), padded(hi[i]), padded(lo[i]),
                            f"fp16:cp1:{n}")
