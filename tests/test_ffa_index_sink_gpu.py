"""GPU parity tests for the attention sink and max_logits on the index
(token-gather) path: flex_flash_attn_func(q, k, v, index_attn_indices=...,
sink=..., sink_layout=..., return_max_logits=...), forward and backward, bf16
(csrc/ffa_index.hip) and fp8 (csrc/ffa_index_fp8.hip).

Oracle: the gather-based PyTorch attention of tests/test_ffa_index_bwd_gpu.py
(copied, not imported), extended: the sink logits are concatenated as extra
score columns before the softmax and dropped before the PV product, the lse
runs over keys plus sink, and autograd gives dsink. Evaluated in fp64
(ref_hi) and in bf16 (ref_lo); for the fp8 forward ref_lo is the fp32 oracle
with P rounded to e4m3 (tests/test_ffa_index_fp8_gpu.py). Sink logits are
randn * 2 + 2: their mass is comparable to a 48-key row, so a dropped sink
moves out by tens of percent.

Budgets (none of them taken from the kernel under test):
  out, dq, dk, dv, dsink  tests/util.py::assert_close_to_ref, default ratio
                          and floor (3 x the bf16 oracle's own error);
  lse                     atol=3e-2, rtol=3e-3 against fp64 (the index tests'
                          lse tolerance);
  max_logits              atol=2e-2, rtol=2e-2 against the fp64 per-head
                          maximum over valid slots (tests/test_ffa_gpu.py::
                          test_max_logits);
  fp8                     out: default ratio against the e4m3-P oracle; lse as
                          above; dq/dk/dv/dsink ratio=4.5, floor=9e-2
                          (tests/test_ffa_index_fp8_gpu.py);
  index vs range path     out within twice the bf16-oracle budget of the case,
                          lse within the lse tolerance.

Measured on an MI355X (worst case of each group; per-case figures are printed
by the tests and tabulated in profiles/r5_index_sink.md):
  bf16 sink fwd+bwd (36 cases, softcap included)
      out 2.3e-3 (budget >= 1.0e-2), dq 2.5e-3 (>= 1.4e-2), dk 2.5e-3
      (>= 1.5e-2), dv 2.4e-3 (>= 1.2e-2), dsink 3.1e-3 (>= 5.7e-3; worst
      err/budget 0.20), lse max abs err 1.0e-6
  all-padding rows    out/dq/dk/dv 2.5e-3, dsink 3.4e-3 (>= 1.6e-2), lse 6e-7
  max_logits          max abs err 8.0e-7 bf16, 1.9e-5 fp8 (atol 2e-2); out and
                      grads with the flag on no worse than with it off (out
                      2.06e-3..2.20e-3 on against 2.15e-3..2.24e-3 off)
  fp8                 out 2.5e-2 (>= 9.9e-2), dq 2.9e-2, dk 2.7e-2, dv 2.7e-2,
                      dsink 2.7e-2 (floor 9e-2), lse 2.0e-6
  index vs range      out rel-L2 diff 8.3e-6 / 4.1e-6 (budget 3.1e-2 /
                      3.7e-2), lse diff 0.0
On the parent commit (sink ignored, max_logits None) cases 1-6 and 8 fail:
out is 2.4e-1 .. 4.7 rel-L2 off (cases 1, 2, 3, 5), meta.max_logits is None
(cases 4, 5, 8), the index and range paths differ by 3.0e-1 / 1.7 in out and
1.8 / 2.6 in lse (case 6). Case 7 passes there by design.

All tensors use the folded layout the kernel takes: q [(b s h_kv), ratio, d],
k/v [(b s h_kv), 1, d], global id = (b*S_kv + t)*NHK + h_kv; "sh" sink is
[s_sink, ratio], "ssh" sink is [(b s h_kv), s_sink, ratio].
"""
import pytest
import torch

from tests.util import FLOOR, MISMATCH_RATIO, assert_close_to_ref

pytestmark = pytest.mark.gpu

from magi_attention.utils import build_index_attn_indices  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

FP8 = torch.float8_e4m3fn
LSE_ATOL, LSE_RTOL = 3e-2, 3e-3
ML_ATOL, ML_RTOL = 2e-2, 2e-2
GRAD_RATIO, GRAD_FLOOR = 4.5, 9e-2  # fp8 gradients

# smallest shapes that reach every branch: a half-valid second 32-row subtile
# with a -1 tail (topk 48 of 64); W=4, W=1 with a full wave, a partial wave;
# D=64; D=96 through the pad route; several gathered tiles per row
SHAPES = {
    "r128": dict(B=2, S_q=33, S_kv=128, ratio=128, nhk=1, D=128, topk=48,
                 max_topk=64),
    "r32x2": dict(B=2, S_q=33, S_kv=128, ratio=32, nhk=2, D=128, topk=48,
                  max_topk=64),
    "r8": dict(B=2, S_q=33, S_kv=128, ratio=8, nhk=1, D=128, topk=48,
               max_topk=64),
    "d64": dict(B=2, S_q=33, S_kv=128, ratio=32, nhk=1, D=64, topk=48,
                max_topk=64),
    "d96": dict(B=2, S_q=33, S_kv=128, ratio=32, nhk=1, D=96, topk=48,
                max_topk=64),
    "multi": dict(B=2, S_q=16, S_kv=256, ratio=64, nhk=1, D=128,
                  topk=[17, 192], max_topk=256),
}
SINKS = [("sh", 1), ("sh", 8), ("ssh", 3)]


def _sink_cols(sink, layout, T):
    """sink logits as score columns [T, H, s_sink]"""
    if layout == "sh":
        return sink.t().unsqueeze(0).expand(T, -1, -1)
    return sink.permute(0, 2, 1)


def _oracle(q, k, v, idx2d, dout, scale, softcap, dtype, sink=None,
            layout="sh", p_dtype=None):
    """Gather-based attention (+ autograd when dout is given) in `dtype`.
    Returns a dict: out, lse, max_logits (per head, valid slots only, no
    sink), and dq, dk, dv, dsink."""
    q = q.detach().to(dtype).requires_grad_(True)
    k = k.detach().to(dtype).requires_grad_(True)
    v = v.detach().to(dtype).requires_grad_(True)
    valid = idx2d >= 0
    g = idx2d.clamp_min(0).long()
    kg = k[g, 0]  # [T, M, D]
    vg = v[g, 0]
    s = torch.einsum("thd,tmd->thm", q, kg) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    M = s.shape[-1]
    sk = None
    full = s
    if sink is not None:
        sk = sink.detach().to(dtype).requires_grad_(True)
        full = torch.cat([s, _sink_cols(sk, layout, s.shape[0])], dim=-1)
    lse = torch.logsumexp(full, dim=-1)
    p = torch.softmax(full, dim=-1).nan_to_num(0.0)[..., :M]
    if p_dtype is not None:
        p = p.to(p_dtype).to(dtype)
    out = torch.einsum("thm,tmd->thd", p, vg)
    r = dict(out=out.detach(), lse=lse.detach(),
             max_logits=s.detach().amax(dim=(0, 2)))
    if dout is not None:
        out.backward(dout.to(dtype))
        r.update(dq=q.grad, dk=k.grad, dv=v.grad,
                 dsink=None if sk is None else sk.grad)
    return r


def _make(B, S_q, S_kv, ratio, nhk, D, topk, max_topk, seed, fp8=False,
          indices=None):
    g = torch.Generator().manual_seed(seed)
    T = B * S_q * nhk

    def rnd(*shape):
        x = torch.randn(*shape, generator=g)
        return (x * 0.5).to(FP8).cuda() if fp8 else x.bfloat16().cuda()

    q = rnd(T, ratio, D)
    k = rnd(B * S_kv * nhk, 1, D)
    v = rnd(B * S_kv * nhk, 1, D)
    # fp8 gradients come back as e4m3, whose normal range ends at 2^-6: with
    # a sink holding most of a row's mass, dq for a randn * 0.5 dout has rms
    # 5e-3 and the cast of the EXACT fp64 dq alone is 1.1e-1 off (subnormal
    # steps), above the 9e-2 floor. The gradients are linear in dout, so
    # randn * 4 lifts them into the normal range (cast error 2.7e-2, the
    # figure the fp8 budgets were set against) and changes nothing else.
    dout = torch.randn(T, ratio, D, generator=g)
    dout = (dout * 4.0 if fp8 else dout).bfloat16().cuda()
    if indices is None:
        torch.manual_seed(seed)
        indices = build_index_attn_indices(
            B, nhk, S_q, S_kv, topk, max_topk, device="cuda"
        )
    return q, k, v, dout, indices


def _make_sink(layout, s_sink, T, H, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 + seed)
    shape = (s_sink, H) if layout == "sh" else (T, s_sink, H)
    return (torch.randn(*shape, generator=g) * 2 + 2).to(dtype).cuda()


def _run_kernel(q, k, v, dout, indices, sink=None, layout="sh", **kw):
    from magi_attention.functional import flex_flash_attn_func

    qg, kg, vg = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    sg = None if sink is None else sink.detach().clone().requires_grad_(True)
    out, meta = flex_flash_attn_func(
        qg, kg, vg, index_attn_indices=indices, sink=sg, sink_layout=layout,
        **kw
    )
    out.backward(dout)
    torch.cuda.synchronize()
    return dict(out=out.detach(), lse=meta.lse, max_logits=meta.max_logits,
                dq=qg.grad, dk=kg.grad, dv=vg.grad,
                dsink=None if sg is None else sg.grad)


def _check_lse(got, hi, name):
    fin = torch.isfinite(hi)
    assert torch.equal(torch.isfinite(got), fin), f"{name}: lse finiteness"
    err = (got[fin].double() - hi[fin]).abs().max().item()
    print(f"    [{name}:lse] max abs err={err:.3e} "
          f"(atol={LSE_ATOL:.0e}, rtol={LSE_RTOL:.0e})")
    torch.testing.assert_close(got[fin], hi[fin].float(),
                               atol=LSE_ATOL, rtol=LSE_RTOL)


def _check_max_logits(got, hi, hq, name):
    assert got is not None, f"{name}: meta.max_logits is None"
    assert got.shape == (hq,) and got.dtype == torch.float32
    err = (got.double() - hi).abs().max().item()
    print(f"    [{name}:max_logits] max abs err={err:.3e} "
          f"(atol={ML_ATOL:.0e}, rtol={ML_RTOL:.0e})")
    torch.testing.assert_close(got, hi.float(), atol=ML_ATOL, rtol=ML_RTOL)


def _check_all(got, hi, lo, name, names=("out", "dq", "dk", "dv", "dsink"),
               **budget):
    for nm in names:
        assert got[nm] is not None, f"{name}: {nm} is None"
        assert got[nm].shape == hi[nm].shape, f"{name}: {nm} shape"
        assert torch.isfinite(got[nm].float()).all(), f"{name}: {nm} not finite"
        kw = budget if nm != "out" else {}
        assert_close_to_ref(got[nm].float(), hi[nm], lo[nm], f"{name}:{nm}",
                            **kw)
    _check_lse(got["lse"], hi["lse"], name)


def _bf16_case(shape, layout, s_sink, softcap=0.0, seed=0, indices=None,
               **kw):
    """run kernel + both oracles for a bf16 case with a sink, check all"""
    cfg = SHAPES[shape] if isinstance(shape, str) else shape
    q, k, v, dout, indices = _make(**cfg, seed=seed, indices=indices)
    T, H, D = q.shape
    sink = _make_sink(layout, s_sink, T, H, seed)
    got = _run_kernel(q, k, v, dout, indices, sink, layout, softcap=softcap,
                      **kw)
    idx2d = indices.reshape(-1, indices.shape[-1])
    scale = D ** (-0.5)
    hi = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.float64, sink,
                 layout)
    lo = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.bfloat16, sink,
                 layout)
    name = f"{shape if isinstance(shape, str) else 'case'}-{layout}{s_sink}"
    _check_all(got, hi, lo, name)
    assert got["dsink"].dtype == sink.dtype
    return (q, k, v, dout, indices, sink), got, hi, lo


# ---------------------------------------------------------------- case 1, 2
@requires_gpu
@pytest.mark.parametrize("layout,s_sink", SINKS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_index_sink_fwd_bwd(shape, layout, s_sink):
    """out, lse, dq, dk, dv, dsink with a sink folded in the epilogue."""
    _bf16_case(shape, layout, s_sink, seed=len(shape) + s_sink)


@requires_gpu
@pytest.mark.parametrize("layout,s_sink", SINKS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_index_sink_fwd_bwd_softcap(shape, layout, s_sink):
    """the same through the HAS_SOFTCAP instances (softcap=2.0)."""
    _bf16_case(shape, layout, s_sink, softcap=2.0, seed=3 + s_sink)


# ------------------------------------------------------------------- case 3
@requires_gpu
@pytest.mark.parametrize("layout,s_sink", [("sh", 2), ("ssh", 3)])
def test_index_sink_all_padding_rows(layout, s_sink):
    """Rows whose whole list is -1 hold the sink's mass alone: out exactly 0,
    lse = lse_sink, dq exactly 0, ("ssh") dsink exactly 0, all finite."""
    cfg = dict(B=1, S_q=8, S_kv=64, ratio=32, nhk=1, D=128, topk=None,
               max_topk=64)
    idx = build_index_attn_indices(1, 1, 8, 64, 32, 64, device="cuda")
    idx[2] = -1
    idx[5] = -1
    (q, k, v, dout, _, sink), got, hi, _ = _bf16_case(
        cfg, layout, s_sink, seed=17, indices=idx
    )
    cols = _sink_cols(sink.double(), layout, q.shape[0])
    lse_sink = torch.logsumexp(cols, dim=-1)
    for r in (2, 5):
        assert (got["out"][r] == 0).all()
        assert (got["dq"][r] == 0).all()
        torch.testing.assert_close(got["lse"][r], lse_sink[r].float(),
                                   atol=LSE_ATOL, rtol=LSE_RTOL)
        torch.testing.assert_close(hi["lse"][r], lse_sink[r],  # the oracle's
                                   atol=0.0, rtol=1e-12)
        if layout == "ssh":
            assert (got["dsink"][r] == 0).all()
    for nm in ("dq", "dk", "dv", "dsink"):
        assert torch.isfinite(got[nm]).all()


# ------------------------------------------------------------------- case 4
@requires_gpu
@pytest.mark.parametrize("softcap", [0.0, 2.0])
@pytest.mark.parametrize("shape", ["r128", "r8", "d96", "multi"])
def test_index_max_logits(shape, softcap):
    """return_max_logits without a sink: per-head maximum over valid slots;
    out/lse/grads with the flag on (defer-max threshold 0) keep the budgets
    they have with it off."""
    cfg = SHAPES[shape]
    q, k, v, dout, idx = _make(**cfg, seed=41)
    T, H, D = q.shape
    idx2d = idx.reshape(-1, idx.shape[-1])
    hi = _oracle(q, k, v, idx2d, dout, D ** -0.5, softcap, torch.float64)
    lo = _oracle(q, k, v, idx2d, dout, D ** -0.5, softcap, torch.bfloat16)
    names = ("out", "dq", "dk", "dv")
    off = _run_kernel(q, k, v, dout, idx, softcap=softcap)
    assert off["max_logits"] is None
    _check_all(off, hi, lo, f"{shape}-ml-off", names)
    on = _run_kernel(q, k, v, dout, idx, softcap=softcap,
                     return_max_logits=True)
    _check_all(on, hi, lo, f"{shape}-ml-on", names)
    _check_max_logits(on["max_logits"], hi["max_logits"], H, shape)
    assert not on["max_logits"].requires_grad


@requires_gpu
@pytest.mark.parametrize("softcap", [0.0, 2.0])
def test_index_max_logits_with_sink_and_empty_batch(softcap):
    """Every row of batch 1 is all padding: those rows add nothing to
    max_logits (their lse is the sink's); the sink logits, far above the
    scores here, do not enter it either. No-grad route."""
    from magi_attention.functional import flex_flash_attn_func

    cfg = SHAPES["r32x2"]
    q, k, v, dout, idx = _make(**cfg, seed=43)
    T, H, D = q.shape
    idx[cfg["S_q"]:] = -1
    idx2d = idx.reshape(-1, idx.shape[-1])
    sink = _make_sink("sh", 4, T, H, 43) + 20.0
    hi = _oracle(q, k, v, idx2d, None, D ** -0.5, softcap, torch.float64,
                 sink, "sh")
    lo = _oracle(q, k, v, idx2d, None, D ** -0.5, softcap, torch.bfloat16,
                 sink, "sh")
    with torch.no_grad():
        out, meta = flex_flash_attn_func(
            q, k, v, index_attn_indices=idx, sink=sink, softcap=softcap,
            return_max_logits=True,
        )
    torch.cuda.synchronize()
    assert torch.isfinite(hi["max_logits"]).all()
    assert hi["max_logits"].max() < sink.min()
    _check_max_logits(meta.max_logits, hi["max_logits"], H, "emptybatch")
    assert_close_to_ref(out, hi["out"], lo["out"], "emptybatch:out")
    _check_lse(meta.lse, hi["lse"], "emptybatch")
    assert (out[cfg["S_q"] * cfg["nhk"]:] == 0).all()


# ------------------------------------------------------------------- case 5
@requires_gpu
@pytest.mark.parametrize(
    "shape,layout,s_sink,softcap",
    [("r128", "sh", 8, 0.0), ("r32x2", "ssh", 3, 0.0), ("d64", "sh", 1, 2.0),
     ("d96", "ssh", 3, 0.0), ("multi", "sh", 8, 0.0)],
)
def test_index_fp8_sink_max_logits(shape, layout, s_sink, softcap):
    """fp8 q/k/v: sink + max_logits in the fp8 epilogue, bf16-upcast
    backward with fp8 gradients and an f32 dsink. Two rows are all padding."""
    cfg = SHAPES[shape]
    q, k, v, dout, idx = _make(**cfg, seed=31, fp8=True)
    idx[1] = -1
    idx[-1] = -1
    T, H, D = q.shape
    sink = _make_sink(layout, s_sink, T, H, 31)
    got = _run_kernel(q, k, v, dout, idx, sink, layout, softcap=softcap,
                      return_max_logits=True)
    idx2d = idx.reshape(-1, idx.shape[-1])
    scale = D ** (-0.5)
    hi = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.float64, sink,
                 layout)
    lo = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.bfloat16, sink,
                 layout)
    lo["out"] = _oracle(q, k, v, idx2d, None, scale, softcap, torch.float32,
                        sink, layout, p_dtype=FP8)["out"]
    name = f"fp8-{shape}-{layout}{s_sink}"
    assert got["out"].dtype == torch.bfloat16
    for nm, src in (("dq", q), ("dk", k), ("dv", v)):
        assert got[nm] is not None and got[nm].dtype == FP8, nm
        assert got[nm].shape == src.shape
    _check_all(got, hi, lo, name, ratio=GRAD_RATIO, floor=GRAD_FLOOR)
    assert got["dsink"].dtype == torch.float32
    _check_max_logits(got["max_logits"], hi["max_logits"], H, name)


# ------------------------------------------------------------------- case 6
@requires_gpu
@pytest.mark.parametrize("s_sink", [1, 8])
def test_index_sink_matches_range_path(s_sink):
    """Each token lists a contiguous run [s, s + 64); the same mask goes to
    the dense kernel as one (q, k) range pair per token with the same "sh"
    sink - code the hand-written oracle does not share."""
    from magi_attention.functional import flex_flash_attn_func

    T, S_kv, H, D, run = 33, 128, 32, 128, 64
    g = torch.Generator().manual_seed(53)
    q = torch.randn(T, H, D, generator=g).bfloat16().cuda()
    k = torch.randn(S_kv, 1, D, generator=g).bfloat16().cuda()
    v = torch.randn(S_kv, 1, D, generator=g).bfloat16().cuda()
    starts = torch.randint(0, S_kv - run + 1, (T,), generator=g)
    idx = (starts[:, None] + torch.arange(run)[None]).int().cuda()
    idx = idx.view(T, 1, run)
    sink = _make_sink("sh", s_sink, T, H, 53)
    rows = torch.arange(T)
    qr = torch.stack([rows, rows + 1], 1).int().cuda()
    kr = torch.stack([starts, starts + run], 1).int().cuda()
    tm = torch.zeros(T, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o_i, m_i = flex_flash_attn_func(q, k, v, index_attn_indices=idx,
                                        sink=sink)
        o_r, m_r = flex_flash_attn_func(q, k, v, qr, kr, tm, sink=sink)
    torch.cuda.synchronize()
    idx2d = idx.view(T, run)
    hi = _oracle(q, k, v, idx2d, None, D ** -0.5, 0.0, torch.float64, sink)
    lo = _oracle(q, k, v, idx2d, None, D ** -0.5, 0.0, torch.bfloat16, sink)
    denom = hi["out"].norm()
    err_lo = ((lo["out"].double() - hi["out"]).norm() / denom).item()
    budget = 2 * max(MISMATCH_RATIO * err_lo, FLOOR)
    diff = ((o_i.double() - o_r.double()).norm() / denom).item()
    lse_diff = (m_i.lse - m_r.lse).abs().max().item()
    print(f"    [range-vs-index sh{s_sink}] out diff={diff:.3e} "
          f"budget={budget:.3e}; lse diff={lse_diff:.3e}")
    assert diff <= budget
    torch.testing.assert_close(m_i.lse, m_r.lse, atol=LSE_ATOL, rtol=LSE_RTOL)
    assert_close_to_ref(o_i, hi["out"], lo["out"], "range-vs-index:index out")


# ------------------------------------------------------------------- case 7
@requires_gpu
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("shape", ["r128", "r8", "d64", "multi"])
def test_index_sink_off_means_off(shape, fp8):
    """sink=None / no max_logits is the old launch bit for bit (the six
    positional arguments), and so is a sink whose logits are all -inf."""
    from magi_attention.functional import flex_flash_attn_func
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward_index,
    )

    cfg = SHAPES[shape]
    q, k, v, _, idx = _make(**cfg, seed=61, fp8=fp8)
    idx[3] = -1
    T, H, D = q.shape
    idx2d = idx.reshape(-1, idx.shape[-1])
    with torch.no_grad():
        o0, m0 = _flex_flash_attn_forward_index(q, k, v, idx2d, D ** -0.5, 0.0)
        o1, m1 = flex_flash_attn_func(q, k, v, index_attn_indices=idx,
                                      sink=None, return_max_logits=False)
        outs = [(o1, m1)]
        for layout, s in (("sh", 2), ("ssh", 8)):
            shp = (s, H) if layout == "sh" else (T, s, H)
            ninf = torch.full(shp, float("-inf"), device="cuda")
            outs.append(flex_flash_attn_func(
                q, k, v, index_attn_indices=idx, sink=ninf,
                sink_layout=layout,
            ))
    torch.cuda.synchronize()
    assert m0.max_logits is None and m1.max_logits is None
    for o, m in outs:
        assert torch.equal(o, o0)
        assert torch.equal(m.lse, m0.lse)  # -inf rows included


# ------------------------------------------------------------------- case 8
@requires_gpu
@pytest.mark.parametrize("layout,s_sink", [("sh", 8), ("ssh", 3)])
def test_index_sink_nograd_equals_autograd_forward(layout, s_sink):
    """The plain forward route with a sink equals the autograd route's
    forward bit for bit, both carry the sink (lse against the oracle), and
    dsink comes back in the sink's dtype / not at all for a frozen sink."""
    from magi_attention.functional import flex_flash_attn_func

    cfg = SHAPES["r32x2"]
    q, k, v, dout, idx = _make(**cfg, seed=71)
    T, H, D = q.shape
    sink = _make_sink(layout, s_sink, T, H, 71, dtype=torch.bfloat16)
    with torch.no_grad():
        o_ng, m_ng = flex_flash_attn_func(
            q, k, v, index_attn_indices=idx, sink=sink, sink_layout=layout,
            return_max_logits=True,
        )
    got = _run_kernel(q, k, v, dout, idx, sink, layout,
                      return_max_logits=True)
    assert torch.equal(got["out"], o_ng)
    assert torch.equal(got["lse"], m_ng.lse)
    assert torch.equal(got["max_logits"], m_ng.max_logits)
    assert not got["lse"].requires_grad
    idx2d = idx.reshape(-1, idx.shape[-1])
    hi = _oracle(q, k, v, idx2d, None, D ** -0.5, 0.0, torch.float64, sink,
                 layout)
    _check_lse(m_ng.lse, hi["lse"], f"nograd-{layout}{s_sink}")
    assert got["dsink"] is not None and got["dsink"].dtype == torch.bfloat16
    assert got["dsink"].shape == sink.shape

    # only the sink needs a gradient: still the differentiable route (same
    # flags, so the same forward; the 132 rows are one row block of the "sh"
    # dsink reduction, so its single atomic add per logit is reproducible)
    sg = sink.clone().requires_grad_(True)
    o, _ = flex_flash_attn_func(q, k, v, index_attn_indices=idx, sink=sg,
                                sink_layout=layout, return_max_logits=True)
    o.backward(dout)
    assert torch.equal(sg.grad, got["dsink"])
    # frozen sink: no dsink from the node
    qg = q.clone().requires_grad_(True)
    o, _ = flex_flash_attn_func(qg, k, v, index_attn_indices=idx, sink=sink,
                                sink_layout=layout, return_max_logits=True)
    grads = o.grad_fn.apply(dout, None, None)
    assert len(grads) == 9 and grads[6] is None
    assert torch.equal(grads[0], got["dq"])
