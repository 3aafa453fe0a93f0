"""sparse_load of the dense forward on the GPU: _ffa_launch.fwd(sparse_load=
True) over hand-written merged tables against the fp64 oracle over the mask
the table spells out. out and lse within tests/util.assert_close_to_ref (lo =
the 16-bit oracle with P rounded to the element type), the lse -inf pattern
exact, rows in no range or in a range with L = 0 untouched; flag on against
flag off within the same budget (not bit-equal: the tile composition changes).
CASES: name -> (tq, tk, [(q range, its k segments in table order)])."""
import functools

import pytest
import torch

from oracle import make_attn_mask, ref_attn, ref_attn_with_grads
from tests.util import assert_close_to_ref, make_flex_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
_B16 = lambda *bs: [(16 * b, 16 * b + 16) for b in bs]  # noqa: E731
CASES = {  # L = a range's virtual length
    "L16": (40, 96, [((0, 40), _B16(2))]),
    "L31": (40, 96, [((0, 40), [(90, 91), (10, 17), (40, 63)])]),
    "L64": (40, 160, [((0, 40), _B16(1, 3, 5, 8))]),  # no tail tile
    "L65": (40, 160, [((0, 40), [(5, 6), (20, 27), (100, 133), (50, 50), (60, 84)])]),
    "L80": (40, 160, [((0, 40), _B16(0, 2, 9, 6, 4))]),  # shuffled
    "L128": (40, 256, [((0, 40), _B16(15, 13, 11, 9, 7, 5, 3, 1))]),  # descending
    "uneq": (40, 256, [((0, 40), [(200, 201), (3, 10), (50, 83), (100, 200),
                                  (90, 90), (20, 36)])]),  # L = 157
    # L = 0 (rows 0..19 stay dead), an unaligned range over several q blocks,
    # a 16-token range; rows 20..36 and 316..319 are in no range
    "two": (320, 256, [((0, 20), [(50, 50)]), ((37, 300), _B16(9, 2, 5)),
                       ((300, 316), [(0, 1), (128, 228), (30, 37), (250, 256)])]),
    # L = SPARSE_MAP_ROWS + 48: the map is rebuilt once, inside a segment
    "chunk": (40, 2200, [((0, 40), [(1150, 2198), (0, 1048)])]),
}
VARIANTS = {
    "base": {}, "w4": dict(MAGI_FWD_WAVES=4), "w8": dict(MAGI_FWD_WAVES=8),
    "d64": dict(d=64), "fp16": dict(dtype=FP16), "softcap": dict(softcap=0.25),
    "direct": dict(direct=True), "d64-fp16-direct": dict(d=64, dtype=FP16, direct=True),
    "pack-g4": dict(hq=4, hk=1, pack=True), "pack-g3": dict(hq=6, hk=2, pack=True),
    "pack-g4-w8-direct": dict(hq=4, hk=1, pack=True, direct=True, MAGI_FWD_WAVES=8),
    "max_logits": dict(hq=6, hk=2, pack=True, ml=True),
    "max_logits-softcap": dict(hq=6, hk=2, pack=True, ml=True, softcap=0.25),
}
PARITY = [(n, "base") for n in CASES] + [
    (n, v) for n in ("uneq", "two") for v in VARIANTS if v != "base"]


@functools.lru_cache(maxsize=None)
def _case(name, hq=2, hk=2, d=128, dtype=BF16, softcap=0.0, sink=False):
    tq, tk, ranges = CASES[name]
    c = type("Case", (), {})()
    c.flat = [(qr, kr) for qr, segs in ranges for kr in segs if kr[0] < kr[1]]
    c.softcap, c.scale, c.msq = softcap, d ** -0.5, max(e - s for (s, e), _ in ranges)
    c.q, c.k, c.v, c.dout, c.qr, c.kr, c.tm = make_flex_case(
        tq, tk, hq, hk, d, [r for r, _ in ranges],
        [kr for _, segs in ranges for kr in segs],
        [0] * sum(len(s) for _, s in ranges), dtype=dtype)
    c.starts = torch.tensor([0] + [len(s) for _, s in ranges]).cumsum(0).int().cuda()
    c.mask = make_attn_mask(tq, tk, *zip(*c.flat), [0] * len(c.flat))
    c.sink = torch.randn(2, hq, generator=torch.Generator().manual_seed(7)) if sink else None
    cpu = [t.cpu() for t in (c.q, c.k, c.v)]
    c.hi = ref_attn(*(t.double() for t in cpu), c.mask, softcap=softcap, sink=c.sink)
    c.lo = ref_attn(*cpu, c.mask, softcap=softcap, sink=c.sink,
                    high_precision=False, p_dtype=dtype)
    assert torch.isfinite(c.hi[0]).all() and c.hi[0].norm() > 0
    return c


def _run(c, sparse, direct=False, pack=False, ml=None, starts=True, q=None):
    from magi_attention.functional import _ffa_launch
    from magi_attention.functional.flex_flash_attn import _get_locks

    tq, hq, d = c.q.shape
    q, k, v = (c.q, c.k, c.v) if q is None else (t.to(q) for t in (c.q, c.k, c.v))
    out = torch.zeros(tq, hq, d, dtype=c.q.dtype if direct else F32, device="cuda")
    lse = torch.full((tq, hq), float("-inf"), device="cuda")
    _ffa_launch.fwd(
        q, k, v, out, lse, c.qr, c.kr, c.tm,
        locks=None if direct else _get_locks(tq, hq, out.device),
        max_logits=ml, qk_starts=c.starts if starts else None,
        max_seqlen_q=c.msq, softmax_scale=c.scale, softcap=c.softcap,
        disable_fwd_atomic_reduction=direct, sm_margin=0, deterministic=False,
        pack_gqa=pack, sparse_load=sparse)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def _check(c, out, lse, what, hi=None):
    hi = hi or c.hi  # hi: what to be close to (the oracle, or the flag-off run)
    live = ~torch.isinf(c.hi[1])
    assert torch.equal(torch.isinf(lse) & (lse < 0), ~live), f"{what}: -inf pattern"
    assert c.sink is not None or (out[~live] == 0).all(), f"{what}: dead rows"
    assert torch.isfinite(out).all()
    for got, i in ((out.to(c.q.dtype), 0), (lse[live], 1)):
        ref, lo = (t if i == 0 else t[live] for t in (c.hi[i], c.lo[i]))
        tgt = hi[i].double() if i == 0 else hi[i][live].double()
        assert_close_to_ref(ref + (got.double() - tgt), ref, lo, f"{what}:{i}")


@pytest.mark.parametrize("name,variant", PARITY)
def test_parity(monkeypatch, name, variant):
    kw = dict(VARIANTS[variant])
    monkeypatch.delenv("MAGI_FWD_WAVES", raising=False)
    if "MAGI_FWD_WAVES" in kw:
        monkeypatch.setenv("MAGI_FWD_WAVES", str(kw.pop("MAGI_FWD_WAVES")))
    run = dict(direct=kw.pop("direct", False), pack=kw.pop("pack", False))
    want_ml = kw.pop("ml", False)
    c = _case(name, **kw)
    ml = torch.full((c.q.shape[1],), float("-inf"), device="cuda") if want_ml else None
    on, off = _run(c, True, ml=ml, **run), _run(c, False, **run)
    _check(c, *on, f"{name}:{variant}")
    _check(c, *on, "on-off", hi=(off[0].to(c.q.dtype), off[1]))
    if want_ml:  # an exact maximum of fp32-accumulated 16-bit products
        kk = c.k.cpu().double().repeat_interleave(3, dim=1).permute(1, 2, 0)
        s = torch.matmul(c.q.cpu().double().permute(1, 0, 2), kk) * c.scale
        s = c.softcap * torch.tanh(s / c.softcap) if c.softcap else s
        ref = s.masked_fill(~c.mask, float("-inf")).amax(dim=(-1, -2)).float()
        torch.testing.assert_close(ml.cpu(), ref, atol=1e-4, rtol=1e-4)


def test_sink():
    from magi_attention.functional.flex_flash_attn import _flex_flash_attn_forward

    c = _case("two", sink=True)
    out, meta = _flex_flash_attn_forward(
        q=c.q, k=c.k, v=c.v, sink=c.sink.cuda(), sink_layout="sh", out=None,
        lse=None, q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
        qk_starts=c.starts, softmax_scale=c.scale, softcap=0.0, out_type=None,
        disable_fwd_atomic_reduction=False, deterministic=False, sm_margin=0,
        sparse_load=True)
    _check(c, out.cpu(), meta.lse.cpu(), "sink")


@pytest.mark.parametrize("what", ["d192", "fp8"])
def test_fallbacks_are_the_flag_off_launch(what):
    """no SPARSE build: the same launch, bit for bit (fp8 has no merged-table
    forward at all, so its table is the one-segment one without qk_starts)"""
    c = _case("two", d=192) if what == "d192" else _case("L16")
    kw = {} if what == "d192" else dict(starts=False, q=torch.float8_e4m3fn)
    on, off = _run(c, True, **kw), _run(c, False, **kw)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert on[0].norm() > 0


def test_public_entry_with_grads():
    from magi_attention.functional import flex_flash_attn_func

    c = _case("two", 4, 2)
    qr, kr = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in zip(*c.flat))
    leaves = [t.clone().requires_grad_(True) for t in (c.q, c.k, c.v)]
    out, meta = flex_flash_attn_func(
        *leaves, qr, kr, torch.zeros(len(c.flat), dtype=torch.int32, device="cuda"),
        auto_range_merge=True, sparse_load=True, pack_gqa=True)
    out.backward(c.dout)
    cpu = [t.cpu() for t in (c.q, c.k, c.v)]
    hi = ref_attn_with_grads(*(t.double() for t in cpu), c.mask, c.dout.cpu().double())
    lo = ref_attn_with_grads(*cpu, c.mask, c.dout.cpu(), high_precision=False,
                             p_dtype=BF16)
    assert torch.equal(torch.isinf(meta.lse.cpu()), torch.isinf(hi[1]))
    for g, i, n in zip([out.detach()] + [t.grad for t in leaves], (0, 2, 3, 4),
                       ("out", "dq", "dk", "dv")):
        assert_close_to_ref(g.cpu(), hi[i], lo[i], f"public:{n}")
