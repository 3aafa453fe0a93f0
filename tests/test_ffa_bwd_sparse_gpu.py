"""sparse_load of the dense dQ pass on the GPU: _flex_flash_attn_backward(
auto_range_merge=True, sparse_load=True) over flat (q range, k range) pair
lists, out and lse from the default forward, against oracle.
ref_attn_with_grads in fp64 over the mask the pairs spell out, within
tests/util.assert_close_to_ref (lo = the 16-bit oracle with P rounded to the
element type). Flag on against flag off within the same budget (not bit-equal:
the tile composition changes); dq rows in no range or in a range with L = 0
exactly zero. CASES: name -> (tq, tk, [(q range, its k ranges)])."""
import functools

import pytest
import torch

from oracle import make_attn_mask, ref_attn_with_grads
from tests.util import assert_close_to_ref, make_flex_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]
BF16, FP16 = torch.bfloat16, torch.float16
_B16 = lambda *bs: [(16 * b, 16 * b + 16) for b in bs]  # noqa: E731
CASES = {  # L = a range's virtual length
    "L16": (40, 96, [((0, 40), _B16(2))]),
    "L31": (40, 96, [((0, 40), [(90, 91), (10, 17), (40, 63)])]),
    "L64": (40, 160, [((0, 40), _B16(1, 3, 5, 8))]),  # no tail subtile
    "L65": (40, 160, [((0, 40), [(5, 6), (20, 27), (100, 133), (50, 50), (60, 84)])]),
    "L80": (40, 160, [((0, 40), _B16(0, 2, 9, 6, 4))]),  # shuffled
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
    "base": {}, "d64": dict(d=64), "fp16": dict(dtype=FP16),
    "softcap": dict(softcap=0.25), "direct": dict(direct=True),
    "w8": dict(MAGI_BWD_DQ_BIGSEQ=1), "gqa": dict(hq=4, hk=2),
}
PARITY = [(n, "base") for n in CASES] + [
    (n, v) for n in ("uneq", "two") for v in VARIANTS if v != "base"]


@functools.lru_cache(maxsize=None)
def _case(name, atype=0, hq=2, hk=2, d=128, dtype=BF16, softcap=0.0):
    tq, tk, ranges = CASES[name]
    c = type("Case", (), {})()
    pairs = [(qr, kr) for qr, segs in ranges for kr in segs]
    c.softcap, c.scale, c.dtype = softcap, d ** -0.5, dtype
    c.q, c.k, c.v, c.dout, c.qr, c.kr, c.tm = make_flex_case(
        tq, tk, hq, hk, d, *zip(*pairs), [atype] * len(pairs), dtype=dtype)
    live = [p for p in pairs if p[1][0] < p[1][1]]
    c.mask = make_attn_mask(tq, tk, *zip(*live), [atype] * len(live))
    cpu = [t.cpu() for t in (c.q, c.k, c.v)]
    c.hi = ref_attn_with_grads(*(t.double() for t in cpu), c.mask,
                               c.dout.cpu().double(), softcap=softcap)
    c.lo = ref_attn_with_grads(*cpu, c.mask, c.dout.cpu(), softcap=softcap,
                               high_precision=False, p_dtype=dtype)
    for g in c.hi[2:]:
        assert torch.isfinite(g).all() and g.norm() > 0
    return c


def _grads(c, sparse, direct=False, fwd=None):
    """(dq, dk, dv) on the CPU; fwd: the case whose mask the forward serves"""
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_backward, _flex_flash_attn_forward)

    fwd = fwd or c
    common = dict(q=c.q, k=c.k, v=c.v, sink=None, sink_layout="sh",
                  q_ranges=c.qr, k_ranges=c.kr, softmax_scale=c.scale,
                  softcap=c.softcap, deterministic=False, sm_margin=0)
    out, meta = _flex_flash_attn_forward(
        out=None, lse=None, attn_type_map=fwd.tm, out_type=None,
        disable_fwd_atomic_reduction=False, **common)
    grads = _flex_flash_attn_backward(
        dout=c.dout, out=out, lse=meta.lse, dq=None, dk=None, dv=None,
        dsink=None, attn_type_map=c.tm, dq_type=None, dk_type=None,
        dv_type=None, disable_bwd_dkv_atomic_reduction=False,
        auto_range_merge=True, sparse_load=sparse,
        disable_bwd_dq_atomic_reduction=direct, **common)[:3]
    torch.cuda.synchronize()
    assert grads[0].dtype == (c.dtype if direct else torch.float32)
    return [g.cpu() for g in grads]


@pytest.mark.parametrize("name,variant", PARITY)
def test_parity(monkeypatch, name, variant):
    kw = dict(VARIANTS[variant])
    monkeypatch.delenv("MAGI_BWD_DQ_BIGSEQ", raising=False)
    if "MAGI_BWD_DQ_BIGSEQ" in kw:
        monkeypatch.setenv("MAGI_BWD_DQ_BIGSEQ", str(kw.pop("MAGI_BWD_DQ_BIGSEQ")))
    direct = kw.pop("direct", False)
    c = _case(name, **kw)
    on, off = _grads(c, True, direct), _grads(c, False, direct)
    for g, i, n in zip(on, (2, 3, 4), ("dq", "dk", "dv")):
        assert_close_to_ref(g.to(c.dtype), c.hi[i], c.lo[i], f"{name}:{variant}:{n}")
    assert_close_to_ref(c.hi[2] + (on[0].double() - off[0].double()), c.hi[2],
                        c.lo[2], "dq on-off")
    assert (on[0][~c.mask.any(1)] == 0).all(), "dq rows without a key"


@pytest.mark.parametrize("name", ["uneq", "two"])
def test_type_map_is_not_read(name):
    """The one observable difference between the two launches: over a table
    whose attn_type_map says causal the sparse kernel serves full blocks (as
    magi_ffa.h documents), the segment loop causal ones."""
    full, causal = _case(name), _case(name, atype=1)
    assert (full.hi[2] - causal.hi[2]).norm() > 0.1 * full.hi[2].norm()
    on = _grads(causal, True, fwd=full)[0]
    assert_close_to_ref(on, full.hi[2], full.lo[2], "flag on: full mask")
    off = _grads(causal, False)[0]
    assert_close_to_ref(off, causal.hi[2], causal.lo[2], "flag off: causal")


def test_d192_is_the_flag_off_launch():
    c = _case("two", d=192)
    on, off = _grads(c, True), _grads(c, False)
    assert torch.equal(on[0], off[0]) and on[0].norm() > 0


def test_public_entry():
    """fails at the parent commit with a TypeError"""
    from magi_attention.functional import flex_flash_attn_func

    c = _case("two", hq=4)
    leaves = [t.clone().requires_grad_(True) for t in (c.q, c.k, c.v)]
    out, _ = flex_flash_attn_func(
        *leaves, c.qr, c.kr, c.tm, auto_range_merge=True, sparse_load=True,
        sparse_load_bwd=True)
    out.backward(c.dout)
    for g, i, n in zip([out.detach()] + [t.grad for t in leaves], (0, 2, 3, 4),
                       ("out", "dq", "dk", "dv")):
        assert_close_to_ref(g.cpu(), c.hi[i], c.lo[i], f"public:{n}")
