"""swap_bwd_qk_loop on the GPU: the one-pass q-outer backward
(csrc/ffa_bwd_qloop.hip) through _flex_flash_attn_backward(
swap_bwd_qk_loop=True), out and lse from the default forward, against
oracle.ref_attn_with_grads in fp64 over the mask the pairs spell out, within
tests/util.assert_close_to_ref (lo = the 16-bit oracle with P rounded to the
element type). Flag on against flag off within the same budget; dq rows in no
range and dk/dv rows of keys in no range exactly zero.
CASES: name -> (tq, tk, auto_range_merge, [(q range, k range, type)])."""
import functools

import pytest
import torch

from oracle import make_attn_mask, ref_attn_with_grads
from tests.util import assert_close_to_ref, make_flex_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]
BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
_B16 = lambda q, *bs: [(q, (16 * b, 16 * b + 16), 0) for b in bs]  # noqa: E731
_SEGS = lambda q, *ks: [(q, k, 0) for k in ks]  # noqa: E731
CASES = {
    # second wave partial, k tail 64 + 32
    "tails": (40, 96, False, [((0, 40), (0, 96), 0)]),
    "short": (40, 96, False, _SEGS((0, 40), (3, 10), (20, 85))),  # 7 and 65
    # tq != tk: some waves skip tiles, the exchange image is zeroed
    "causal": (72, 104, False, [((0, 72), (0, 104), 1)]),
    "inv": (72, 104, False, [((0, 72), (0, 104), 2)]),
    "bi": (72, 104, False, [((0, 72), (0, 104), 3)]),
    # two q ranges on one k range (dK/dV atomics across workgroups), two
    # overlapping q ranges (dQ atomics)
    "shared": (104, 160, False, [((0, 40), (10, 90), 0), ((50, 100), (10, 90), 0),
                                 ((30, 70), (100, 140), 1)]),
    # 300 rows from an unaligned start: three workgroups on the same keys
    "wgs": (340, 80, False, [((37, 337), (0, 70), 0)]),
    # an empty k range (rows 0..19 dead, lse = -inf); rows 20..29 and keys
    # 40.. in no range
    "empty": (64, 96, False, [((0, 20), (50, 50), 0), ((30, 60), (0, 40), 1)]),
    # merged: k segments out of order, of unequal length, one empty
    "uneq": (40, 256, True, _SEGS((0, 40), (200, 201), (3, 10), (50, 83),
                                  (100, 200), (90, 90), (20, 36))),
    "two": (320, 256, True, _SEGS((0, 20), (50, 50)) + _B16((37, 300), 9, 2, 5)
            + _SEGS((300, 316), (0, 1), (128, 228), (30, 37), (250, 256))),
}
VARIANTS = {
    "base": {}, "d64": dict(d=64), "fp16": dict(dtype=FP16),
    "softcap": dict(softcap=0.25), "direct": dict(direct=True),
    "gqa": dict(hq=4, hk=2), "margin": dict(sm_margin=250),
}
PARITY = [(n, "base") for n in CASES] + [
    (n, v) for n in ("bi", "two") for v in VARIANTS if v != "base"]


@functools.lru_cache(maxsize=None)
def _case(name, hq=2, hk=2, d=128, dtype=BF16, softcap=0.0):
    tq, tk, merge, slices = CASES[name]
    c = type("Case", (), {})()
    c.softcap, c.scale, c.dtype, c.merge = softcap, d ** -0.5, dtype, merge
    c.q, c.k, c.v, c.dout, c.qr, c.kr, c.tm = make_flex_case(
        tq, tk, hq, hk, d, *zip(*slices), dtype=dtype)
    live = [s for s in slices if s[1][0] < s[1][1]]
    c.mask = make_attn_mask(tq, tk, *zip(*live))
    cpu = [t.cpu() for t in (c.q, c.k, c.v)]
    c.hi = ref_attn_with_grads(*(t.double() for t in cpu), c.mask,
                               c.dout.cpu().double(), softcap=softcap)
    c.lo = ref_attn_with_grads(*cpu, c.mask, c.dout.cpu(), softcap=softcap,
                               high_precision=False, p_dtype=dtype)
    for g in c.hi[2:]:
        assert torch.isfinite(g).all() and g.norm() > 0
    return c


def _fwd_and_common(c, sm_margin=0):
    from magi_attention.functional.flex_flash_attn import _flex_flash_attn_forward

    common = dict(q=c.q, k=c.k, v=c.v, sink=None, sink_layout="sh",
                  q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
                  softmax_scale=c.scale, softcap=c.softcap,
                  deterministic=False, sm_margin=sm_margin)
    out, meta = _flex_flash_attn_forward(
        out=None, lse=None, out_type=None,
        disable_fwd_atomic_reduction=False, **common)
    return out, meta.lse, common


def _grads(c, swap, direct=False, sm_margin=0):
    """(dq, dk, dv) on the CPU"""
    from magi_attention.functional.flex_flash_attn import _flex_flash_attn_backward

    out, lse, common = _fwd_and_common(c, sm_margin)
    grads = _flex_flash_attn_backward(
        dout=c.dout, out=out, lse=lse, dq=None, dk=None, dv=None, dsink=None,
        dq_type=None, dk_type=None, dv_type=None,
        disable_bwd_dkv_atomic_reduction=False, auto_range_merge=c.merge,
        disable_bwd_dq_atomic_reduction=direct, swap_bwd_qk_loop=swap,
        **common)[:3]
    torch.cuda.synchronize()
    assert grads[0].dtype == (c.dtype if direct else torch.float32)
    assert grads[1].dtype == grads[2].dtype == torch.float32
    return [g.cpu() for g in grads]


def _check(c, grads, what):
    for g, i, n in zip(grads, (2, 3, 4), ("dq", "dk", "dv")):
        assert_close_to_ref(g.to(c.dtype), c.hi[i], c.lo[i], f"{what}:{n}")


@pytest.mark.parametrize("name,variant", PARITY)
def test_parity(name, variant):
    kw = dict(VARIANTS[variant])
    direct, margin = kw.pop("direct", False), kw.pop("sm_margin", 0)
    c = _case(name, **kw)
    on, off = _grads(c, True, direct, margin), _grads(c, False, direct, margin)
    _check(c, on, f"{name}:{variant}")
    for a, b, i in zip(on, off, (2, 3, 4)):
        assert_close_to_ref(c.hi[i] + (a.double() - b.double()), c.hi[i],
                            c.lo[i], "on-off")
    assert (on[0][~c.mask.any(1)] == 0).all(), "dq rows without a key"
    for g in on[1:]:
        assert (g[~c.mask.any(0)] == 0).all(), "dk/dv rows of keys in no range"


@pytest.mark.parametrize("name", ["shared", "two"])
def test_entry_alone(name):
    """One launch of the new entry produces all three gradients (fails at the
    parent commit: there is no such entry)"""
    from magi_attention.functional import _ffa_launch
    from magi_attention.functional.flex_flash_attn import _merged_tables

    c = _case(name)
    out, lse, _ = _fwd_and_common(c)
    dq, dk, dv = (torch.zeros_like(t, dtype=torch.float32)
                  for t in (c.q, c.k, c.v))
    dpsum = torch.empty(c.q.shape[:2], dtype=torch.float32, device="cuda")
    args = _ffa_launch.bwd_args(
        c.dout, out, dpsum, q=c.q, k=c.k, v=c.v, lse=lse, dq=dq, dk=dk, dv=dv,
        q_ranges=c.qr, k_ranges=c.kr, attn_type_map=c.tm,
        max_seqlen_k=c.k.shape[0], softmax_scale=c.scale)
    _ffa_launch.bwd_preprocess(args)
    tables = _merged_tables(c.qr, c.kr, c.tm) if c.merge else None
    _ffa_launch.run_bwd_qloop(args, tables)
    torch.cuda.synchronize()
    _check(c, [g.cpu() for g in (dq, dk, dv)], f"entry:{name}")


def test_d192_is_the_flag_off_launch():
    """No element of "two" collects more than two atomic adds in the two
    passes (dq one; a dk/dv row lies in at most two distinct k ranges), and
    a + b is b + a: flag off is reproducible bit for bit."""
    c = _case("two", d=192)
    on, off = _grads(c, True), _grads(c, False)
    for a, b in zip(on, off):
        assert torch.equal(a, b) and a.norm() > 0


@pytest.mark.parametrize("fp8", [False, True], ids=["merge", "fp8"])
def test_public_entry(monkeypatch, fp8):
    """The flag from the public entry to the one-pass launch, which must be
    what ran (at the parent commit the flag is dropped and there is no such
    launch). fp8 inputs go through FlexFlashAttnFunc.apply and the
    bf16-upcast backward; their budget is the one of
    tests/test_ffa_fp8_flex_gpu.py (test_softcap_merged_backward), fp8
    gradients included."""
    from magi_attention.functional import _ffa_launch, flex_flash_attn_func
    from magi_attention.functional.flex_flash_attn import FlexFlashAttnFunc

    calls, launch = [], _ffa_launch.run_bwd_qloop
    monkeypatch.setattr(_ffa_launch, "run_bwd_qloop",
                        lambda *a: (calls.append(1), launch(*a))[1])
    c = _case("two", hq=4)
    ins = [t.to(FP8) if fp8 else t.clone() for t in (c.q, c.k, c.v)]
    leaves = [t.requires_grad_(True) for t in ins]
    if fp8:
        out = FlexFlashAttnFunc.apply(
            *leaves, None, "sh", c.qr, c.kr, c.tm, None, 0.0, False, 0, False,
            False, None, None, True, False, False, False, False, False, True)[0]
        args = [t.detach().cpu().float() for t in leaves] + [c.mask, c.dout.cpu().float()]
        hi = ref_attn_with_grads(*args)
        lo = ref_attn_with_grads(*args, high_precision=False, p_dtype=BF16)
        budget = {0: dict(ratio=8.0, floor=3.5e-2)}
        grad_budget = dict(ratio=4.5, floor=9e-2)
    else:
        out, _ = flex_flash_attn_func(*leaves, c.qr, c.kr, c.tm,
                                      auto_range_merge=True,
                                      swap_bwd_qk_loop=True)
        hi, lo, budget, grad_budget = c.hi, c.lo, {}, {}
    out.backward(c.dout)
    assert calls == [1]
    for g, i, n in zip([out.detach()] + [t.grad for t in leaves], (0, 2, 3, 4),
                       ("out", "dq", "dk", "dv")):
        assert_close_to_ref(g.cpu().float(), hi[i].float(), lo[i].float(),
                            f"public:{n}", **budget.get(i, grad_budget))
