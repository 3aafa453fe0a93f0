"""magi_ffa_fwd_fp8_flex and its launcher rule, everything that needs no GPU:
the entry's validation order (fake pointers, nothing is launched), which fp8
calls _ffa_launch.fwd sends to it, and the yardstick of the softcap tests in
tests/test_ffa_fp8_flex_gpu.py (an fp32 emulation of the kernel's rounding
stays inside the envelope of the softcapped fp64 oracle)."""
import ctypes
import math
import types

import pytest
import torch

from magi_attention import _ffa_lib
from magi_attention.functional import _ffa_launch
from oracle import make_attn_mask
from oracle.ref_attn import merge_out_lse
from tests import test_ffa_fp8_flex_gpu as F

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
# magi_ffa.h's validation order: (what breaks it, code)
ORDER = [(dict(q=None), -1), (dict(d=192), -2), (dict(hk=3), -3),
         (dict(out_is_fp32=0, disable_atomic_reduction=0), -6),
         (dict(softcap=-1.0), -7), (dict(n_ranges=0), 0),
         (dict(locks=None), -4), (dict(n_ranges=70000), -5)]


def _call(**over):
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    kw = dict(q=1, k=1, v=1, out=1, lse=1, q_ranges=1, k_ranges=1, locks=1,
              qk_starts=1, n_ranges=1, total_q=8, total_k=8, hq=4, hk=2,
              d=128, max_seqlen_q=8, softmax_scale=1.0, softcap=2.0,
              out_is_fp32=1)
    kw.update(over)
    fn = _ffa_lib.lib().magi_ffa_fwd_fp8_flex
    assert fn(None) == -1
    return fn(ctypes.byref(_ffa_lib.MagiFfaFwdArgs(**kw)))


@pytest.mark.parametrize("i", range(len(ORDER)), ids=[str(c) for _, c in ORDER])
def test_validation_order(i):
    """code i comes back with everything before it valid and everything after
    it broken as well"""
    over = {}
    for o, _ in reversed(ORDER[i:]):
        over.update(o)
    assert _call(**over) == ORDER[i][1]


@pytest.mark.parametrize("out_is_fp32", [0, 1])
def test_direct_store_needs_no_locks(out_is_fp32):
    """past -6 and -4 with either out type: the next check answers"""
    assert _call(disable_atomic_reduction=1, out_is_fp32=out_is_fp32,
                 locks=None, n_ranges=70000) == -5


@pytest.mark.parametrize("dtype,kw,flex", [
    (FP8, {}, False), (FP8, dict(softcap=2.0), True),
    (FP8, dict(qk_starts=True), True),
    (FP8, dict(disable_fwd_atomic_reduction=True), True),
    (BF16, dict(softcap=2.0, qk_starts=True,
                disable_fwd_atomic_reduction=True), False)])
def test_routing_rule(monkeypatch, dtype, kw, flex):
    seen = []
    fake = types.SimpleNamespace(**{
        n: (lambda a, n=n: seen.append((n, a.n_ranges)) or 0)
        for n in ("magi_ffa_fwd", "magi_ffa_fwd_fp8", "magi_ffa_fwd_fp8_flex")})
    monkeypatch.setattr(_ffa_launch._ffa_lib, "lib", lambda: fake)
    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    q = torch.zeros(8, 4, 64).to(dtype)
    k = torch.zeros(8, 2, 64).to(dtype)
    out, lse = torch.zeros(8, 4, 64), torch.zeros(8, 4)
    r = torch.tensor([[0, 8], [0, 8]], dtype=torch.int32)  # two q groups
    starts = torch.zeros(3, dtype=torch.int32) if kw.get("qk_starts") else None
    args = dict(locks=lse, max_logits=None, max_seqlen_q=8, softmax_scale=1.0,
                softcap=0.0, disable_fwd_atomic_reduction=False, sm_margin=0)
    args.update(kw, qk_starts=starts)
    assert _ffa_launch.fp8_flex_active(
        dtype, args["softcap"], starts,
        args["disable_fwd_atomic_reduction"]) is flex
    entry = ("magi_ffa_fwd_fp8_flex" if flex else
             "magi_ffa_fwd_fp8" if dtype == FP8 else "magi_ffa_fwd")
    for det in (False, True):
        del seen[:]
        if det and starts is not None:
            # deterministic + merged: refused (16 bit: by the caller of fwd)
            if flex:
                with pytest.raises(AssertionError, match="deterministic"):
                    _ffa_launch.fwd(q, k, k, out, lse, r, r, None,
                                    deterministic=True, **args)
            continue
        _ffa_launch.fwd(q, k, k, out, lse, r, r, None, deterministic=det,
                        **args)
        assert seen == ([(entry, 1)] * 2 if det else [(entry, 2)])


def emulate_softcap(r):
    """E.emulate with s -> CAP * tanh(s / CAP) (r.s holds it, masked by the
    union): per table row, P scaled to [0, 256] and rounded to e4m3,
    normalised by the unrounded sum; rows merged by lse; out through bf16"""
    c = r.case
    hq, hk = c["hq"], c["hk"]
    vf = r.v8.float()[:, [h // (hq // hk) for h in range(hq)]].permute(1, 0, 2)
    outs, lses = [], []
    for qr, kr, ty in zip(c["qr"], c["kr"], c["ty"]):
        m = make_attn_mask(c["tq"], c["tk"], [qr], [kr], [ty])
        s = r.s.float().masked_fill(~m.unsqueeze(0), float("-inf"))
        mx = s.amax(dim=-1, keepdim=True)
        mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
        pr = torch.exp(s - mx) * 256.0
        l_ = pr.sum(dim=-1, keepdim=True)
        o = torch.matmul(pr.to(FP8).float(), vf)
        outs.append(torch.where(l_ > 0, o / l_, torch.zeros_like(o))
                    .permute(1, 0, 2))
        lses.append(torch.where(l_ > 0, mx + torch.log(l_) - math.log(256.0),
                                torch.full_like(l_, float("-inf")))
                    .squeeze(-1).permute(1, 0))
    out, lse = merge_out_lse(outs, lses)
    return out.float().bfloat16().float(), lse.float()


@pytest.mark.parametrize("d", F.E.DIMS)
@pytest.mark.parametrize("name", ["causal_unaligned", "bicausal_192x224",
                                  "merged_segments"])
def test_softcap_emulation_inside_envelope(name, d):
    r = F.softcap_ref(name, d)
    assert F.ATOL_LSE_CAP <= 0.5 * r.p_min and F.E.ATOL_LSE <= 0.5 * r.p_min
    out, lse = emulate_softcap(r)
    assert torch.equal(torch.isfinite(lse), torch.isfinite(r.lse64))
    assert F.E.lse_errors(lse, r) <= 0.5 * r.p_min
    assert F.E.out_ratio(out, r) <= 1.0
    assert torch.equal(out[~r.has_key], torch.zeros_like(out[~r.has_key]))
