"""pack_gqa of the dense forward, everything that needs no GPU.

magi_ffa_fwd_args keeps its size (tests/test_ffa_fp16_cpu.py pins it); the
switch rides behind an embedded copy in magi_ffa_fwd_pack_args, which
magi_ffa_fwd_pack takes. The entry validates before it touches a pointer or
the HIP runtime, so fake non-null pointers are enough and nothing is launched.
Host layer: _ffa_launch.fwd over CPU tensors with recording functions in place
of the C entries."""
import ctypes
import types

import pytest
import torch

from magi_attention import _ffa_lib
from magi_attention.functional import _ffa_launch

BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# magi_ffa.h's validation order with pack_gqa = 1: (what breaks it, code)
ORDER = [(dict(q=None), -1), (dict(d=96), -2), (dict(hk=3), -3),
         (dict(elem_type=2), -9), (dict(reserved=1), -14),
         (dict(n_ranges=0), 0), (dict(locks=None), -4),
         (dict(n_ranges=70000), -5), (dict(out_is_fp32=0), -10)]


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _args(**over):
    kw = dict(q=1, k=1, v=1, out=1, lse=1, q_ranges=1, k_ranges=1, locks=1,
              n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128,
              max_seqlen_q=8, softmax_scale=1.0, out_is_fp32=1, pack_gqa=1)
    kw.update(over)
    return _ffa_lib.MagiFfaFwdPackArgs(**kw)


def test_struct_size_and_layout():
    lib = _lib()
    base, cls = _ffa_lib.MagiFfaFwdArgs, _ffa_lib.MagiFfaFwdPackArgs
    assert lib.magi_ffa_args_size(0) == ctypes.sizeof(base)
    assert lib.magi_ffa_fwd_pack_args_size() == ctypes.sizeof(cls)
    assert ctypes.sizeof(cls) == ctypes.sizeof(base) + 8
    assert [f[0] for f in cls._fields_] == ["pack_gqa", "reserved"]
    assert cls.pack_gqa.offset == ctypes.sizeof(base)
    assert cls.reserved.offset == ctypes.sizeof(base) + 4
    for name, _ in base._fields_:
        assert getattr(cls, name).offset == getattr(base, name).offset, name


@pytest.mark.parametrize("i", range(len(ORDER)), ids=[str(c) for _, c in ORDER])
def test_validation_order(i):
    """Code i is returned with everything before it valid and everything after
    it broken as well. With pack_gqa = 0 the entry is magi_ffa_fwd, which does
    not read reserved."""
    lib = _lib()
    over = {}
    for o, _ in reversed(ORDER[i:]):
        over.update(o)
    code = ORDER[i][1]
    assert lib.magi_ffa_fwd_pack(None) == -1
    assert lib.magi_ffa_fwd_pack(ctypes.byref(_args(**over))) == code
    off = _args(pack_gqa=0, **over)
    assert (lib.magi_ffa_fwd_pack(ctypes.byref(off)) == lib.magi_ffa_fwd(off)
            == (0 if code == -14 else code))


@pytest.mark.parametrize("flag,dtype,hq,hk,want", [
    (True, BF16, 4, 2, True), (True, FP16, 6, 2, True), (1, BF16, 8, 1, True),
    (False, BF16, 4, 2, False), (None, FP16, 4, 2, False),
    (True, BF16, 2, 2, False), (True, FP8, 4, 2, False)])
def test_active_rule_and_entry(monkeypatch, flag, dtype, hq, hk, want):
    assert _ffa_launch.pack_gqa_active(flag, dtype, hq, hk) is want
    seen = []
    fake = types.SimpleNamespace(**{
        n: (lambda a, n=n: seen.append((n, type(a), a.n_ranges)) or 0)
        for n in ("magi_ffa_fwd", "magi_ffa_fwd_fp8", "magi_ffa_fwd_pack")})
    monkeypatch.setattr(_ffa_launch._ffa_lib, "lib", lambda: fake)
    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    q = torch.zeros(8, hq, 64).to(dtype)
    k = torch.zeros(8, hk, 64).to(dtype)
    out, lse = torch.zeros(8, hq, 64), torch.zeros(8, hq)
    r = torch.tensor([[0, 8], [0, 8]], dtype=torch.int32)  # two q groups
    for det in (False, True):
        del seen[:]
        _ffa_launch.fwd(
            q, k, k, out, lse, r, r, None, locks=lse, max_logits=None,
            qk_starts=None, max_seqlen_q=8, softmax_scale=1.0, softcap=0.0,
            disable_fwd_atomic_reduction=False, sm_margin=0,
            deterministic=det, pack_gqa=flag)
        entry = ("magi_ffa_fwd_pack", _ffa_lib.MagiFfaFwdPackArgs) if want else (
            "magi_ffa_fwd_fp8" if dtype == FP8 else "magi_ffa_fwd",
            _ffa_lib.MagiFfaFwdArgs)
        assert seen == ([entry + (1,)] * 2 if det else [entry + (2,)])


def test_pack_gqa_with_cat_gqa_still_raises():
    from magi_attention.functional import flex_flash_attn_func

    q, k = torch.zeros(4, 4, 64, dtype=BF16), torch.zeros(6, 2, 64, dtype=BF16)
    r = torch.zeros(0, 2, dtype=torch.int32)
    with pytest.raises(AssertionError, match="cannot be both True"):
        flex_flash_attn_func(q, k, k, r, r, None, pack_gqa=True, cat_gqa=True)
