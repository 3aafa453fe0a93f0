"""swap_ab (the split-k forward), everything that needs no GPU, as
tests/test_ffa_fwd_pack_cpu.py does for pack_gqa: magi_ffa_fwd_splitk validates
before it touches a pointer or the HIP runtime, so fake non-null pointers are
enough; _ffa_launch.fwd runs over CPU tensors with recording fakes."""
import ctypes
import types

import pytest
import torch

from magi_attention import _ffa_lib
from magi_attention.functional import _ffa_launch
from tests.test_ffa_fwd_pack_cpu import _lib  # skips without the library

BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# magi_ffa.h's validation order with swap_ab = 1: (what breaks it, code)
ORDER = [(dict(q=None), -1), (dict(d=96), -2), (dict(hk=3), -3),
         (dict(elem_type=2), -9), (dict(reserved=1), -14),
         (dict(n_ranges=0), 0), (dict(locks=None), -4),
         (dict(n_ranges=70000), -5), (dict(out_is_fp32=0), -10)]


def _args(**over):
    kw = dict(q=1, k=1, v=1, out=1, lse=1, q_ranges=1, k_ranges=1, locks=1,
              n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128,
              max_seqlen_q=8, softmax_scale=1.0, out_is_fp32=1, swap_ab=1)
    kw.update(over)
    return _ffa_lib.MagiFfaFwdSplitkArgs(**kw)


def test_struct_size_and_layout():
    lib = _lib()
    base, cls = _ffa_lib.MagiFfaFwdArgs, _ffa_lib.MagiFfaFwdSplitkArgs
    assert lib.magi_ffa_fwd_splitk_args_size() == ctypes.sizeof(cls)
    assert ctypes.sizeof(cls) == ctypes.sizeof(base) + 8
    assert [f[0] for f in cls._fields_] == ["swap_ab", "reserved"]
    assert cls.swap_ab.offset == ctypes.sizeof(base)
    assert cls.reserved.offset == ctypes.sizeof(base) + 4
    for name, _ in base._fields_:
        assert getattr(cls, name).offset == getattr(base, name).offset, name


@pytest.mark.parametrize("i", range(len(ORDER)), ids=[str(c) for _, c in ORDER])
def test_validation_order(i):
    """Code i with everything before it valid and everything after it broken
    too, at d = 128 and d = 192 (the default launch, no error). swap_ab = 0 is
    magi_ffa_fwd, which does not read reserved."""
    lib = _lib()
    over = {}
    for o, _ in reversed(ORDER[i:]):
        over.update(o)
    code = ORDER[i][1]
    assert lib.magi_ffa_fwd_splitk(None) == -1
    assert lib.magi_ffa_fwd_splitk(ctypes.byref(_args(**over))) == code
    if code != -2:
        d192 = _args(**dict(over, d=192))
        assert lib.magi_ffa_fwd_splitk(ctypes.byref(d192)) == code
    off = _args(**dict(over, swap_ab=0))
    assert (lib.magi_ffa_fwd_splitk(ctypes.byref(off)) == lib.magi_ffa_fwd(off)
            == (0 if code == -14 else code))


@pytest.mark.parametrize("flag,dtype,d,hq,hk,pack,sparse,want", [
    (True, BF16, 64, 2, 2, False, False, True),
    (1, FP16, 128, 4, 2, False, False, True),   # GQA, unpacked
    (True, BF16, 64, 2, 2, True, False, True),  # pack_gqa with no group
    (False, BF16, 64, 2, 2, False, False, False),
    (None, FP16, 64, 2, 2, False, False, False),
    (True, FP8, 64, 2, 2, False, False, False),
    (True, BF16, 192, 2, 2, False, False, False),
    (True, BF16, 64, 4, 2, True, False, False),   # pack_gqa's kernel runs
    (True, BF16, 64, 2, 2, False, True, False)])  # sparse_load's kernel runs
def test_active_rule_and_entry(monkeypatch, flag, dtype, d, hq, hk, pack,
                               sparse, want):
    """The fake library has the split-k entry only where fwd must look it up."""
    qk_starts = torch.tensor([0, 1, 2], dtype=torch.int32) if sparse else None
    pack_on = _ffa_launch.pack_gqa_active(pack, dtype, hq, hk)
    sparse_on = _ffa_launch.sparse_load_active(sparse, dtype, d, qk_starts)
    assert _ffa_launch.swap_ab_active(flag, dtype, d, pack_on, sparse_on) is want
    if sparse_on:
        entry = ("magi_ffa_fwd_sparse", _ffa_lib.MagiFfaFwdSparseArgs)
    elif pack_on:
        entry = ("magi_ffa_fwd_pack", _ffa_lib.MagiFfaFwdPackArgs)
    elif want:
        entry = ("magi_ffa_fwd_splitk", _ffa_lib.MagiFfaFwdSplitkArgs)
    else:
        entry = ("magi_ffa_fwd_fp8" if dtype == FP8 else "magi_ffa_fwd",
                 _ffa_lib.MagiFfaFwdArgs)
    seen = []
    names = {"magi_ffa_fwd", "magi_ffa_fwd_fp8", entry[0]}
    fake = types.SimpleNamespace(**{
        n: (lambda a, n=n: seen.append(
            (n, type(a), a.n_ranges, getattr(a, "swap_ab", 0))) or 0)
        for n in names})
    monkeypatch.setattr(_ffa_launch._ffa_lib, "lib", lambda: fake)
    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    q = torch.zeros(8, hq, d).to(dtype)
    k = torch.zeros(8, hk, d).to(dtype)
    out, lse = torch.zeros(8, hq, d), torch.zeros(8, hq)
    r = torch.tensor([[0, 8], [0, 8]], dtype=torch.int32)  # two q groups
    for det in (False,) if sparse else (False, True):
        del seen[:]
        _ffa_launch.fwd(
            q, k, k, out, lse, r, r, None, locks=lse, max_logits=None,
            qk_starts=qk_starts, max_seqlen_q=8, softmax_scale=1.0,
            softcap=0.0, disable_fwd_atomic_reduction=False, sm_margin=0,
            deterministic=det, pack_gqa=pack, sparse_load=sparse,
            swap_ab=flag)
        n = 1 if det else 2  # ranges per launch
        assert seen == [entry + (n, int(want))] * (3 - n)
