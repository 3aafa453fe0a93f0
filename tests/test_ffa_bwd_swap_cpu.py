"""swap_bwd_qk_loop, everything that needs no GPU. magi_ffa_bwd_qloop
validates before it touches a pointer or the HIP runtime, so fake non-null
pointers are enough and nothing is launched."""
import ctypes

import pytest
import torch

from magi_attention import _ffa_lib
from magi_attention.functional import _ffa_launch, flex_flash_attn_func
from magi_attention.functional.flex_flash_attn import FlexFlashAttnFunc

BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# magi_ffa.h's validation order: (what breaks it, code)
ORDER = [(dict(dv=None), -1), (dict(d=192), -2), (dict(hk=3), -3),
         (dict(elem_type=2), -9), (dict(cu_margin=2 << 24), -12),
         (dict(dkv_is_16bit=1), -16), (dict(n_ranges=0), 0)]


def _args(**over):
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    kw = dict(dout=1, q=1, k=1, v=1, out=1, lse=1, dq=1, dk=1, dv=1, dpsum=1,
              q_ranges=1, k_ranges=1, n_ranges=1, total_q=8, total_k=8, hq=4,
              hk=2, d=128, max_seqlen_k=8, softmax_scale=1.0, dq_is_16bit=1)
    kw.update(over)
    return _ffa_lib.MagiFfaBwdSparseArgs(**kw)


@pytest.mark.parametrize("i", range(len(ORDER)),
                         ids=[f"{i}:{c}" for i, (_, c) in enumerate(ORDER)])
def test_validation_order(i):
    """Code i is returned with everything before it valid and everything after
    it broken as well"""
    over = {}
    for o, _ in reversed(ORDER[i:]):
        over.update(o)
    lib = _ffa_lib.lib()
    assert lib.magi_ffa_bwd_qloop(None) == -1
    assert lib.magi_ffa_bwd_qloop(ctypes.byref(_args(**over))) == ORDER[i][1]
    assert lib.magi_ffa_bwd_qloop(ctypes.byref(_args(d=96))) == -2
    # no existing struct grew for the new entry
    assert lib.magi_ffa_bwd_direct_args_size() == ctypes.sizeof(
        _ffa_lib.MagiFfaBwdDirectArgs)


@pytest.mark.parametrize("flag,dtype,d,want", [
    (True, BF16, 128, True), (1, FP16, 64, True), (False, BF16, 128, False),
    (None, BF16, 64, False), (True, FP8, 128, False),
    (True, torch.float32, 64, False), (True, BF16, 192, False)])
def test_active_rule(flag, dtype, d, want):
    assert _ffa_launch.bwd_swap_active(flag, dtype, d) is want


def test_refused_combinations():
    """Both fail at the parent commit, where the flag is dropped unread"""
    q, r = torch.zeros(4, 2, 64, dtype=BF16), torch.zeros(0, 2, dtype=torch.int32)
    msg = "disable_bwd_dkv_atomic_reduction is true, swap_bwd_qk_loop must be false"
    with pytest.raises(RuntimeError, match=msg):
        flex_flash_attn_func(q, q, q, r, r, None, swap_bwd_qk_loop=True,
                             disable_bwd_dkv_atomic_reduction=True)
    with pytest.raises(RuntimeError, match=msg):
        FlexFlashAttnFunc.apply(q, q, q, None, "sh", r, r, None, None, 0.0,
                                False, 0, False, True, None, None, False,
                                False, False, False, False, False, True)
    with pytest.raises(AssertionError, match="Deterministic mode is not supported"):
        flex_flash_attn_func(q, q, q, r, r, None, swap_bwd_qk_loop=True,
                             deterministic=True)
