"""sparse_load of the dense dQ pass, everything that needs no GPU. The entry
validates before it touches a pointer or the HIP runtime, so fake non-null
pointers are enough and nothing is launched."""
import ctypes

import pytest
import torch

from magi_attention import _ffa_lib
from magi_attention.functional import _ffa_launch, flex_flash_attn_func

BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# magi_ffa.h's validation order with sparse_load = 1: (what breaks it, code)
ORDER = [(dict(q=None), -1), (dict(d=96), -2), (dict(hk=3), -3),
         (dict(elem_type=2), -9), (dict(sparse_reserved=1), -14),
         (dict(seg_starts=None), -15), (dict(k_cum=None), -1),
         (dict(n_ranges=0), 0)]


def _args(**over):
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    kw = dict(dout=1, q=1, k=1, v=1, out=1, lse=1, dq=1, dk=1, dv=1, dpsum=1,
              q_ranges=1, k_ranges=1, seg_starts=1, k_cum=1, n_ranges=1,
              total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_k=8,
              softmax_scale=1.0, sparse_load=1)
    kw.update(over)
    return _ffa_lib.MagiFfaBwdSparseArgs(**kw)


@pytest.mark.parametrize("i", range(len(ORDER)),
                         ids=[f"{i}:{c}" for i, (_, c) in enumerate(ORDER)])
def test_size_and_validation_order(i):
    """Code i is returned with everything before it valid and everything after
    it broken as well; with sparse_load = 0 the entry is the _direct one."""
    over = {}
    for o, _ in reversed(ORDER[i:]):
        over.update(o)
    on, off = _args(**over), _args(sparse_load=0, **over)
    lib = _ffa_lib.lib()
    assert lib.magi_ffa_bwd_sparse_args_size() == ctypes.sizeof(on)
    assert ctypes.sizeof(on) == ctypes.sizeof(_ffa_lib.MagiFfaBwdCatArgs) + 16
    assert lib.magi_ffa_bwd_dq_sparse(None) == -1
    assert lib.magi_ffa_bwd_dq_sparse(ctypes.byref(on)) == ORDER[i][1]
    assert lib.magi_ffa_bwd_dq_sparse(ctypes.byref(off)) == (
        lib.magi_ffa_bwd_dq_direct(off))
    # d = 192 under the flag is the segment-loop launch, not an error
    assert lib.magi_ffa_bwd_dq_sparse(ctypes.byref(_args(d=192, n_ranges=0))) == 0
    # the dkv entries take the struct and ignore the new members
    assert lib.magi_ffa_bwd_dkv_cat(_args(n_ranges=0, sparse_reserved=1)) == 0


@pytest.mark.parametrize("flag,dtype,d,tables,want", [
    (True, BF16, 128, (), True), (1, FP16, 64, (), True),
    (False, BF16, 128, (), False), (True, FP8, 128, (), False),
    (True, torch.float32, 64, (), False), (True, BF16, 192, (), False),
    (True, BF16, 128, None, False)])
def test_active_rule(flag, dtype, d, tables, want):
    assert _ffa_launch.bwd_sparse_load_active(flag, dtype, d, tables) is want


def test_sparse_load_bwd_needs_sparse_load():
    q, r = torch.zeros(4, 2, 64, dtype=BF16), torch.zeros(0, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="requires sparse_load=True"):
        flex_flash_attn_func(q, q, q, r, r, None, auto_range_merge=True,
                             sparse_load_bwd=True)
    with pytest.raises(RuntimeError, match="range merge must be enabled"):
        flex_flash_attn_func(q, q, q, r, r, None, sparse_load=True,
                             sparse_load_bwd=True)
