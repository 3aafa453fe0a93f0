"""C-ABI surface of the index-attention backward (include/magi_ffa.h
magi_ffa_bwd_index): the symbol and its ctypes struct exist, and the
argument-validation codes come back BEFORE any GPU work, so they are checkable
without a GPU (fake non-null pointers, no kernel is launched)."""
import ctypes

import pytest

from magi_attention import _ffa_lib


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _args(**over):
    from magi_attention._ffa_lib import MagiFfaIndexBwdArgs

    kw = dict(
        dout=1, q=1, k=1, v=1, lse=1, dpsum=1, indices_2d=1, dq=1, dk=1, dv=1,
        total_q=8, total_k=8, max_topk=64, hq=4, hk=1, d=128,
        softmax_scale=1.0, softcap=0.0, stream=None,
    )
    kw.update(over)
    return MagiFfaIndexBwdArgs(**kw)


def test_index_bwd_symbol_and_struct():
    lib = _lib()
    from magi_attention._ffa_lib import MagiFfaIndexBwdArgs

    fn = lib.magi_ffa_bwd_index
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.POINTER(MagiFfaIndexBwdArgs)]
    names = [f[0] for f in MagiFfaIndexBwdArgs._fields_]
    assert names == [
        "dout", "q", "k", "v", "lse", "dpsum", "indices_2d", "dq", "dk", "dv",
        "total_q", "total_k", "max_topk", "hq", "hk", "d",
        "softmax_scale", "softcap", "stream",
    ]
    # 10 pointers + 2 int64 + 4 int32 + 2 float + stream, no padding holes
    assert ctypes.sizeof(MagiFfaIndexBwdArgs) == 10 * 8 + 2 * 8 + 6 * 4 + 8


def test_index_bwd_validation_codes():
    lib = _lib()
    a = _args(hk=2)
    assert lib.magi_ffa_bwd_index(ctypes.byref(a)) == -3  # hk must be 1
    a.hk = 1
    a.d = 96
    assert lib.magi_ffa_bwd_index(ctypes.byref(a)) == -2  # d bucket
    a.d = 128
    for bad in (50, 0, -64):
        a.max_topk = bad
        assert lib.magi_ffa_bwd_index(ctypes.byref(a)) == -4  # 64 | max_topk
    a.max_topk = 64
    for field in ("dout", "q", "k", "v", "lse", "dpsum", "indices_2d",
                  "dq", "dk", "dv"):
        b = _args(**{field: None})
        assert lib.magi_ffa_bwd_index(ctypes.byref(b)) == -1, field
    assert lib.magi_ffa_bwd_index(None) == -1
    # nothing to do: returns 0 without a launch
    assert lib.magi_ffa_bwd_index(ctypes.byref(_args(total_q=0))) == 0
