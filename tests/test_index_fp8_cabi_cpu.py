"""C-ABI surface of the fp8 index-attention forward (include/magi_ffa.h
magi_ffa_fwd_index_fp8): the symbol exists, its ctypes signature is declared,
and the argument-validation codes come back BEFORE any GPU work, so they are
checkable without a GPU (fake non-null pointers, no kernel is launched)."""
import ctypes

import pytest

from magi_attention import _ffa_lib


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _args(**over):
    from magi_attention._ffa_lib import MagiFfaIndexArgs

    kw = dict(
        q=1, k=1, v=1, out=1, lse=1, indices_2d=1,
        total_q=8, total_k=8, max_topk=64, hq=4, hk=1, d=128,
        softmax_scale=1.0, softcap=0.0, out_is_fp32=0, stream=None,
    )
    kw.update(over)
    return MagiFfaIndexArgs(**kw)


def test_index_fp8_symbol_and_signature():
    lib = _lib()
    from magi_attention._ffa_lib import MagiFfaIndexArgs

    fn = lib.magi_ffa_fwd_index_fp8
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.POINTER(MagiFfaIndexArgs)]
    # the fp8 entry reuses the bf16 entry's struct unchanged
    assert lib.magi_ffa_fwd_index.argtypes == fn.argtypes
    names = [f[0] for f in MagiFfaIndexArgs._fields_]
    assert names == [
        "q", "k", "v", "out", "lse", "indices_2d",
        "total_q", "total_k", "max_topk", "hq", "hk", "d",
        "softmax_scale", "softcap", "out_is_fp32", "stream",
    ]


def test_index_fp8_validation_codes():
    lib = _lib()
    a = _args(hk=2)
    assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(a)) == -3  # hk must be 1
    a.hk = 1
    a.d = 96
    assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(a)) == -2  # d bucket
    a.d = 128
    for bad in (50, 0, -64):
        a.max_topk = bad
        assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(a)) == -4  # 64 | max_topk
    a.max_topk = 64
    for field in ("q", "k", "v", "out", "lse", "indices_2d"):
        b = _args(**{field: None})
        assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(b)) == -1, field
    assert lib.magi_ffa_fwd_index_fp8(None) == -1
    # nothing to do: returns 0 without a launch
    assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(_args(total_q=0))) == 0
    assert lib.magi_ffa_fwd_index_fp8(ctypes.byref(_args(total_q=-3))) == 0


def test_index_fp8_validation_order_matches_bf16_entry():
    """Several faults at once: both entries report the same first one."""
    lib = _lib()
    for over in (
        dict(q=None, d=96, hk=2, max_topk=50),   # null wins
        dict(d=96, hk=2, max_topk=50),           # then d
        dict(hk=2, max_topk=50),                 # then hk
        dict(max_topk=50, total_q=0),            # then max_topk, before sizes
    ):
        a = _args(**over)
        assert (lib.magi_ffa_fwd_index_fp8(ctypes.byref(a))
                == lib.magi_ffa_fwd_index(ctypes.byref(a))), over


def test_index_fp8_dtype_asserts_cpu():
    """Python-side dtype rules fire before any native call."""
    import torch

    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward_index,
    )

    q8 = torch.zeros(2, 4, 64).to(torch.float8_e4m3fn)
    kb = torch.zeros(4, 1, 64, dtype=torch.bfloat16)
    idx = torch.zeros(2, 64, dtype=torch.int32)
    with pytest.raises(AssertionError, match="float8_e4m3fn.*bfloat16"):
        _flex_flash_attn_forward_index(q8, kb, kb, idx, 1.0, 0.0)
    qh = torch.zeros(2, 4, 64, dtype=torch.float16)
    with pytest.raises(AssertionError, match="index_attn requires bf16 inputs"):
        _flex_flash_attn_forward_index(qh, qh[:, :1], qh[:, :1], idx, 1.0, 0.0)


def test_index_fp8_head_dim_pad_cpu():
    """The fp8 pad goes through a byte view: zero bytes are e4m3 +0 and the
    original columns are untouched."""
    import torch

    from magi_attention.functional.flex_flash_attn import (
        _index_head_dim_pad,
        _pad_head_dim,
    )

    assert [_index_head_dim_pad(d) for d in (64, 128, 96, 40)] == [0, 0, 32, 24]
    x = (torch.randn(5, 3, 96) * 0.5).to(torch.float8_e4m3fn)
    y = _pad_head_dim(x, 32)
    assert y.dtype == torch.float8_e4m3fn and y.shape == (5, 3, 128)
    assert torch.equal(y[..., :96].view(torch.uint8), x.view(torch.uint8))
    assert torch.equal(y[..., 96:].view(torch.uint8),
                       torch.zeros(5, 3, 32, dtype=torch.uint8))
    assert _pad_head_dim(x, 0) is x
