"""What the dense fp8 forward refuses (include/magi_ffa.h magi_ffa_fwd_fp8).
The C entry returns its validation codes before it touches a pointer, so fake
non-null pointers are enough and no kernel is launched; the Python-side rule
fires before any native call."""
import ctypes

import pytest

from magi_attention import _ffa_lib


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _args(**over):
    from magi_attention._ffa_lib import MagiFfaFwdArgs

    kw = dict(
        q=1, k=1, v=1, out=1, lse=1, q_ranges=1, k_ranges=1,
        attn_type_map=None, locks=1, max_logits=None, qk_starts=None,
        n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_q=8,
        softmax_scale=1.0, softcap=0.0, out_is_fp32=1,
        disable_atomic_reduction=0, cu_margin=0, stream=None,
    )
    kw.update(over)
    return MagiFfaFwdArgs(**kw)


def test_fp8_fwd_rejects_softcap():
    lib = _lib()
    for cap in (20.0, -1.0, 1e-3):
        a = _args(softcap=cap)
        assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == -7, cap
    # also with nothing to do: the refusal does not depend on the range count
    a = _args(softcap=20.0, n_ranges=0)
    assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == -7


def test_fp8_fwd_rejects_head_dim_192():
    lib = _lib()
    for d in (192, 96, 32, 256, 0):
        a = _args(d=d)
        assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == -2, d
    # the bf16 entry has a 192 bucket and gets past the d check: with no
    # range it returns 0 without a launch
    a = _args(d=192, n_ranges=0)
    assert lib.magi_ffa_fwd(ctypes.byref(a)) == 0
    assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == -2


def test_fp8_fwd_accepts_the_base_arguments():
    """The two tests above fail for the stated field alone: the same struct
    with softcap 0, d in (64, 128) and no range is accepted."""
    lib = _lib()
    for d in (64, 128):
        a = _args(d=d, n_ranges=0)
        assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == 0


def test_fp8_padded_head_dim_requires_bf16():
    import torch

    from magi_attention.functional import flex_flash_attn_func

    q = torch.zeros(4, 2, 96).to(torch.float8_e4m3fn)
    k = torch.zeros(6, 2, 96).to(torch.float8_e4m3fn)
    empty = torch.zeros(0, 2, dtype=torch.int32)
    with pytest.raises(AssertionError, match="padded head dims require bf16"):
        flex_flash_attn_func(q, k, k.clone(), empty, empty.clone(), None)
