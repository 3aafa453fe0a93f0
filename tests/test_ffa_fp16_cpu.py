"""fp16 q/k/v on the dense path, everything that needs no GPU.

ABI: magi_ffa_fwd_args and magi_ffa_bwd_args end in elem_type (0 bf16, 1
fp16). The C entries validate before they touch a pointer or the HIP runtime,
so fake non-null pointers are enough and no kernel is launched. A ctypes
mirror that disagrees with the C struct would hand a kernel garbage pointers:
magi_ffa_args_size is compared with ctypes.sizeof for every public struct.

Host layer: the dtype rules fire before anything is allocated or launched;
every call passes an EMPTY range table, with which the C entries return before
any launch even if a rule were missing.

Oracle only: the fp16-vs-bf16 error ratio that tests/test_ffa_fp16_gpu.py asks
of the kernels (0.5) can be met - on the same inputs the fp16-P oracle's error
is at most 0.25 of the bf16-P oracle's."""
import ctypes
import itertools
import re

import pytest
import torch

from magi_attention import _ffa_lib
from tests.fp16_cases import RATIO_CASES, reference, rel_l2

FP16, BF16, FP8 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
BAD_ELEM_TYPE = -9
BWD_ENTRIES = ("magi_ffa_bwd_preprocess", "magi_ffa_bwd_dq", "magi_ffa_bwd_dkv",
               "magi_ffa_bwd_dv", "magi_ffa_bwd_dk", "magi_ffa_bwd")


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _fwd_args(**over):
    kw = dict(
        q=1, k=1, v=1, out=1, lse=1, q_ranges=1, k_ranges=1,
        attn_type_map=None, locks=1, max_logits=None, qk_starts=None,
        n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_q=8,
        softmax_scale=1.0, softcap=0.0, out_is_fp32=1,
        disable_atomic_reduction=0, cu_margin=0, stream=None,
    )
    kw.update(over)
    return _ffa_lib.MagiFfaFwdArgs(**kw)


def _bwd_args(**over):
    kw = dict(
        dout=1, q=1, k=1, v=1, out=1, lse=1, dq=1, dk=1, dv=1, dpsum=1,
        q_ranges=1, k_ranges=1, attn_type_map=None, seg_starts=None,
        n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_k=8,
        out_is_fp32=0, softmax_scale=1.0, softcap=0.0, cu_margin=0,
        stream=None,
    )
    kw.update(over)
    return _ffa_lib.MagiFfaBwdArgs(**kw)


# ───────────────────────── C ABI ─────────────────────────

def test_args_size_matches_ctypes():
    lib = _lib()
    mirrors = [
        _ffa_lib.MagiFfaFwdArgs, _ffa_lib.MagiFfaBwdArgs,
        _ffa_lib.MagiRangeOpArgs, _ffa_lib.MagiSinkArgs,
        _ffa_lib.MagiCorrectArgs,
        # what constructing MagiFfaIndexArgs returns: the struct with its tail
        type(_ffa_lib.MagiFfaIndexArgs()),
        _ffa_lib.MagiFfaIndexBwdArgs,
    ]
    for which, cls in enumerate(mirrors):
        assert lib.magi_ffa_args_size(which) == ctypes.sizeof(cls), cls
    assert lib.magi_ffa_args_size(len(mirrors)) == -1
    assert lib.magi_ffa_args_size(-1) == -1


def test_elem_type_is_the_last_member_and_defaults_to_bf16():
    for cls in (_ffa_lib.MagiFfaFwdArgs, _ffa_lib.MagiFfaBwdArgs):
        assert cls._fields_[-1][0] == "elem_type"
        assert cls._fields_[-2][0] == "stream"
        assert cls.elem_type.offset == (
            cls.stream.offset + ctypes.sizeof(ctypes.c_void_p)
        )
        assert cls().elem_type == 0
    assert _fwd_args().elem_type == 0 and _bwd_args().elem_type == 0
    assert (_ffa_lib.ELEM_BF16, _ffa_lib.ELEM_FP16) == (0, 1)
    assert _ffa_lib.elem_type_of(FP16) == 1
    assert _ffa_lib.elem_type_of(BF16) == 0


def test_fp16_with_no_range_is_accepted():
    lib = _lib()
    a = _fwd_args(elem_type=1, n_ranges=0)
    assert lib.magi_ffa_fwd(ctypes.byref(a)) == 0
    # the preprocess has no range count: no row is its "nothing to do"
    b = _bwd_args(elem_type=1, n_ranges=0, total_q=0)
    for name in BWD_ENTRIES:
        assert getattr(lib, name)(ctypes.byref(b)) == 0, name


def test_unknown_elem_type_is_refused():
    lib = _lib()
    for et in (2, -1, 255):
        a = _fwd_args(elem_type=et)
        assert lib.magi_ffa_fwd(ctypes.byref(a)) == BAD_ELEM_TYPE, et
        b = _bwd_args(elem_type=et)
        for name in BWD_ENTRIES:
            assert getattr(lib, name)(ctypes.byref(b)) == BAD_ELEM_TYPE, (
                name, et)
    # the refusal does not depend on the range count
    a = _fwd_args(elem_type=2, n_ranges=0)
    assert lib.magi_ffa_fwd(ctypes.byref(a)) == BAD_ELEM_TYPE
    # the earlier codes keep their order in front of it
    assert lib.magi_ffa_fwd(ctypes.byref(_fwd_args(elem_type=2, d=96))) == -2
    assert lib.magi_ffa_fwd(ctypes.byref(_fwd_args(elem_type=2, hk=3))) == -3
    b = _bwd_args(elem_type=2, d=96)
    assert lib.magi_ffa_bwd_dq(ctypes.byref(b)) == -2


def test_fp8_entry_ignores_elem_type():
    lib = _lib()
    for et in (0, 1, 2):
        a = _fwd_args(elem_type=et, n_ranges=0)
        assert lib.magi_ffa_fwd_fp8(ctypes.byref(a)) == 0, et


# ───────────────────────── host layer ─────────────────────────

MIXED_16 = [
    c for c in itertools.product((FP16, BF16), repeat=3) if len(set(c)) > 1
]
MIXED_FP8 = [
    c for c in itertools.product((FP16, FP8), repeat=3) if len(set(c)) > 1
]


def _tensors(dq, dk, dv, d=64):
    q = torch.zeros(4, 2, d).to(dq)
    k = torch.zeros(6, 2, d).to(dk)
    v = torch.zeros(6, 2, d).to(dv)
    empty = torch.zeros(0, 2, dtype=torch.int32)
    return q, k, v, empty


def _forward(q, k, v, empty, **over):
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward,
    )

    kw = dict(
        q=q, k=k, v=v, sink=None, sink_layout="sh", out=None, lse=None,
        q_ranges=empty, k_ranges=empty.clone(), attn_type_map=None,
        softmax_scale=1.0, softcap=0.0, out_type=None,
        disable_fwd_atomic_reduction=False, deterministic=False,
        sm_margin=0, max_seqlen_q=0,
    )
    kw.update(over)
    return _flex_flash_attn_forward(**kw)


def _names(dq, dk, dv):
    return f"q={dq}.*k={dk}.*v={dv}".replace("torch.", r"torch\.")


def test_mixed_combinations_are_six_each():
    assert len(MIXED_16) == 6 and len(MIXED_FP8) == 6


@pytest.mark.parametrize("dq,dk,dv", MIXED_16 + MIXED_FP8,
                         ids=lambda t: str(t)[6:])
def test_forward_rejects_mixed_dtypes(dq, dk, dv):
    q, k, v, empty = _tensors(dq, dk, dv)
    with pytest.raises(AssertionError, match=_names(dq, dk, dv)) as ei:
        _forward(q, k, v, empty)
    assert re.search("must all be fp8-e4m3 or all be bf16", str(ei.value))


@pytest.mark.parametrize("dq,dk,dv", MIXED_16 + MIXED_FP8,
                         ids=lambda t: str(t)[6:])
def test_public_entry_rejects_mixed_dtypes(dq, dk, dv):
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, empty = _tensors(dq, dk, dv)
    with pytest.raises(AssertionError, match=_names(dq, dk, dv)):
        flex_flash_attn_func(q, k, v, empty, empty.clone(), None,
                             max_seqlen_q=0)


def _null_stream(monkeypatch):
    """A call that passes the dtype rules goes on to fill the argument struct,
    stream included, and torch cannot name a current stream without a device.
    The null (default) stream stands in: with an empty range table the C
    entry returns before it would use it."""
    from magi_attention.functional import _ffa_launch

    _lib()
    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))


@pytest.mark.parametrize("direct", [False, True], ids=["merge", "direct"])
def test_all_fp16_is_accepted(monkeypatch, direct):
    _null_stream(monkeypatch)
    q, k, v, empty = _tensors(FP16, FP16, FP16)
    out, meta = _forward(q, k, v, empty, disable_fwd_atomic_reduction=direct)
    assert out.dtype == (FP16 if direct else torch.float32)
    assert out.shape == q.shape and meta.lse.dtype == torch.float32

    from magi_attention.functional import flex_flash_attn_func

    out, meta = flex_flash_attn_func(
        q, k, v, empty, empty.clone(), None, max_seqlen_q=0,
        disable_fwd_atomic_reduction=direct,
    )
    assert out.dtype == FP16 and meta.lse.dtype == torch.float32


@pytest.mark.parametrize("qd,od", [(FP16, BF16), (BF16, FP16)],
                         ids=["fp16q-bf16out", "bf16q-fp16out"])
def test_other_16bit_out_is_rejected(qd, od):
    """Refused before anything is allocated or launched, as out_type and as
    an explicit out."""
    q, k, v, empty = _tensors(qd, qd, qd)
    with pytest.raises(AssertionError, match="out_type .* must be float32 or"):
        _forward(q, k, v, empty, out_type=od,
                 disable_fwd_atomic_reduction=True)
    with pytest.raises(AssertionError, match="out .* must be float32 or"):
        _forward(q, k, v, empty, out=torch.zeros(4, 2, 64, dtype=od),
                 disable_fwd_atomic_reduction=True)


def test_index_attn_still_requires_bf16():
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, _ = _tensors(FP16, FP16, FP16)
    idx = torch.full((4, 1, 64), -1, dtype=torch.int32)
    with pytest.raises(AssertionError, match="index_attn requires bf16 inputs"):
        flex_flash_attn_func(q, k[:, :1], v[:, :1], index_attn_indices=idx)


# ───────────────────────── oracle only ─────────────────────────

@pytest.mark.parametrize("name", RATIO_CASES)
def test_ratio_condition_is_satisfiable(name):
    """Test 9 of tests/test_ffa_fp16_gpu.py asks err(fp16 kernel) <= 0.5 *
    err(bf16 kernel). The oracles that round what the kernels round (inputs
    exact, P and the results in the 16-bit type) are 4x or more apart."""
    r = reference(name, 128)
    for i, what in ((0, "out"), (2, "dq"), (3, "dk"), (4, "dv")):
        e16, ebf = rel_l2(r.lo16[i], r.hi[i]), rel_l2(r.lobf[i], r.hi[i])
        print(f"    [fp16sat:{r.name}:{what}] fp16={e16:.3e} bf16={ebf:.3e} "
              f"ratio={e16 / ebf:.3f}")
        assert e16 <= 0.25 * ebf, (what, e16, ebf)
