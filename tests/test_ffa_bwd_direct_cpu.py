"""Direct 16-bit dQ/dK/dV stores of the dense backward, everything that needs
no GPU.

ABI: magi_ffa_bwd_args keeps its size and its last member, which
tests/test_ffa_fp16_cpu.py pins; the two switches dq_is_16bit and dkv_is_16bit
ride behind an embedded copy of it in magi_ffa_bwd_direct_args, which the
magi_ffa_bwd_{dq,dkv,dv,dk}_direct entries take. A zero-filled tail is the f32
atomic path. The C entries validate before they touch a pointer or the HIP
runtime, so fake non-null pointers are enough and no kernel is launched: -11
for dkv_is_16bit with hq != hk and -12 for dkv_is_16bit with a deterministic
GQA head split in cu_margin, both after the older codes and before the "no
range, nothing to do" return.

Host layer: the dtype rules of _flex_flash_attn_backward fire before anything
is launched; every call passes an EMPTY range table, with which the C entries
return before any launch even if a rule were missing."""
import ctypes

import pytest
import torch

from magi_attention import _ffa_lib

FP16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DKV_GQA, DKV_HEAD_SPLIT = -11, -12
DKV_DIRECT = ("magi_ffa_bwd_dkv_direct", "magi_ffa_bwd_dv_direct",
              "magi_ffa_bwd_dk_direct")
DIRECT_ENTRIES = ("magi_ffa_bwd_dq_direct",) + DKV_DIRECT
PLAIN_ENTRIES = ("magi_ffa_bwd_preprocess", "magi_ffa_bwd_dq",
                 "magi_ffa_bwd_dkv", "magi_ffa_bwd_dv", "magi_ffa_bwd_dk",
                 "magi_ffa_bwd")


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _bwd_args(**over):
    kw = dict(
        dout=1, q=1, k=1, v=1, out=1, lse=1, dq=1, dk=1, dv=1, dpsum=1,
        q_ranges=1, k_ranges=1, attn_type_map=None, seg_starts=None,
        n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_k=8,
        out_is_fp32=0, softmax_scale=1.0, softcap=0.0, cu_margin=0,
        stream=None,
    )
    kw.update(over)
    return _ffa_lib.MagiFfaBwdDirectArgs(**kw)


# ───────────────────────── C ABI ─────────────────────────

def test_direct_args_size_and_layout():
    lib = _lib()
    base, cls = _ffa_lib.MagiFfaBwdArgs, _ffa_lib.MagiFfaBwdDirectArgs
    assert lib.magi_ffa_args_size(1) == ctypes.sizeof(base)
    assert lib.magi_ffa_bwd_direct_args_size() == ctypes.sizeof(cls)
    # the plain struct comes first, whole; the switches follow it
    assert issubclass(cls, base)
    assert [f[0] for f in cls._fields_] == ["dq_is_16bit", "dkv_is_16bit"]
    assert cls.dq_is_16bit.offset == ctypes.sizeof(base)
    assert cls.dkv_is_16bit.offset == ctypes.sizeof(base) + 4
    assert ctypes.sizeof(cls) == ctypes.sizeof(base) + 8
    for name, _ in base._fields_:
        assert getattr(cls, name).offset == getattr(base, name).offset, name
    a = cls()
    assert a.dq_is_16bit == 0 and a.dkv_is_16bit == 0


def test_zero_flags_with_no_range_return_0():
    """the plain entries on the plain struct, and on the longer one, which
    starts with it; the direct entries with a zero tail"""
    lib = _lib()
    # the preprocess has no range count: no row is its "nothing to do"
    kw = dict(n_ranges=0, total_q=0)
    plain = _ffa_lib.MagiFfaBwdArgs(**{
        n: getattr(_bwd_args(**kw), n) for n, _ in
        _ffa_lib.MagiFfaBwdArgs._fields_})
    longer = _bwd_args(**kw)
    assert longer.dq_is_16bit == 0 and longer.dkv_is_16bit == 0
    for name in PLAIN_ENTRIES:
        assert getattr(lib, name)(ctypes.byref(plain)) == 0, name
        assert getattr(lib, name)(longer) == 0, name
    for name in DIRECT_ENTRIES:
        assert getattr(lib, name)(ctypes.byref(longer)) == 0, name


@pytest.mark.parametrize("elem_type", [0, 1], ids=["bf16", "fp16"])
def test_set_flags_with_no_range_return_0(elem_type):
    lib = _lib()
    a = _bwd_args(n_ranges=0, total_q=0, hq=2, hk=2, elem_type=elem_type,
                  dq_is_16bit=1, dkv_is_16bit=1)
    for name in DIRECT_ENTRIES:
        assert getattr(lib, name)(ctypes.byref(a)) == 0, name


@pytest.mark.parametrize("n_ranges", [0, 1])
def test_direct_dkv_refuses_gqa(n_ranges):
    """hq = 4, hk = 2: two q heads add into every dK/dV row. Refused before
    any launch, with a range (fake pointers: a launch would fault) and
    without."""
    lib = _lib()
    a = _bwd_args(dkv_is_16bit=1, n_ranges=n_ranges)
    for name in DKV_DIRECT:
        assert getattr(lib, name)(ctypes.byref(a)) == DKV_GQA, name
    # the dq pass has one owner per element whatever the head ratio
    b = _bwd_args(dq_is_16bit=1, n_ranges=0)
    assert lib.magi_ffa_bwd_dq_direct(ctypes.byref(b)) == 0
    # and with the switch off GQA is what it always was
    c = _bwd_args(dq_is_16bit=1, n_ranges=0)
    for name in DKV_DIRECT:
        assert getattr(lib, name)(ctypes.byref(c)) == 0, name


def test_direct_dkv_refuses_a_head_split():
    """(mult << 24) | (off << 16) in cu_margin is the deterministic GQA
    sub-launch; the low 16 bits, the CU margin proper, are not."""
    lib = _lib()
    a = _bwd_args(dkv_is_16bit=1, hq=2, hk=2, cu_margin=(2 << 24) | (1 << 16))
    for name in DKV_DIRECT:
        assert getattr(lib, name)(ctypes.byref(a)) == DKV_HEAD_SPLIT, name
    b = _bwd_args(dkv_is_16bit=1, hq=2, hk=2, cu_margin=8, n_ranges=0)
    for name in DKV_DIRECT:
        assert getattr(lib, name)(ctypes.byref(b)) == 0, name
    # hq != hk is looked at first
    c = _bwd_args(dkv_is_16bit=1, cu_margin=(2 << 24) | (1 << 16))
    assert lib.magi_ffa_bwd_dkv_direct(ctypes.byref(c)) == DKV_GQA


def test_older_codes_come_first():
    lib = _lib()
    for name in DIRECT_ENTRIES:
        fn = getattr(lib, name)
        both = dict(dq_is_16bit=1, dkv_is_16bit=1)
        assert fn(None) == -1
        assert fn(ctypes.byref(_bwd_args(q=None, **both))) == -1
        assert fn(ctypes.byref(_bwd_args(d=96, **both))) == -2
        assert fn(ctypes.byref(_bwd_args(hk=3, **both))) == -3
        assert fn(ctypes.byref(_bwd_args(elem_type=2, **both))) == -9


# ───────────────────────── host layer ─────────────────────────

def _backward(dtype=BF16, hq=2, hk=2, **over):
    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_backward,
    )

    q = torch.zeros(4, hq, 64, dtype=dtype)
    k = torch.zeros(6, hk, 64, dtype=dtype)
    empty = torch.zeros(0, 2, dtype=torch.int32)
    kw = dict(
        dout=torch.zeros_like(q), q=q, k=k, v=k.clone(), sink=None,
        sink_layout="sh", out=torch.zeros_like(q),
        lse=torch.zeros(4, hq), dq=None, dk=None, dv=None, dsink=None,
        q_ranges=empty, k_ranges=empty.clone(), attn_type_map=None,
        softmax_scale=1.0, softcap=0.0, dq_type=None, dk_type=None,
        dv_type=None, disable_bwd_dkv_atomic_reduction=False,
        deterministic=False, sm_margin=0, max_seqlen_k=0,
    )
    kw.update(over)
    return _flex_flash_attn_backward(**kw)


@pytest.mark.parametrize("which", ["dk_type", "dv_type"])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_16bit_dkv_type_needs_the_flag(dtype, which):
    with pytest.raises(AssertionError,
                       match="needs disable_bwd_dkv_atomic_reduction"):
        _backward(dtype, **{which: dtype})
    with pytest.raises(AssertionError,
                       match="needs disable_bwd_dkv_atomic_reduction"):
        _backward(dtype, **{which[:2]: torch.zeros(6, 2, 64, dtype=dtype)})


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_16bit_dq_type_needs_the_flag(dtype):
    with pytest.raises(AssertionError,
                       match="needs disable_bwd_dq_atomic_reduction"):
        _backward(dtype, dq_type=dtype)
    # the dK/dV promise says nothing about the q ranges
    with pytest.raises(AssertionError,
                       match="needs disable_bwd_dq_atomic_reduction"):
        _backward(dtype, dq_type=dtype, disable_bwd_dkv_atomic_reduction=True)


@pytest.mark.parametrize("qd,gd", [(FP16, BF16), (BF16, FP16)],
                         ids=["fp16q-bf16grad", "bf16q-fp16grad"])
def test_other_16bit_type_is_rejected(qd, gd):
    both = dict(disable_bwd_dkv_atomic_reduction=True,
                disable_bwd_dq_atomic_reduction=True)
    for which in ("dq_type", "dk_type", "dv_type"):
        with pytest.raises(AssertionError,
                           match="must be float32 or q's own 16-bit type"):
            _backward(qd, **{which: gd}, **both)


def test_16bit_dkv_with_gqa_is_rejected():
    """With hq != hk the flag falls back to f32; an explicit 16-bit dk_type
    cannot be honoured."""
    with pytest.raises(AssertionError, match=r"hq == hk \(hq=4, hk=2\)"):
        _backward(BF16, hq=4, hk=2, dk_type=BF16,
                  disable_bwd_dkv_atomic_reduction=True)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_struct_flags_follow_the_buffer_dtypes(monkeypatch, dtype):
    """_ffa_launch.bwd_args fills the two members from the buffers it is
    given (torch cannot name a current stream without a device; the null
    stream stands in, nothing is launched)."""
    from magi_attention.functional import _ffa_launch

    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    q = torch.zeros(4, 2, 64, dtype=dtype)
    k = torch.zeros(6, 2, 64, dtype=dtype)
    dpsum = torch.zeros(4, 2)

    def flags(dq, dk, dv):
        a = _ffa_launch.bwd_args(q, q, dpsum, q=q, k=k, v=k, lse=dpsum,
                                 dq=dq, dk=dk, dv=dv)
        return a.dq_is_16bit, a.dkv_is_16bit

    def f32(t):
        return torch.zeros_like(t, dtype=F32)

    assert flags(f32(q), f32(k), f32(k)) == (0, 0)
    assert flags(q, f32(k), f32(k)) == (1, 0)
    assert flags(f32(q), k, k) == (0, 1)
    assert flags(q, k, k) == (1, 1)
    assert flags(None, None, None) == (0, 0)
    with pytest.raises(AssertionError, match="share a dtype"):
        flags(f32(q), k, f32(k))


def test_launch_helpers_take_either_struct():
    """run_bwd_passes / run_bwd_deterministic pick the *_direct entries for the
    struct bwd_args() builds and the plain ones for a bare MagiFfaBwdArgs,
    which the stand-alone probes fill by hand."""
    from magi_attention.functional._ffa_launch import _bwd_entries

    lib = _lib()
    names = ("dq", "dkv", "dv", "dk")
    plain = _bwd_entries(_ffa_lib.MagiFfaBwdArgs(n_ranges=0))
    assert plain == tuple(getattr(lib, f"magi_ffa_bwd_{n}") for n in names)
    direct = _bwd_entries(_bwd_args(n_ranges=0))
    assert direct == tuple(
        getattr(lib, f"magi_ffa_bwd_{n}_direct") for n in names)
    for fn in plain:
        assert fn(_ffa_lib.MagiFfaBwdArgs(
            dout=1, q=1, k=1, v=1, lse=1, hq=2, hk=2, d=64, n_ranges=0)) == 0
