"""cat_gqa of the dense backward, everything that needs no GPU.

ABI: magi_ffa_bwd_args and magi_ffa_bwd_direct_args keep their sizes, which
tests/test_ffa_fp16_cpu.py and tests/test_ffa_bwd_direct_cpu.py pin; the
switch cat_gqa and a reserved word ride behind an embedded
magi_ffa_bwd_direct_args in magi_ffa_bwd_cat_args, which the
magi_ffa_bwd_{dkv,dv,dk}_cat entries take. The C entries validate before they
touch a pointer or the HIP runtime, so fake non-null pointers are enough and
no kernel is launched. With cat_gqa = 0 an entry is its _direct twin (-11 and
-12 included); with cat_gqa = 1 a 16-bit dK/dV with hq != hk is accepted, a
deterministic GQA head split in cu_margin is -13 and reserved != 0 is -14,
all after the older codes and before the "no range, nothing to do" return.

Host layer: the dtype rules of _flex_flash_attn_backward fire before anything
is launched; every call passes an EMPTY range table, with which the C entries
return before any launch. launch_per_group / run_bwd_deterministic run over
CPU tensors with a recording function in place of the C entries."""
import ctypes

import pytest
import torch

from magi_attention import _ffa_lib

BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
DKV_GQA, DKV_HEAD_SPLIT, CAT_HEAD_SPLIT, CAT_RESERVED = -11, -12, -13, -14
HEAD_SPLIT = (2 << 24) | (1 << 16)
CAT_ENTRIES = ("magi_ffa_bwd_dkv_cat", "magi_ffa_bwd_dv_cat",
               "magi_ffa_bwd_dk_cat")


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _cat_args(**over):
    kw = dict(
        dout=1, q=1, k=1, v=1, out=1, lse=1, dq=1, dk=1, dv=1, dpsum=1,
        q_ranges=1, k_ranges=1, attn_type_map=None, seg_starts=None,
        n_ranges=1, total_q=8, total_k=8, hq=4, hk=2, d=128, max_seqlen_k=8,
        out_is_fp32=0, softmax_scale=1.0, softcap=0.0, cu_margin=0,
        stream=None,
    )
    kw.update(over)
    return _ffa_lib.MagiFfaBwdCatArgs(**kw)


# ───────────────────────── C ABI ─────────────────────────

def test_cat_symbols_exist():
    lib = _lib()
    for name in CAT_ENTRIES + ("magi_ffa_bwd_cat_args_size",):
        assert getattr(lib, name) is not None, name
    assert hasattr(_ffa_lib, "MagiFfaBwdCatArgs")


def test_cat_args_size_and_layout():
    lib = _lib()
    base, direct, cls = (_ffa_lib.MagiFfaBwdArgs, _ffa_lib.MagiFfaBwdDirectArgs,
                         _ffa_lib.MagiFfaBwdCatArgs)
    assert lib.magi_ffa_bwd_cat_args_size() == ctypes.sizeof(cls)
    # the embedded structs keep their sizes
    assert lib.magi_ffa_args_size(1) == ctypes.sizeof(base)
    assert lib.magi_ffa_bwd_direct_args_size() == ctypes.sizeof(direct)
    assert ctypes.sizeof(direct) == ctypes.sizeof(base) + 8
    # the direct struct comes first, whole; the switch and reserved follow it
    assert issubclass(cls, direct) and issubclass(direct, base)
    assert [f[0] for f in cls._fields_] == ["cat_gqa", "reserved"]
    assert cls.cat_gqa.offset == ctypes.sizeof(direct)
    assert cls.reserved.offset == ctypes.sizeof(direct) + 4
    assert ctypes.sizeof(cls) == ctypes.sizeof(direct) + 8
    for name, _ in base._fields_ + direct._fields_:
        assert getattr(cls, name).offset == getattr(direct, name).offset, name
    a = cls()
    assert a.cat_gqa == 0 and a.reserved == 0


@pytest.mark.parametrize("n_ranges", [0, 1])
def test_cat_off_is_the_direct_entry(n_ranges):
    """cat_gqa = 0 through the _cat entries: -11 and -12 as the _direct twins
    give them, with a range (fake pointers: a launch would fault) and without;
    reserved is not read."""
    lib = _lib()
    for reserved in (0, 7):
        a = _cat_args(dkv_is_16bit=1, n_ranges=n_ranges, reserved=reserved)
        b = _cat_args(dkv_is_16bit=1, hq=2, hk=2, cu_margin=HEAD_SPLIT,
                      n_ranges=n_ranges, reserved=reserved)
        for name in CAT_ENTRIES:
            twin = getattr(lib, name.replace("_cat", "_direct"))
            assert getattr(lib, name)(ctypes.byref(a)) == DKV_GQA, name
            assert twin(ctypes.byref(a)) == DKV_GQA, name
            assert getattr(lib, name)(ctypes.byref(b)) == DKV_HEAD_SPLIT, name
            assert twin(ctypes.byref(b)) == DKV_HEAD_SPLIT, name
    # f32 dK/dV under GQA, with a head split: what it always was
    c = _cat_args(cu_margin=HEAD_SPLIT, n_ranges=0)
    for name in CAT_ENTRIES:
        assert getattr(lib, name)(ctypes.byref(c)) == 0, name


@pytest.mark.parametrize("elem_type", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hq,hk", [(4, 2), (6, 2), (8, 1), (2, 2)])
def test_cat_on_accepts_16bit_dkv_under_gqa(hq, hk, elem_type):
    lib = _lib()
    for dkv16 in (0, 1):
        a = _cat_args(cat_gqa=1, dkv_is_16bit=dkv16, hq=hq, hk=hk,
                      n_ranges=0, elem_type=elem_type, cu_margin=8)
        for name in CAT_ENTRIES:
            assert getattr(lib, name)(ctypes.byref(a)) == 0, (name, dkv16)
    # the struct passes as the two it starts with; they know no cat_gqa
    a = _cat_args(cat_gqa=1, dkv_is_16bit=1, hq=hq, hk=hk, n_ranges=0)
    want = 0 if hq == hk else DKV_GQA
    assert lib.magi_ffa_bwd_dkv_direct(a) == want
    assert lib.magi_ffa_bwd_dkv(a) == 0


@pytest.mark.parametrize("n_ranges", [0, 1])
def test_cat_on_refuses_a_head_split_and_reserved(n_ranges):
    lib = _lib()
    split = _cat_args(cat_gqa=1, cu_margin=HEAD_SPLIT, n_ranges=n_ranges)
    resv = _cat_args(cat_gqa=1, reserved=1, n_ranges=n_ranges)
    both = _cat_args(cat_gqa=1, cu_margin=HEAD_SPLIT, reserved=1,
                     n_ranges=n_ranges)
    # with a direct store the head split is the older -12
    split16 = _cat_args(cat_gqa=1, dkv_is_16bit=1, cu_margin=HEAD_SPLIT,
                        n_ranges=n_ranges)
    for name in CAT_ENTRIES:
        fn = getattr(lib, name)
        assert fn(ctypes.byref(split)) == CAT_HEAD_SPLIT, name
        assert fn(ctypes.byref(resv)) == CAT_RESERVED, name
        assert fn(ctypes.byref(both)) == CAT_HEAD_SPLIT, name
        assert fn(ctypes.byref(split16)) == DKV_HEAD_SPLIT, name


def test_older_codes_come_first():
    lib = _lib()
    for name in CAT_ENTRIES:
        fn = getattr(lib, name)
        bad = dict(cat_gqa=1, dkv_is_16bit=1, cu_margin=HEAD_SPLIT, reserved=1)
        assert fn(None) == -1
        assert fn(ctypes.byref(_cat_args(q=None, **bad))) == -1
        assert fn(ctypes.byref(_cat_args(d=96, **bad))) == -2
        assert fn(ctypes.byref(_cat_args(hk=3, **bad))) == -3
        assert fn(ctypes.byref(_cat_args(elem_type=2, **bad))) == -9


# ───────────────────────── host layer ─────────────────────────

def _backward(dtype=BF16, hq=4, hk=2, **over):
    """_flex_flash_attn_backward over CPU tensors and empty range tables: the
    rules under test fire before anything is launched."""
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


@pytest.fixture
def no_device(monkeypatch):
    """What an accepted call needs a device for, replaced: the null stream
    stands in for torch's current one, the dpsum preprocess (it has no range
    count to return on) is left out, and in place of the two-stream pass
    scheduling the struct goes straight to the entries that scheduling would
    call, which return 0 on the empty table before any launch. Returns the
    list of structs seen."""
    from magi_attention.functional import _ffa_launch

    seen = []

    def run_bwd(args, q_ranges, k_ranges, attn_type_map, device, **kw):
        assert args.n_ranges == 0
        seen.append(args)
        for fn in _ffa_launch._bwd_entries(args):
            assert fn(args) == 0

    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(_ffa_launch, "bwd_preprocess", lambda args: None)
    monkeypatch.setattr(_ffa_launch, "run_bwd", run_bwd)
    return seen


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_16bit_dkv_with_gqa_and_cat_is_accepted(no_device, dtype):
    """fails at the parent commit, where cat_gqa is swallowed and hq != hk
    refuses a 16-bit dk_type"""
    _lib()
    dq, dk, dv, _ = _backward(dtype, dk_type=dtype, cat_gqa=True,
                              disable_bwd_dkv_atomic_reduction=True)
    assert (dq.dtype, dk.dtype, dv.dtype) == (F32, dtype, dtype)
    # the flag alone picks the 16-bit store under cat_gqa, as with hq == hk
    dq, dk, dv, _ = _backward(dtype, cat_gqa=True,
                              disable_bwd_dkv_atomic_reduction=True)
    assert (dq.dtype, dk.dtype, dv.dtype) == (F32, dtype, dtype)
    # and cat_gqa alone keeps the f32 accumulators
    dq, dk, dv, _ = _backward(dtype, cat_gqa=True)
    assert (dq.dtype, dk.dtype, dv.dtype) == (F32, F32, F32)
    assert [(a.cat_gqa, a.dkv_is_16bit) for a in no_device] == [
        (1, 1), (1, 1), (1, 0)]
    # a group of one head: cat_gqa is today's launch
    no_device.clear()
    _backward(dtype, hq=2, hk=2, cat_gqa=True)
    assert [a.cat_gqa for a in no_device] == [0]


def test_16bit_dkv_with_gqa_without_cat_keeps_the_old_message():
    with pytest.raises(AssertionError, match=r"hq == hk \(hq=4, hk=2\)"):
        _backward(BF16, dk_type=BF16, disable_bwd_dkv_atomic_reduction=True)
    with pytest.raises(AssertionError, match=r"hq == hk \(hq=4, hk=2\)"):
        _backward(BF16, dk_type=BF16, disable_bwd_dkv_atomic_reduction=True,
                  cat_gqa=False)
    # cat_gqa is no promise of disjoint k ranges: the flag is still needed
    with pytest.raises(AssertionError,
                       match="needs disable_bwd_dkv_atomic_reduction"):
        _backward(BF16, dk_type=BF16, cat_gqa=True)


def test_pack_gqa_and_cat_gqa_exclude_each_other():
    from magi_attention.functional import flex_flash_attn_func

    q = torch.zeros(4, 4, 64, dtype=BF16)
    k = torch.zeros(6, 2, 64, dtype=BF16)
    r = torch.zeros(0, 2, dtype=torch.int32)
    with pytest.raises(AssertionError,
                       match="pack_gqa and cat_gqa cannot be both True"):
        flex_flash_attn_func(q, k, k, r, r, None, pack_gqa=True, cat_gqa=True)


def test_struct_carries_cat_gqa(monkeypatch):
    from magi_attention.functional import _ffa_launch

    monkeypatch.setattr(_ffa_launch, "current_stream_ptr",
                        lambda: ctypes.c_void_p(0))
    q = torch.zeros(4, 4, 64, dtype=BF16)
    k = torch.zeros(6, 2, 64, dtype=BF16)
    dpsum = torch.zeros(4, 4)
    for cat in (False, True):
        a = _ffa_launch.bwd_args(q, q, dpsum, q=q, k=k, v=k, lse=dpsum,
                                 dk=k, dv=k, cat_gqa=cat)
        assert isinstance(a, _ffa_lib.MagiFfaBwdCatArgs)
        assert isinstance(a, _ffa_lib.MagiFfaBwdDirectArgs)
        assert (a.cat_gqa, a.reserved, a.dkv_is_16bit) == (int(cat), 0, 1)
    assert _ffa_launch.bwd_args(q, q, dpsum).cat_gqa == 0


def test_launch_helpers_pick_the_cat_entries():
    from magi_attention.functional._ffa_launch import _bwd_entries

    lib = _lib()
    got = _bwd_entries(_cat_args(n_ranges=0))
    assert got == (lib.magi_ffa_bwd_dq_direct, lib.magi_ffa_bwd_dkv_cat,
                   lib.magi_ffa_bwd_dv_cat, lib.magi_ffa_bwd_dk_cat)
    for fn in got:
        assert fn(_cat_args(n_ranges=0, cat_gqa=1, dkv_is_16bit=1)) == 0


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
@pytest.mark.parametrize("cat", [False, True], ids=["cat_off", "cat_on"])
def test_deterministic_launch_count(monkeypatch, cat, split):
    """hq = 8, hk = 2 (g = 4), two k-disjoint groups: with cat_gqa each group
    is ONE dkv launch and cu_margin's top bits stay 0; without, 4, one per
    member of the GQA group."""
    from magi_attention.functional import _ffa_launch

    calls = []

    def entry(what):
        def fn(args):
            calls.append((what, args.n_ranges, args.cu_margin))
            return 0
        return fn

    monkeypatch.setattr(
        _ffa_launch, "_bwd_entries",
        lambda args: tuple(entry(n) for n in ("dq", "dkv", "dv", "dk")))
    monkeypatch.setattr(_ffa_launch.env, "is_bwd_split_dkv",
                        lambda *_: split)
    # k ranges 0 and 2 are disjoint, 1 overlaps both: two k groups
    qr = torch.tensor([[0, 8], [8, 16], [16, 24]], dtype=torch.int32)
    kr = torch.tensor([[0, 8], [4, 12], [8, 16]], dtype=torch.int32)
    args = _cat_args(hq=8, hk=2, cat_gqa=int(cat), cu_margin=3, n_ranges=3)
    _ffa_launch.run_bwd_deterministic(args, qr, kr, None)

    passes = ("dv", "dk") if split else ("dkv",)
    dkv = [c for c in calls if c[0] != "dq"]
    assert [c[0] for c in calls if c[0] == "dq"] == ["dq"]  # q ranges disjoint
    per_group = 1 if cat else 4
    assert len(dkv) == len(passes) * 2 * per_group
    for what in passes:
        mine = [c for c in dkv if c[0] == what]
        assert sorted(c[1] for c in mine) == sorted(
            [2] * per_group + [1] * per_group)
        if cat:
            assert all(c[2] == 3 for c in mine), "top bits of cu_margin set"
        else:
            assert sorted({c[2] >> 16 for c in mine}) == [
                (4 << 8) | j for j in range(4)]
            assert all(c[2] & 0xFFFF == 3 for c in mine)
    assert args.cu_margin == 3
