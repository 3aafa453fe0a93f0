"""C-ABI surface of the index-attention sink / max_logits arguments
(include/magi_ffa.h magi_ffa_index_args: sink, s_sink, sink_ssh, max_logits,
appended after `stream`). Everything here comes back BEFORE any GPU work, so
it is checkable without a GPU: fake non-null pointers, no kernel is launched.

  - the optional tail sits at the C offsets, behind the original sixteen
    members, and a struct built without it has it zero-filled;
  - sink != NULL with s_sink outside [1, 8] returns -5 on both entries, after
    the older codes (-1, -2, -3, -4) and before the total_q <= 0 early-out;
  - a null sink accepts any s_sink;
  - _check_sink fires on CPU tensors through _flex_flash_attn_forward_index,
    before any native call.
"""
import ctypes

import pytest

from magi_attention import _ffa_lib


def _lib():
    if not _ffa_lib.is_available():
        pytest.skip("native library not built")
    return _ffa_lib.lib()


def _entries(lib):
    return (lib.magi_ffa_fwd_index, lib.magi_ffa_fwd_index_fp8)


def _args(**over):
    from magi_attention._ffa_lib import MagiFfaIndexArgs

    kw = dict(
        q=1, k=1, v=1, out=1, lse=1, indices_2d=1,
        total_q=8, total_k=8, max_topk=64, hq=4, hk=1, d=128,
        softmax_scale=1.0, softcap=0.0, out_is_fp32=0, stream=None,
    )
    kw.update(over)
    return MagiFfaIndexArgs(**kw)


def test_index_args_tail_layout():
    """The four new members follow `stream` at the offsets a C compiler gives
    `const float*; int32_t; int32_t; float*` (LP64), the old members keep
    theirs, and a struct built the old way has a zero tail."""
    from magi_attention._ffa_lib import MagiFfaIndexArgs

    a = _args()
    t = type(a)
    assert isinstance(a, MagiFfaIndexArgs)
    end = t.stream.offset + ctypes.sizeof(ctypes.c_void_p)
    assert MagiFfaIndexArgs.stream.offset == t.stream.offset == 96
    assert ctypes.sizeof(MagiFfaIndexArgs) == end
    assert t.sink.offset == end
    assert t.s_sink.offset == end + 8
    assert t.sink_ssh.offset == end + 12
    assert t.max_logits.offset == end + 16
    assert ctypes.sizeof(a) == end + 24
    assert a.sink is None and a.max_logits is None
    assert a.s_sink == 0 and a.sink_ssh == 0
    b = _args(sink=5, s_sink=3, sink_ssh=1, max_logits=7)
    assert (b.sink, b.s_sink, b.sink_ssh, b.max_logits) == (5, 3, 1, 7)
    assert (b.q, b.d, b.max_topk) == (1, 128, 64)


@pytest.mark.parametrize("s_sink", [0, 9, -1])
def test_index_sink_code_minus5(s_sink):
    lib = _lib()
    for fn in _entries(lib):
        a = _args(sink=1, s_sink=s_sink)
        assert fn(ctypes.byref(a)) == -5
        # -5 is a validation code: it comes before the empty-problem early-out
        a.total_q = 0
        assert fn(ctypes.byref(a)) == -5
        # either layout
        a.sink_ssh = 1
        assert fn(ctypes.byref(a)) == -5


def test_index_sink_older_codes_win():
    """Several faults at once: -1, -2, -3, -4 in their documented order, each
    ahead of -5."""
    lib = _lib()
    bad_sink = dict(sink=1, s_sink=9)
    for fn in _entries(lib):
        for over, code in (
            (dict(q=None, d=96, hk=2, max_topk=50), -1),
            (dict(d=96, hk=2, max_topk=50), -2),
            (dict(hk=2, max_topk=50), -3),
            (dict(max_topk=50, total_q=0), -4),
            (dict(total_q=0), -5),
            (dict(hq=0), -5),
        ):
            a = _args(**over, **bad_sink)
            assert fn(ctypes.byref(a)) == code, over
        # hq == 0 is an empty problem like total_q <= 0: after every
        # validation code it returns 0 without a launch (total_q stays 8)
        assert fn(ctypes.byref(_args(hq=0))) == 0
        assert fn(ctypes.byref(_args(hq=0, sink=1, s_sink=8, max_logits=1))) == 0
        assert fn(ctypes.byref(_args(hq=0, max_topk=50))) == -4


@pytest.mark.parametrize("s_sink", [0, 1, 8, 9, -1, 1 << 20])
def test_index_null_sink_accepts_any_s_sink(s_sink):
    lib = _lib()
    for fn in _entries(lib):
        a = _args(sink=None, s_sink=s_sink, total_q=0)
        assert fn(ctypes.byref(a)) == 0
    # a valid sink with nothing to do: 0 as well, no launch
    for fn in _entries(lib):
        for ok in (1, 8):
            a = _args(sink=1, s_sink=ok, total_q=0, max_logits=1)
            assert fn(ctypes.byref(a)) == 0


def test_index_check_sink_asserts_cpu():
    """_check_sink runs inside _flex_flash_attn_forward_index ahead of any
    allocation or native call, so CPU tensors reach it."""
    import torch

    from magi_attention.functional.flex_flash_attn import (
        _flex_flash_attn_forward_index,
    )

    tq, hq, d = 2, 4, 64
    q = torch.zeros(tq, hq, d, dtype=torch.bfloat16)
    k = torch.zeros(4, 1, d, dtype=torch.bfloat16)
    idx = torch.zeros(tq, 64, dtype=torch.int32)

    def call(sink, layout):
        _flex_flash_attn_forward_index(q, k, k, idx, 1.0, 0.0,
                                       sink=sink, sink_layout=layout)

    with pytest.raises(AssertionError, match=r"\[s_sink, hq\]"):
        call(torch.zeros(2, hq + 1), "sh")                  # wrong hq
    with pytest.raises(AssertionError, match=r"\[total_q, s_sink, hq\]"):
        call(torch.zeros(tq + 1, 2, hq), "ssh")             # wrong row count
    with pytest.raises(AssertionError, match=r"\[total_q, s_sink, hq\]"):
        call(torch.zeros(tq, 2, hq + 1), "ssh")             # wrong hq, ssh
    with pytest.raises(AssertionError, match="seqlen_sink"):
        call(torch.zeros(9, hq), "sh")                      # s_sink = 9
    with pytest.raises(AssertionError, match="seqlen_sink"):
        call(torch.zeros(tq, 9, hq), "ssh")
    with pytest.raises(AssertionError, match="sink_layout"):
        call(torch.zeros(2, hq), "hs")
    with pytest.raises(AssertionError, match=r"max_logits must be f32 \[hq\]"):
        _flex_flash_attn_forward_index(
            q, k, k, idx, 1.0, 0.0, max_logits=torch.zeros(hq + 1)
        )
