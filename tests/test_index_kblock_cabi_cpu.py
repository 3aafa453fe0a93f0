"""C-ABI surface of k_block_size on the index path (include/magi_ffa.h
magi_ffa_fwd_index_kblock / magi_ffa_fwd_index_fp8_kblock /
magi_ffa_bwd_index_kblock): the symbols and their ctypes mirrors exist and
agree in size, and validation runs in the embedded entries' order with their
codes - the -4 rule now on max_topk * k_block_size - then the new
k_block_size code, all BEFORE any GPU work (fake non-null pointers, no kernel
is launched)."""
import ctypes

import pytest

from magi_attention import _ffa_lib

_BASE = dict(q=1, k=1, v=1, indices_2d=1, total_q=8, total_k=8, max_topk=64,
             hq=4, hk=1, d=128, softmax_scale=1.0, softcap=0.0, stream=None,
             k_block_size=16)
_FWD = dict(out=1, lse=1, out_is_fp32=0)
# entry: (args mirror, its other arguments, code for q_block_size < 1 or None
# where the struct has none, code for a bad k_block_size)
ENTRIES = {
    "magi_ffa_fwd_index_kblock": (
        "MagiFfaIndexKBlockArgs", dict(_FWD, q_block_size=4), -6, -7),
    "magi_ffa_fwd_index_fp8_kblock": (
        "MagiFfaIndexFp8KBlockArgs", _FWD, None, -6),
    "magi_ffa_bwd_index_kblock": (
        "MagiFfaIndexBwdKBlockArgs",
        dict(dout=1, lse=1, dpsum=1, dq=1, dk=1, dv=1, q_block_size=4), -5, -6),
}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_index_kblock_entry(entry):
    lib = _ffa_lib.lib()
    mirror, extra, bad_q, bad_k = ENTRIES[entry]
    cls = getattr(_ffa_lib, mirror)
    fn = getattr(lib, entry)
    assert fn.argtypes == [ctypes.POINTER(cls)] and fn.restype is ctypes.c_int
    assert getattr(lib, entry + "_args_size")() == ctypes.sizeof(cls)
    assert [f[0] for f in cls._fields_] == ["k_block_size", "k_reserved"]
    assert cls.k_block_size.offset == ctypes.sizeof(cls.__mro__[1])
    assert hasattr(cls, "q_block_size") == (bad_q is not None)

    def rc(**over):
        return fn(ctypes.byref(cls(**{**_BASE, **extra, **over})))

    assert fn(None) == -1
    for field in ("q", "k", "v", "indices_2d", *extra):
        if field not in ("out_is_fp32", "q_block_size"):
            assert rc(**{field: None}) == -1, field
    # each embedded code wins over the ones after it, k_block_size comes last
    assert rc(d=96, hk=2, max_topk=50, k_block_size=0) == -2
    assert rc(hk=2, max_topk=50, k_block_size=0) == -3
    assert rc(max_topk=50, k_block_size=0) == -4  # a bad Bk is judged as 1
    # -4 is on max_topk * Bk: 3 * 64 passes, 3 * 16 does not
    assert rc(max_topk=3, k_block_size=64, total_q=0) == 0
    assert rc(max_topk=3, k_block_size=16) == -4
    assert rc(max_topk=0, k_block_size=64) == -4
    if "out" in extra:
        assert rc(sink=1, s_sink=9, k_block_size=0) == -5
    if bad_q is not None:
        assert rc(q_block_size=0, k_block_size=0) == bad_q
    for bad in (0, 1, 3, -4):
        assert rc(k_block_size=bad) == bad_k
        assert rc(k_block_size=bad, total_q=0) == bad_k
    assert rc(max_topk=1 << 26, k_block_size=64) == bad_k  # past int32
    assert rc(total_q=0) == 0 and rc(total_q=-3) == 0
