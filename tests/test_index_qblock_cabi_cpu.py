"""C-ABI surface of q_block_size on the index path (include/magi_ffa.h
magi_ffa_fwd_index_block / magi_ffa_bwd_index_block): the symbols and their
ctypes mirrors exist and agree in size, and validation runs in the base
entries' order with their codes, then the new q_block_size code, all BEFORE
any GPU work (fake non-null pointers, no kernel is launched)."""
import ctypes

import pytest

from magi_attention import _ffa_lib

_BASE = dict(q=1, k=1, v=1, indices_2d=1, total_q=8, total_k=8, max_topk=64,
             hq=4, hk=1, d=128, softmax_scale=1.0, softcap=0.0, stream=None,
             q_block_size=4)
# entry: (args mirror, its other pointers, code for q_block_size < 1)
ENTRIES = {
    "magi_ffa_fwd_index_block": (
        "MagiFfaIndexBlockArgs", dict(out=1, lse=1, out_is_fp32=0), -6),
    "magi_ffa_bwd_index_block": (
        "MagiFfaIndexBwdBlockArgs",
        dict(dout=1, lse=1, dpsum=1, dq=1, dk=1, dv=1), -5),
}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_index_block_entry(entry):
    lib = _ffa_lib.lib()
    mirror, ptrs, bad_block = ENTRIES[entry]
    cls = getattr(_ffa_lib, mirror)
    fn = getattr(lib, entry)
    assert fn.argtypes == [ctypes.POINTER(cls)] and fn.restype is ctypes.c_int
    assert getattr(lib, entry + "_args_size")() == ctypes.sizeof(cls)
    assert [f[0] for f in cls._fields_] == ["q_block_size", "reserved"]
    assert cls.q_block_size.offset == ctypes.sizeof(cls.__mro__[1])

    def rc(**over):
        return fn(ctypes.byref(cls(**{**_BASE, **ptrs, **over})))

    assert fn(None) == -1
    for field in ("q", "k", "v", "indices_2d", *ptrs):
        if field != "out_is_fp32":
            assert rc(**{field: None}) == -1, field
    # each base code wins over the ones after it, q_block_size < 1 comes last
    assert rc(d=96, hk=2, max_topk=50, q_block_size=0) == -2
    assert rc(hk=2, max_topk=50, q_block_size=0) == -3
    assert rc(max_topk=50, q_block_size=0) == -4
    if entry == "magi_ffa_fwd_index_block":
        assert rc(sink=1, s_sink=9, q_block_size=0) == -5
    for bad in (0, -4):
        assert rc(q_block_size=bad) == bad_block
        assert rc(q_block_size=bad, total_q=0) == bad_block
    assert rc(total_q=0) == 0 and rc(total_q=-3) == 0

