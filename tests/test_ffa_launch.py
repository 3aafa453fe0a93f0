"""Host launch layer (magi_attention/functional/_ffa_launch.py) and the
autograd nodes' gradient count: every backward returns exactly one gradient
per forward input, taken from the forward signature."""
import ctypes
import inspect

import pytest
import torch

from magi_attention._ffa_lib import MagiFfaBwdArgs


def _n_inputs(func_cls):
    return len(inspect.signature(func_cls.forward).parameters) - 1  # ctx


def test_input_grads_follow_the_forward_signature():
    from magi_attention.functional.flex_flash_attn import (
        FlexFlashAttnFunc,
        IndexAttnFunc,
        IndexAttnSinkFunc,
        _input_grads,
    )

    assert _n_inputs(IndexAttnFunc) == 6 and _n_inputs(IndexAttnSinkFunc) == 9
    for cls in (FlexFlashAttnFunc, IndexAttnFunc, IndexAttnSinkFunc):
        names = list(inspect.signature(cls.forward).parameters)[1:]
        grads = _input_grads(cls, q="dq", k="dk", v="dv")
        assert len(grads) == _n_inputs(cls)
        assert grads[:3] == ("dq", "dk", "dv") and set(grads[3:]) == {None}
        if "sink" in names:
            grads = _input_grads(cls, sink="dsink")
            assert len(grads) == _n_inputs(cls)
            assert grads.index("dsink") == names.index("sink")
    with pytest.raises(AssertionError):
        _input_grads(IndexAttnFunc, sink="dsink")  # not an input of this node


def test_launch_per_group_subsets_tables_and_packs_head_splits():
    from magi_attention.functional._ffa_launch import launch_per_group

    qr = torch.tensor([[0, 4], [2, 6], [6, 8]], dtype=torch.int32)
    kr = torch.tensor([[0, 8], [8, 16], [16, 24]], dtype=torch.int32)
    tm = torch.tensor([0, 1, 2], dtype=torch.int32)
    args = MagiFfaBwdArgs(hq=6, hk=2, cu_margin=5)
    seen = []

    def read(p, n, cols):
        flat = (ctypes.c_int32 * (n * cols)).from_address(p)
        return [list(flat[i * cols:(i + 1) * cols]) for i in range(n)]

    def fn(a):
        n = a.n_ranges
        seen.append((read(a.q_ranges, n, 2), read(a.k_ranges, n, 2),
                     read(a.attn_type_map, n, 1), a.cu_margin))
        return 0

    launch_per_group(args, qr, kr, tm, [(fn, "one", [[0, 2], [1]], 1),
                                        (fn, "gqa", [[1, 2]], 3)])
    assert seen[0] == ([[0, 4], [6, 8]], [[0, 8], [16, 24]], [[0], [2]], 5)
    assert seen[1] == ([[2, 6]], [[8, 16]], [[1]], 5)
    # one launch per GQA member j: margin | gqa << 24 | j << 16
    assert [s[3] for s in seen[2:]] == [5 | 3 << 24 | j << 16 for j in range(3)]
    assert all(s[:3] == ([[2, 6], [6, 8]], [[8, 16], [16, 24]], [[1], [2]])
               for s in seen[2:])
    assert args.cu_margin == 5  # restored for the next pass

    # no type map: the pointer stays null
    launch_per_group(args, qr, kr, None,
                     [(lambda a: seen.append(a.attn_type_map) or 0, "x", [[0]], 1)])
    assert seen[-1] is None


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_flex_flash_attn_backward_gradient_count():
    from magi_attention.functional import flex_flash_attn_func
    from magi_attention.functional.flex_flash_attn import FlexFlashAttnFunc

    g = torch.Generator().manual_seed(5)
    q, k, v, dout = [
        (torch.randn(32, 1, 64, generator=g) * 0.5).bfloat16().cuda()
        for _ in range(4)
    ]
    q, k, v = [t.requires_grad_(True) for t in (q, k, v)]
    rng = torch.tensor([[0, 32]], dtype=torch.int32, device="cuda")
    tm = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, _ = flex_flash_attn_func(q, k, v, rng, rng, tm, deterministic=True)
    grads = out.grad_fn.apply(dout, None, None)
    assert len(grads) == _n_inputs(FlexFlashAttnFunc)
    out.backward(dout)
    for got, leaf, name in zip(grads, (q, k, v), ("dq", "dk", "dv")):
        assert torch.equal(got, leaf.grad), name
    assert all(x is None for x in grads[3:])
