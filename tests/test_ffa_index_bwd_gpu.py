"""GPU parity tests for the index-attention backward (csrc/ffa_index_bwd.hip
through flex_flash_attn_func(..., index_attn_indices=...) under autograd).

Oracle: a gather-based PyTorch attention written here (NOT the dense mask):
K/V rows are gathered with the index lists, padding slots are set to -inf,
and autograd through the indexing produces the scatter gradients. It is
evaluated twice per case, in fp64 (ref_hi) and in bf16 on the same bf16
inputs (ref_lo); out/dq/dk/dv are held to tests/util.py::assert_close_to_ref
with its default ratio and floor, so every budget is measured
from the bf16 oracle on that case and printed.

All tensors use the folded layout the kernel takes: q [(b s h_kv), ratio, d],
k/v [(b s h_kv), 1, d], global id = (b*S_kv + t)*NHK + h_kv.
"""
import pytest
import torch

from tests.util import assert_close_to_ref

pytestmark = pytest.mark.gpu

from magi_attention.utils import build_index_attn_indices  # noqa: E402

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


def _oracle(q, k, v, idx2d, dout, scale, softcap, dtype):
    """Gather-based attention + autograd in `dtype`. Returns out, dq, dk, dv."""
    q = q.detach().to(dtype).requires_grad_(True)
    k = k.detach().to(dtype).requires_grad_(True)
    v = v.detach().to(dtype).requires_grad_(True)
    valid = idx2d >= 0
    g = idx2d.clamp_min(0).long()
    kg = k[g, 0]  # [T, M, D]
    vg = v[g, 0]
    s = torch.einsum("thd,tmd->thm", q, kg) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)
    out = torch.einsum("thm,tmd->thd", p, vg)
    out.backward(dout.to(dtype))
    return out.detach(), q.grad, k.grad, v.grad


def _make(B, S_q, S_kv, NHQ, NHK, D, topk, max_topk, seed, indices=None):
    torch.manual_seed(seed)
    dev = "cuda"
    ratio = NHQ // NHK
    q = torch.randn(B * S_q * NHK, ratio, D, dtype=torch.bfloat16, device=dev)
    k = torch.randn(B * S_kv * NHK, 1, D, dtype=torch.bfloat16, device=dev)
    v = torch.randn(B * S_kv * NHK, 1, D, dtype=torch.bfloat16, device=dev)
    dout = torch.randn_like(q)
    if indices is None:
        indices = build_index_attn_indices(
            B, NHK, S_q, S_kv, topk, max_topk, device=dev
        )
    return q, k, v, dout, indices


def _run_kernel(q, k, v, dout, indices, softcap=0.0, **kw):
    from magi_attention.functional import flex_flash_attn_func

    qg = q.detach().clone().requires_grad_(True)
    kg = k.detach().clone().requires_grad_(True)
    vg = v.detach().clone().requires_grad_(True)
    out, meta = flex_flash_attn_func(
        qg, kg, vg, index_attn_indices=indices, softcap=softcap, **kw
    )
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), meta, qg.grad, kg.grad, vg.grad


def _check_case(B, S_q, S_kv, NHQ, NHK, D, topk, max_topk, seed=0,
                softcap=0.0, indices=None):
    q, k, v, dout, indices = _make(
        B, S_q, S_kv, NHQ, NHK, D, topk, max_topk, seed, indices
    )
    out, meta, dq, dk, dv = _run_kernel(q, k, v, dout, indices, softcap)
    idx2d = indices.reshape(-1, indices.shape[-1])
    scale = D ** (-0.5)
    hi = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.float64)
    lo = _oracle(q, k, v, idx2d, dout, scale, softcap, torch.bfloat16)
    for name, got, h, l in zip(("out", "dq", "dk", "dv"),
                               (out, dq, dk, dv), hi, lo):
        assert got.shape == h.shape
        assert torch.isfinite(got).all(), f"{name} has non-finite values"
        assert_close_to_ref(got, h, l, name)
    return (q, k, v, dout, idx2d), (out, meta, dq, dk, dv)


@requires_gpu
@pytest.mark.parametrize(
    "ratio,nhk", [(128, 1), (64, 1), (32, 2), (8, 1), (1, 4)]
)
def test_index_bwd_gqa_ratios(ratio, nhk):
    """W = 4/2/1 head blocks, partial head blocks (8 and 1 of 32 lanes), a
    half-valid second 32-row subtile (topk 48) and -1 tail padding."""
    _check_case(B=2, S_q=33, S_kv=128, NHQ=ratio * nhk, NHK=nhk, D=128,
                topk=48, max_topk=64, seed=ratio)


@requires_gpu
def test_index_bwd_cross_batch_topk():
    """Multi-tile lists (up to 8 gathered tiles), per-batch topk."""
    _check_case(B=3, S_q=16, S_kv=256, NHQ=64, NHK=1, D=128,
                topk=[17, 192, 256], max_topk=256, seed=7)


@requires_gpu
@pytest.mark.parametrize("d", [64, 96])
def test_index_bwd_head_dims(d):
    """D=64 bucket, and D=96 through the zero-pad path (autograd through
    F.pad and the output slice)."""
    _check_case(B=2, S_q=24, S_kv=192, NHQ=32, NHK=1, D=d,
                topk=64, max_topk=64, seed=d)


@requires_gpu
def test_index_bwd_softcap():
    """softcap=2.0: 1 - tanh^2 is far from 1 on unit-variance scores."""
    _check_case(B=1, S_q=16, S_kv=128, NHQ=64, NHK=1, D=128,
                topk=64, max_topk=64, seed=3, softcap=2.0)


@requires_gpu
def test_index_bwd_all_padding_rows():
    """Rows whose whole list is -1: dq exactly 0, every gradient finite."""
    B, S_q, S_kv, NHQ, NHK, D = 1, 8, 64, 32, 1, 128
    idx = build_index_attn_indices(B, NHK, S_q, S_kv, 32, 64, device="cuda")
    idx[2] = -1
    idx[5] = -1
    _, (out, meta, dq, dk, dv) = _check_case(
        B, S_q, S_kv, NHQ, NHK, D, topk=None, max_topk=64, seed=17,
        indices=idx,
    )
    assert (dq[2] == 0).all() and (dq[5] == 0).all()
    assert (out[2] == 0).all() and (out[5] == 0).all()
    for t in (dq, dk, dv):
        assert torch.isfinite(t).all()


@requires_gpu
def test_index_bwd_scatter_contention_and_sparsity():
    """Every q row lists the same 64 K rows: 64 contributions per listed
    row; the 192 unlisted rows of dk/dv receive no atomic and stay 0.0."""
    B, S_q, S_kv, NHQ, NHK, D = 1, 64, 256, 32, 1, 128
    torch.manual_seed(23)
    listed = torch.randperm(S_kv, device="cuda")[:64].sort().values.int()
    idx = listed.view(1, 1, 64).expand(S_q, 1, 64).contiguous()
    _, (out, meta, dq, dk, dv) = _check_case(
        B, S_q, S_kv, NHQ, NHK, D, topk=None, max_topk=64, seed=23,
        indices=idx,
    )
    unlisted = torch.ones(S_kv, dtype=torch.bool, device="cuda")
    unlisted[listed.long()] = False
    assert int(unlisted.sum()) == 192
    assert (dk[unlisted] == 0).all()
    assert (dv[unlisted] == 0).all()
    assert (dk[~unlisted] != 0).any() and (dv[~unlisted] != 0).any()


@requires_gpu
def test_index_bwd_long_sequence_ids():
    """S_kv=65536: scatter row offsets g*D*4 B reach 2^25 B and the ids near
    2^16 exercise the 64-bit row arithmetic of gather and scatter."""
    _check_case(B=1, S_q=4, S_kv=65536, NHQ=64, NHK=1, D=128,
                topk=128, max_topk=128, seed=13)


@requires_gpu
def test_index_bwd_plumbing():
    from magi_attention.functional import flex_flash_attn_func

    B, S_q, S_kv, NHQ, NHK, D = 1, 8, 128, 32, 1, 128
    q, k, v, dout, idx = _make(B, S_q, S_kv, NHQ, NHK, D, 40, 64, seed=29)

    # gradient dtypes equal input dtypes; out/lse bit-identical to no_grad
    out, meta, dq, dk, dv = _run_kernel(q, k, v, dout, idx)
    assert dq.dtype == q.dtype and dk.dtype == k.dtype and dv.dtype == v.dtype
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    with torch.no_grad():
        out_ng, meta_ng = flex_flash_attn_func(q, k, v, index_attn_indices=idx)
    assert torch.equal(out, out_ng)
    assert torch.equal(meta.lse, meta_ng.lse)
    assert not meta.lse.requires_grad

    # only q requires grad
    qg = q.clone().requires_grad_(True)
    o, _ = flex_flash_attn_func(qg, k, v, index_attn_indices=idx)
    o.backward(dout)
    assert torch.equal(qg.grad, dq) and k.grad is None and v.grad is None
    # the autograd node itself hands back None for the frozen inputs
    o2, _ = flex_flash_attn_func(qg, k, v, index_attn_indices=idx)
    grads = o2.grad_fn.apply(dout, None)
    assert len(grads) == 6
    assert torch.equal(grads[0], dq)
    assert all(g is None for g in grads[1:])

    # only k and v require grad (dk/dv are atomically accumulated: compare
    # with the calibrated budget of this case, not bitwise)
    kg = k.clone().requires_grad_(True)
    vg = v.clone().requires_grad_(True)
    o, _ = flex_flash_attn_func(q, kg, vg, index_attn_indices=idx)
    o.backward(dout)
    assert q.grad is None
    assert kg.grad is not None and vg.grad is not None
    idx2d = idx.reshape(-1, idx.shape[-1])
    hi = _oracle(q, k, v, idx2d, dout, D ** (-0.5), 0.0, torch.float64)
    lo = _oracle(q, k, v, idx2d, dout, D ** (-0.5), 0.0, torch.bfloat16)
    assert_close_to_ref(kg.grad, hi[2], lo[2], "dk (q frozen)")
    assert_close_to_ref(vg.grad, hi[3], lo[3], "dv (q frozen)")

    # no deterministic scatter: rejected when a gradient is needed
    with pytest.raises(AssertionError, match="deterministic"):
        flex_flash_attn_func(
            qg, k, v, index_attn_indices=idx, deterministic=True
        )
    # ... and still accepted on the no-grad forward
    with torch.no_grad():
        flex_flash_attn_func(
            qg, k, v, index_attn_indices=idx, deterministic=True
        )
