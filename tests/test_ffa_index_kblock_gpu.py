"""GPU parity tests for k_block_size > 1 on the index path:
flex_flash_attn_func(q, k, v, index_attn_indices=[lists of K BLOCK ids],
q_block_size=B, k_block_size=Bk) under autograd - the KBLOCK kernels of
csrc/ffa_index.hip, csrc/ffa_index_fp8.hip and csrc/ffa_index_bwd.hip.

Oracle: the gather-based PyTorch attention of tests/test_ffa_index_qblock_gpu.py
(copied, not imported) over the lists expanded here to per-token row ids
(id*Bk + arange(Bk); rows >= total_k and -1 entries become -1 in place), in
fp64 (ref_hi) and bf16 (ref_lo). Budgets are the index tests':
assert_close_to_ref at its defaults for out, dq, dk, dv, dsink; lse atol=3e-2,
rtol=3e-3 and max_logits atol=rtol=2e-2 against fp64. The fp8 case takes the
oracle and budgets of tests/test_ffa_index_fp8_gpu.py: dequantised inputs,
ref_lo of out in fp32 with P rounded to e4m3, gradients ratio 4.5, floor 9e-2.
S_KV = 250, so every Bk >= 4 has a ragged last block. Every parity case fails
on the parent commit at its k_block_size == 1 assertion.
"""
import pytest
import torch

from tests.util import assert_close_to_ref

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

S_KV = 250
FP8 = torch.float8_e4m3fn

# counts: valid ids per list, cycled. Generated lists never name block 0 (its
# rows must get no atomic) and put the last block - ragged for Bk >= 4 - at
# slot 1, in the middle of a list. bk64: max_topk not a multiple of 64, an
# all -1 list, the uniform-base arm. bk16: the per-lane arm, a ragged tile that
# is not the last, a half-valid tile. bk128: a block over several stages,
# ragged block 1 (122 rows) listed first. b3/b16: packed q rows straddle a
# wave; two workgroups per q block.
K4 = dict(Bk=32, hq=8, max_topk=4, counts=[4, 3])
CASES = {
    "bk64": dict(Bk=64, hq=8, max_topk=3, counts=[3, 1, 0]),
    "bk16": dict(Bk=16, hq=8, max_topk=12, counts=[12, 5]),
    "bk2": dict(Bk=2, hq=4, max_topk=64, counts=[64, 37]),
    "bk128": dict(Bk=128, hq=40, max_topk=2, lists=[[1, 0], [1, -1]]),
    "b3": dict(Bk=32, B=3, hq=24, tq=20, max_topk=4, counts=[4, 0, 3]),
    "b16": dict(Bk=64, B=16, hq=16, tq=40, max_topk=2, counts=[2, 1]),
    "d64": dict(K4, D=64),
    "d96": dict(K4, D=96),
    "softcap": dict(K4, softcap=2.0),
    "sink": dict(K4, counts=[4, 0, 3], sink=("sh", 2)),
    "fp8": dict(Bk=64, hq=8, max_topk=3, counts=[3, 1, 0], fp8=True),
}


def _oracle(q, k, v, idx2d, dout, scale, softcap, dtype, sink, p_dtype=None):
    q, k, v = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    valid = idx2d >= 0
    g = idx2d.clamp_min(0).long()
    s = torch.einsum("thd,tmd->thm", q, k[g, 0]) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    full, sk = s, None
    if sink is not None:  # "sh" layout
        sk = sink.detach().to(dtype).requires_grad_(True)
        full = torch.cat([s, sk.t().unsqueeze(0).expand(s.shape[0], -1, -1)], -1)
    p = torch.softmax(full, dim=-1).nan_to_num(0.0)[..., :s.shape[-1]]
    if p_dtype is not None:
        p = p.to(p_dtype).to(dtype)
    out = torch.einsum("thm,tmd->thd", p, v[g, 0])
    out.backward(dout.to(dtype))
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad,
                dsink=None if sk is None else sk.grad,
                lse=torch.logsumexp(full, dim=-1).detach(),
                max_logits=s.detach().amax(dim=(0, 2)))


def _make(Bk, hq, max_topk, B=1, tq=5, D=128, counts=(), lists=None, fp8=False,
          seed=0):
    g = torch.Generator().manual_seed(seed)
    cast = (lambda t: (t * 0.5).to(FP8)) if fp8 else (lambda t: t.bfloat16())
    q = cast(torch.randn(tq, hq, D, generator=g)).cuda()
    dout = torch.randn(tq, hq, D, generator=g).bfloat16().cuda()
    k, v = [cast(torch.randn(S_KV, 1, D, generator=g)).cuda() for _ in "ab"]
    nl, nb = -(-tq // B), -(-S_KV // Bk)
    idx = torch.full((nl, 1, max_topk), -1, dtype=torch.int32)
    for i in range(nl):
        if lists is not None:
            ids = lists[i % len(lists)]
        else:
            ids = (torch.randperm(nb - 2, generator=g) + 1).tolist()
            ids = (ids[:1] + [nb - 1] + ids[1:])[:counts[i % len(counts)]]
        idx[i, 0, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return q, k, v, dout, idx.cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_index_k_block(name):
    from magi_attention.functional import flex_flash_attn_func

    c = dict(CASES[name])
    softcap, sink_spec = c.pop("softcap", 0.0), c.pop("sink", None)
    Bk, B, hq, fp8 = c["Bk"], c.get("B", 1), c["hq"], c.get("fp8", False)
    q, k, v, dout, idx = _make(**c, seed=len(name) + hq)
    tq, sink = q.shape[0], None
    if sink_spec:
        g = torch.Generator().manual_seed(1000)
        sink = (torch.randn(sink_spec[1], hq, generator=g) * 2 + 2).cuda()

    qg, kg, vg = [t.clone().requires_grad_(True) for t in (q, k, v)]
    sg = None if sink is None else sink.clone().requires_grad_(True)
    out, meta = flex_flash_attn_func(
        qg, kg, vg, index_attn_indices=idx, q_block_size=B, k_block_size=Bk,
        softcap=softcap, sink=sg, return_max_logits=sink is not None,
    )
    out.backward(dout)
    got = dict(out=out.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad,
               dsink=None if sg is None else sg.grad)

    # expansion to per-token row ids, holes left in place
    ids = idx[:, 0].long()
    rows = ids[:, :, None] * Bk + torch.arange(Bk, device="cuda")
    rows[(ids[:, :, None] < 0) | (rows >= S_KV)] = -1
    per_tok = rows.reshape(len(ids), -1).repeat_interleave(B, 0)[:tq]
    ref = [_oracle(q, k, v, per_tok, dout, q.shape[-1] ** -0.5, softcap, dt,
                   sink) for dt in (torch.float64, torch.bfloat16)]
    if fp8:
        ref[1]["out"] = _oracle(q, k, v, per_tok, dout, q.shape[-1] ** -0.5,
                                softcap, torch.float32, sink, FP8)["out"]
    for what, t in ((w, t.float()) for w, t in got.items() if t is not None):
        assert t.shape == ref[0][what].shape and torch.isfinite(t).all(), what
        budget = dict(ratio=4.5, floor=9e-2) if fp8 and what != "out" else {}
        assert_close_to_ref(t, ref[0][what], ref[1][what], f"{name}:{what}",
                            **budget)
    fin = torch.isfinite(ref[0]["lse"])
    assert torch.equal(torch.isfinite(meta.lse), fin)
    torch.testing.assert_close(meta.lse[fin], ref[0]["lse"][fin].float(),
                               atol=3e-2, rtol=3e-3)
    if sink is not None:
        torch.testing.assert_close(meta.max_logits, ref[0]["max_logits"].float(),
                                   atol=2e-2, rtol=2e-2)

    # K rows in no listed block get no atomic; rows of an all -1 list: out 0,
    # dq 0, lse -inf without a sink (with one, lse_sink: the oracle above)
    listed = torch.zeros(S_KV, dtype=torch.bool, device="cuda")
    listed[per_tok[per_tok >= 0]] = True
    assert (got["dk"].float()[~listed] == 0).all()
    assert (got["dv"].float()[~listed] == 0).all()
    dead = (per_tok < 0).all(dim=1)
    assert dead.any() == (0 in c.get("counts", ()))
    assert (got["out"][dead] == 0).all() and (got["dq"].float()[dead] == 0).all()
    if sink is None:
        assert (meta.lse[dead] == float("-inf")).all()


def test_index_k_block_refusals():
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, _, idx = _make(Bk=16, hq=8, max_topk=12, counts=[12])
    call = lambda *a, **kw: flex_flash_attn_func(*a, index_attn_indices=idx, **kw)
    with pytest.raises(AssertionError, match="power of two"):
        call(q, k, v, k_block_size=3)
    with pytest.raises(AssertionError, match="multiple of 64"):
        flex_flash_attn_func(q, k, v, index_attn_indices=idx[..., :3],
                             k_block_size=16)
    with pytest.raises(AssertionError, match="fp8"):
        q8, k8, v8 = [t.to(FP8) for t in (q, k, v)]
        call(q8, k8, v8, q_block_size=5, k_block_size=16)
    with pytest.raises(AssertionError, match="deterministic"):
        call(q.clone().requires_grad_(True), k, v, k_block_size=16,
             deterministic=True)
