"""GPU parity tests for q_block_size > 1 on the index (token-gather) path:
flex_flash_attn_func(q, k, v, index_attn_indices=[ceil(total_q / B) lists],
q_block_size=B) under autograd - the BLOCK kernels of csrc/ffa_index.hip and
csrc/ffa_index_bwd.hip.

Oracle: the gather-based PyTorch attention of tests/test_ffa_index_sink_gpu.py
(copied, not imported) over the lists expanded to one per token with
repeat_interleave(B, 0)[:total_q], in fp64 (ref_hi) and in bf16 (ref_lo).
Budgets are the index tests': assert_close_to_ref at its defaults for out, dq,
dk, dv, dsink; lse atol=3e-2, rtol=3e-3 and max_logits atol=rtol=2e-2 against
fp64. Every case fails on the parent commit at its q_block_size assertion.
"""
import pytest
import torch

from tests.util import assert_close_to_ref

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

S_KV, UNLISTED = 256, 16  # the last UNLISTED K rows are in no list

# (B, hq, total_q) -> what the packing reaches. (4, 8, 18): one exact wave,
# partial last block of 16 rows. (3, 24, 20): 72 rows, a token's heads straddle
# a wave boundary, partial last wave, empty fourth wave. (16, 16, 40): 256
# rows, two workgroups per block at 4 waves, the last block leaves its second
# one without a row. (64, 1, 80): single head, 2 waves. counts: valid ids per
# block, cycled (48 of 64: half-valid second subtile; 0: all -1; 64: full)
CASES = {
    "b4h8": dict(B=4, hq=8, tq=18, counts=[48, 0, 48]),
    "b3h24": dict(B=3, hq=24, tq=20),
    "b16h16": dict(B=16, hq=16, tq=40, counts=[48, 0, 48]),
    "b64h1": dict(B=64, hq=1, tq=80, counts=[64, 48]),
    "multi": dict(B=4, hq=8, tq=18, max_topk=256,
                  counts=[17, 192, 240, 64, 100]),
    "d64": dict(B=3, hq=24, tq=20, D=64),
    "d96": dict(B=3, hq=24, tq=20, D=96),
    "softcap": dict(B=4, hq=8, tq=18, softcap=2.0),
    "sink_sh": dict(B=3, hq=24, tq=20, counts=[48, 0], sink=("sh", 2)),
    "sink_ssh": dict(B=16, hq=16, tq=40, counts=[48, 0, 48], sink=("ssh", 3)),
}


def _oracle(q, k, v, idx2d, dout, scale, softcap, dtype, sink, layout):
    q, k, v = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    valid = idx2d >= 0
    g = idx2d.clamp_min(0).long()
    s = torch.einsum("thd,tmd->thm", q, k[g, 0]) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    full, sk = s, None
    if sink is not None:
        sk = sink.detach().to(dtype).requires_grad_(True)
        cols = (sk.t().unsqueeze(0).expand(s.shape[0], -1, -1)
                if layout == "sh" else sk.permute(0, 2, 1))
        full = torch.cat([s, cols], dim=-1)
    p = torch.softmax(full, dim=-1).nan_to_num(0.0)[..., :s.shape[-1]]
    out = torch.einsum("thm,tmd->thd", p, v[g, 0])
    out.backward(dout.to(dtype))
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad,
                dsink=None if sk is None else sk.grad,
                lse=torch.logsumexp(full, dim=-1).detach(),
                max_logits=s.detach().amax(dim=(0, 2)))


def _make(B, hq, tq, D=128, max_topk=64, counts=(48,), seed=0):
    g = torch.Generator().manual_seed(seed)
    q, dout = [torch.randn(tq, hq, D, generator=g).bfloat16().cuda() for _ in "ab"]
    k, v = [torch.randn(S_KV, 1, D, generator=g).bfloat16().cuda() for _ in "ab"]
    nb = -(-tq // B)
    idx = torch.full((nb, 1, max_topk), -1, dtype=torch.int32)
    for b in range(nb):
        c = counts[b % len(counts)]
        idx[b, 0, :c] = torch.randperm(S_KV - UNLISTED, generator=g)[:c].int()
    return q, k, v, dout, idx.cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_index_q_block(name):
    from magi_attention.functional import flex_flash_attn_func

    c = dict(CASES[name])
    softcap, sink_spec = c.pop("softcap", 0.0), c.pop("sink", None)
    B, hq, tq = c["B"], c["hq"], c["tq"]
    q, k, v, dout, idx = _make(**c, seed=len(name) + hq)
    sink = layout = None
    if sink_spec:
        layout, ns = sink_spec
        shape = (ns, hq) if layout == "sh" else (tq, ns, hq)
        g = torch.Generator().manual_seed(1000 + ns)
        sink = (torch.randn(*shape, generator=g) * 2 + 2).cuda()

    qg, kg, vg = [t.clone().requires_grad_(True) for t in (q, k, v)]
    sg = None if sink is None else sink.clone().requires_grad_(True)
    out, meta = flex_flash_attn_func(
        qg, kg, vg, index_attn_indices=idx, q_block_size=B, softcap=softcap,
        sink=sg, sink_layout=layout or "sh", return_max_logits=sink is not None,
    )
    out.backward(dout)
    got = dict(out=out.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad,
               dsink=None if sg is None else sg.grad)

    idx2d = idx[:, 0]
    per_tok = idx2d.repeat_interleave(B, 0)[:tq]
    ref = [_oracle(q, k, v, per_tok, dout, q.shape[-1] ** -0.5, softcap, dt,
                   sink, layout) for dt in (torch.float64, torch.bfloat16)]
    for what, t in ((w, t) for w, t in got.items() if t is not None):
        assert t.shape == ref[0][what].shape and torch.isfinite(t).all(), what
        assert_close_to_ref(t, ref[0][what], ref[1][what], f"{name}:{what}")
    fin = torch.isfinite(ref[0]["lse"])
    assert torch.equal(torch.isfinite(meta.lse), fin)
    torch.testing.assert_close(meta.lse[fin], ref[0]["lse"][fin].float(),
                               atol=3e-2, rtol=3e-3)
    if sink is not None:
        torch.testing.assert_close(meta.max_logits, ref[0]["max_logits"].float(),
                                   atol=2e-2, rtol=2e-2)

    # K rows in no list get no atomic; rows of an all -1 block: out 0, dq 0,
    # lse -inf without a sink (with one, lse_sink: held by the oracle above)
    listed = torch.zeros(S_KV, dtype=torch.bool, device="cuda")
    listed[idx2d[idx2d >= 0].long()] = True
    assert (got["dk"][~listed] == 0).all() and (got["dv"][~listed] == 0).all()
    dead = (per_tok < 0).all(dim=1)
    assert dead.any() == (0 in c.get("counts", ()))
    assert (got["out"][dead] == 0).all() and (got["dq"][dead] == 0).all()
    if sink is None:
        assert (meta.lse[dead] == float("-inf")).all()


def test_index_q_block_refusals():
    from magi_attention.functional import flex_flash_attn_func

    q, k, v, _, idx = _make(B=4, hq=8, tq=18)
    with pytest.raises(AssertionError, match="ceil"):  # 5 lists wanted
        flex_flash_attn_func(q, k, v, index_attn_indices=idx[:4], q_block_size=4)
    with pytest.raises(AssertionError, match="fp8"):
        q8, k8, v8 = [t.to(torch.float8_e4m3fn) for t in (q, k, v)]
        flex_flash_attn_func(q8, k8, v8, index_attn_indices=idx, q_block_size=4)
