"""Edge-shape parity tests for the memory-bound kernels of csrc/range_ops.hip:
the range copy / sum / lse-merge kernels behind group-cast and group-reduce,
the fused correct_out_lse, the sink fold and dsink.

Every reference is plain torch on the CPU: a bit-exact index copy for the copy
kernels, fp64 arithmetic for everything else. Bound conventions:

* copies: bitwise (compared through a uint8 view);
* fp32 sum: per element K * 2^-23 * (|dst0| + sum|addend|), K = addends + 1
  (the textbook bound for K fp32 additions in any order);
* one lse merge / sink fold in fp32: atol = rtol = 1e-5 per element; four
  sequenced merges: 4e-5;
* bf16 sink fold: one bf16 ulp (2^-8 relative) plus 2^-134 absolute;
* dsink "sh": 1e-5 * sum_rows|term| per element; "ssh": atol = rtol = 1e-5.

"The sentinel check": every in-place destination is pre-filled with a
recognisable pattern (byte 0xA5 for copies, a fixed finite float for reduces),
is longer than the last targeted row, and every row the table does not target
must be bit-identical afterwards.

Not tested on purpose: ONE lse-reduce call whose ranges overlap in the output.
That is a read-modify-write race by design (only the fp32 sum is atomic);
callers such as group_reduce_out_lse sequence one call per partial, and that
sequencing is what test_lse_reduce_sequenced_partials pins."""
import itertools

import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

from magi_attention import _ffa_lib  # noqa: E402
from magi_attention.comm.primitive import _rows_copy  # noqa: E402
from magi_attention.common.range_op import (  # noqa: E402
    correct_out_lse,
    range_gather,
    range_reduce,
    range_scatter,
)
from magi_attention.meta.containers import RowChunkMap  # noqa: E402

INF = float("inf")
BF16, FP32, FP8, U8 = (torch.bfloat16, torch.float32, torch.float8_e4m3fn,
                       torch.uint8)
SENT_BYTE = 0xA5     # copy destinations
SENT_F = -1234.5     # reduce destinations (out)
SENT_LSE = 7.25      # reduce destinations (lse)
BIG = 1e30           # finite payload of a side whose lse is -inf

# One table with every awkward range at once: a 3000-row range next to five
# tiny ones (1 row, 3 rows, EMPTY in the middle, 4 rows, 2 rows), out_starts
# non-increasing. total 3010 rows / 6 ranges -> grid.x = 502, so the long range
# grid-strides six times (and, at 4 row-heads per block, the lse kernel loops).
SKEW_RANGES = [(10, 3010), (3020, 3021), (3030, 3033), (3040, 3040), (5, 9),
               (3050, 3052)]
SKEW_STARTS = [200, 150, 140, 140, 100, 50]
SKEW_TOTAL = 3010
SKEW_T_IN = 3060
SKEW_T_OUT = 3216  # last targeted row is 3199

# Three ranges onto the same destination rows: two identical, one shifted by
# half, so an element receives 2 (rows 10..309), 3 (310..609) or 1 (610..909)
# addends.
OVER_RANGES = [(0, 600), (0, 600), (700, 1300)]
OVER_STARTS = [10, 10, 310]
OVER_TOTAL = 1800
OVER_T_IN = 1300
OVER_T_OUT = 926


# ----------------------------------------------------------------- helpers
def _table(ranges, starts):
    r = torch.tensor(ranges, dtype=torch.int32, device="cuda").reshape(-1, 2)
    s = torch.tensor(starts, dtype=torch.int32, device="cuda")
    return r, s


def _pairs(ranges, starts):
    """(source row, destination row) of every row a table moves, table order."""
    src = [torch.arange(a, b) for a, b in ranges]
    dst = [torch.arange(o, o + b - a) for (a, b), o in zip(ranges, starts)]
    return torch.cat(src), torch.cat(dst)


def _packed_starts(ranges):
    out, acc = [], 0
    for a, b in ranges:
        out.append(acc)
        acc += b - a
    return out


def _row_bytes(dtype, tail):
    n = torch.empty((), dtype=dtype).element_size()
    for s in tail:
        n *= s
    return n


def _from_bytes(b, dtype, tail):
    """[T, row_bytes] uint8 -> [T, *tail] of dtype, same bytes."""
    return b.view(dtype).reshape(b.shape[0], *tail)


def _bytes(t):
    """[T, *tail] tensor -> CPU [T, row_bytes] uint8, same bytes."""
    t = t.detach().cpu().contiguous()
    return t.view(U8).reshape(t.shape[0], _row_bytes(t.dtype, t.shape[1:]))


def _random_bytes(rows, row_bytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (rows, row_bytes), dtype=U8, generator=g)


def _sentinel_bytes(rows, row_bytes):
    return torch.full((rows, row_bytes), SENT_BYTE, dtype=U8)


def _assert_bits_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got.contiguous().flatten().view(U8),
                       want.contiguous().flatten().view(U8))


# ------------------------------------------------------------------ 1. copy
# (id, dtype, row tail): the id leads with the range_rows_kernel instantiation
# that launch_range picks for that row byte count.
COPY_LAYOUTS = [
    ("float4-bf16_4x32-256B", BF16, (4, 32)),
    ("float4-bf16_32x160-10240B", BF16, (32, 160)),  # 640 vectors: 2.5 passes
    ("float4-fp8_2x64-128B", FP8, (2, 64)),
    ("float-fp32_3-12B", FP32, (3,)),
    ("float-fp32_2-8B", FP32, (2,)),
    ("float-bf16_1x6-12B", BF16, (1, 6)),
    ("float-fp32_1d-4B", FP32, ()),
    ("char-bf16_1x1-2B", BF16, (1, 1)),
    ("char-bf16_3x5-30B", BF16, (3, 5)),
    ("char-fp8_1x7-7B", FP8, (1, 7)),
]
COPY_IDS = [c[0] for c in COPY_LAYOUTS]
ONE_PER_INST = [COPY_LAYOUTS[1], COPY_LAYOUTS[3], COPY_LAYOUTS[8]]
ONE_PER_INST_IDS = [c[0] for c in ONE_PER_INST]


@pytest.mark.parametrize("api", ["range_gather", "rows_copy"])
@pytest.mark.parametrize("name,dtype,tail", COPY_LAYOUTS, ids=COPY_IDS)
def test_copy_skewed_table(name, dtype, tail, api):
    rb = _row_bytes(dtype, tail)
    src_b = _random_bytes(SKEW_T_IN, rb, seed=11)
    x = _from_bytes(src_b, dtype, tail).cuda()
    dst = _from_bytes(_sentinel_bytes(SKEW_T_OUT, rb), dtype, tail).cuda()
    if api == "range_gather":
        r, s = _table(SKEW_RANGES, SKEW_STARTS)
        ret = range_gather(x, r, s, SKEW_TOTAL, output=dst)
        assert ret is dst
    else:
        cmap = RowChunkMap(in_ranges=list(SKEW_RANGES),
                           out_starts=list(SKEW_STARTS), total_rows=SKEW_TOTAL)
        _rows_copy(x, dst, cmap, reduce="copy")
    torch.cuda.synchronize()

    si, di = _pairs(SKEW_RANGES, SKEW_STARTS)
    want = _sentinel_bytes(SKEW_T_OUT, rb)
    want[di] = src_b[si]
    got = _bytes(dst)
    untouched = torch.ones(SKEW_T_OUT, dtype=torch.bool)
    untouched[di] = False
    assert untouched[-16:].all()
    assert (got[untouched] == SENT_BYTE).all(), "rows outside the table changed"
    assert torch.equal(got, want)


@pytest.mark.parametrize("name,dtype,tail", ONE_PER_INST, ids=ONE_PER_INST_IDS)
def test_gather_default_starts(name, dtype, tail):
    """out_starts=None / total_size=None: dense packing in table order."""
    rb = _row_bytes(dtype, tail)
    src_b = _random_bytes(SKEW_T_IN, rb, seed=12)
    x = _from_bytes(src_b, dtype, tail).cuda()
    r, _ = _table(SKEW_RANGES, SKEW_STARTS)
    out = range_gather(x, r)
    torch.cuda.synchronize()
    si, _ = _pairs(SKEW_RANGES, SKEW_STARTS)
    assert out.shape == (SKEW_TOTAL, *tail) and out.dtype == dtype
    assert torch.equal(_bytes(out), src_b[si])


def test_gather_explicit_starts_default_size():
    """out_starts given, total_size=None: the starts are honoured and the
    output reaches the furthest placed row."""
    rb = _row_bytes(FP32, (3,))
    src_b = _random_bytes(SKEW_T_IN, rb, seed=13)
    x = _from_bytes(src_b, FP32, (3,)).cuda()
    r, s = _table(SKEW_RANGES, SKEW_STARTS)
    out = range_gather(x, r, s)
    torch.cuda.synchronize()
    si, di = _pairs(SKEW_RANGES, SKEW_STARTS)
    assert out.shape == (3200, 3)
    assert torch.equal(_bytes(out)[di], src_b[si])


def test_gather_noncontiguous_input():
    g = torch.Generator().manual_seed(14)
    base = torch.randn(4, 90, 32, generator=g).bfloat16().cuda()
    x = base.transpose(0, 1)  # [90, 4, 32], strided
    assert not x.is_contiguous()
    ranges, starts = [(70, 90), (3, 4), (20, 20), (30, 41)], [12, 11, 11, 0]
    r, s = _table(ranges, starts)
    dst = _from_bytes(_sentinel_bytes(40, 256), BF16, (4, 32)).cuda()
    range_gather(x, r, s, 32, output=dst)
    torch.cuda.synchronize()
    si, di = _pairs(ranges, starts)
    want = _sentinel_bytes(40, 256)
    want[di] = _bytes(x)[si]
    assert torch.equal(_bytes(dst), want)


def test_zero_ranges_touch_nothing():
    r = torch.empty((0, 2), dtype=torch.int32, device="cuda")
    s = torch.empty((0,), dtype=torch.int32, device="cuda")
    x = torch.randn(8, 4).cuda()
    out = range_gather(x, r)
    assert out.shape == (0, 4)

    sent = torch.full((8, 4), SENT_F)
    lse_sent = torch.full((8, 1), SENT_LSE)
    dst = sent.cuda()
    range_gather(x, r, s, 0, output=dst)
    range_scatter(x, dst, r, s)
    range_reduce(x, dst, r, s, op="sum")
    _rows_copy(x, dst, RowChunkMap([], [], 0), reduce="copy")
    _rows_copy(x, dst, RowChunkMap([], [], 0), reduce="sum")
    dst3, dl = dst.view(8, 1, 4), lse_sent.cuda()
    range_reduce(x.view(8, 1, 4), dst3, r, s, op="lse",
                 in_lse=torch.zeros(8, 1).cuda(), out_lse=dl)
    torch.cuda.synchronize()
    _assert_bits_equal(dst.cpu(), sent)
    _assert_bits_equal(dl.cpu(), lse_sent)


@pytest.mark.parametrize("name,dtype,tail", ONE_PER_INST, ids=ONE_PER_INST_IDS)
def test_scatter_inverts_gather(name, dtype, tail):
    """scatter(gather(x)) restores exactly the ranged rows of a sentinel
    buffer and nothing else."""
    rb = _row_bytes(dtype, tail)
    src_b = _random_bytes(SKEW_T_IN, rb, seed=15)
    x = _from_bytes(src_b, dtype, tail).cuda()
    r, _ = _table(SKEW_RANGES, SKEW_STARTS)
    packed = range_gather(x, r)
    in_starts = torch.tensor(_packed_starts(SKEW_RANGES), dtype=torch.int32,
                             device="cuda")
    buf = _from_bytes(_sentinel_bytes(SKEW_T_IN + 16, rb), dtype, tail).cuda()
    ret = range_scatter(packed, buf, r, in_starts)
    torch.cuda.synchronize()
    assert ret is buf
    si, _ = _pairs(SKEW_RANGES, SKEW_STARTS)
    want = _sentinel_bytes(SKEW_T_IN + 16, rb)
    want[si] = src_b[si]
    assert torch.equal(_bytes(buf), want)


def test_scatter_hand_written():
    x = torch.arange(12, dtype=FP32).reshape(6, 2).cuda()
    sent = _from_bytes(_sentinel_bytes(8, 8), FP32, (2,))
    buf = sent.clone().cuda()
    # output rows [5,7) <- input rows 0,1 ; output row 1 <- input row 4
    ranges = torch.tensor([[5, 7], [1, 2]], dtype=torch.int32, device="cuda")
    in_starts = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    range_scatter(x, buf, ranges, in_starts)
    torch.cuda.synchronize()
    want = sent.clone()
    want[5] = torch.tensor([0.0, 1.0])
    want[6] = torch.tensor([2.0, 3.0])
    want[1] = torch.tensor([8.0, 9.0])
    _assert_bits_equal(buf.cpu(), want)


# ------------------------------------------------------------ 2. sum-reduce
SUM_TABLES = {
    "overlap": (OVER_RANGES, OVER_STARTS, OVER_TOTAL, OVER_T_IN, OVER_T_OUT),
    "skewed": (SKEW_RANGES, SKEW_STARTS, SKEW_TOTAL, SKEW_T_IN, SKEW_T_OUT),
}
SUM_TAILS = {"16B": (1, 4), "10240B": (16, 160)}


def _sum_case(table, tail, seed):
    """src, dst0 (sentinel everywhere, random non-zero on targeted rows), the
    fp64 expected sum, the per-element bound and the untouched-row mask."""
    ranges, starts, _, t_in, t_out = SUM_TABLES[table]
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(t_in, *tail, generator=g)
    dst0 = torch.full((t_out, *tail), SENT_F)
    si, di = _pairs(ranges, starts)
    targeted = torch.zeros(t_out, dtype=torch.bool)
    targeted[di] = True
    dst0[targeted] = torch.randn(int(targeted.sum()), *tail, generator=g) + 2.0
    want = dst0.double().index_add(0, di, src.double()[si])
    mag = dst0.double().abs().index_add(0, di, src.double().abs()[si])
    n_add = torch.zeros(t_out, dtype=torch.float64).index_add(
        0, di, torch.ones(di.numel(), dtype=torch.float64))
    bound = (n_add + 1).reshape(-1, *([1] * len(tail))) * 2.0 ** -23 * mag
    return src, dst0, want, bound, ~targeted


def _check_sum(got, dst0, want, bound, untouched):
    assert untouched[-16:].all()
    _assert_bits_equal(got[untouched], dst0[untouched])
    err = (got.double() - want).abs()
    worst = (err / bound).max().item()
    print(f"sum: max err/bound = {worst:.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("api", ["range_reduce", "rows_copy"])
@pytest.mark.parametrize("width", list(SUM_TAILS))
@pytest.mark.parametrize("table", list(SUM_TABLES))
def test_sum_reduce(table, width, api, monkeypatch):
    monkeypatch.delenv("MAGI_ATTENTION_DETERMINISTIC_MODE", raising=False)
    ranges, starts, total, _, _ = SUM_TABLES[table]
    src, dst0, want, bound, untouched = _sum_case(table, SUM_TAILS[width], 21)
    dst = dst0.cuda()
    if api == "range_reduce":
        r, s = _table(ranges, starts)
        ret = range_reduce(src.cuda(), dst, r, s, op="sum", total_rows=total)
        assert ret is dst
    else:
        _rows_copy(src.cuda(), dst, RowChunkMap(list(ranges), list(starts),
                                                total), reduce="sum")
    torch.cuda.synchronize()
    _check_sum(dst.cpu(), dst0, want, bound, untouched)


@pytest.mark.parametrize("width", list(SUM_TAILS))
def test_sum_reduce_deterministic_mode(width, monkeypatch):
    """Deterministic mode sequences overlapping ranges one call at a time:
    two runs are bit-identical and meet the same bound."""
    monkeypatch.setenv("MAGI_ATTENTION_DETERMINISTIC_MODE", "1")
    ranges, starts, total, _, _ = SUM_TABLES["overlap"]
    src, dst0, want, bound, untouched = _sum_case("overlap", SUM_TAILS[width], 22)
    runs = []
    for _ in range(2):
        dst = dst0.cuda()
        _rows_copy(src.cuda(), dst, RowChunkMap(list(ranges), list(starts),
                                                total), reduce="sum")
        torch.cuda.synchronize()
        runs.append(dst.cpu())
    _assert_bits_equal(runs[0], runs[1])
    _check_sum(runs[0], dst0, want, bound, untouched)


def test_sum_reduce_rejects_unaligned_rows():
    """12-byte rows cannot take the float4 atomic path: launch_range returns
    -2 before any launch, the wrapper raises, the destination is untouched."""
    src = torch.randn(8, 3).cuda()
    dst0 = torch.full((8, 3), SENT_F)
    dst = dst0.cuda()
    r, s = _table([(0, 4)], [2])
    with pytest.raises(RuntimeError, match="-2"):
        range_reduce(src, dst, r, s, op="sum")
    torch.cuda.synchronize()
    _assert_bits_equal(dst.cpu(), dst0)


# --------------------------------------------------------------- 3. lse merge
MERGE_DH = list(itertools.product([32, 64, 96, 128, 192], [1, 3]))
MERGE_IDS = [f"d{d}-h{h}" for d, h in MERGE_DH]


def _merge_operands(n, h, d, seed):
    """n row pairs (o_old, l_old, o_new, l_new), fp32. Row-heads cycle through
    eight kinds: 0 both finite, 1 new -inf, 2 old -inf, 3 both -inf, 4 equal
    lse, 5 new = old + 100, 6 new = old - 100 (the smaller weight underflows),
    7 magnitude near +-80. A side whose lse is -inf carries a BIG finite
    payload, so a kernel that forgets its zero weight is far off."""
    assert n * h >= 8
    g = torch.Generator().manual_seed(seed)
    o_old = torch.randn(n, h, d, generator=g)
    o_new = torch.randn(n, h, d, generator=g)
    l_old = torch.randn(n, h, generator=g) * 3
    l_new = torch.randn(n, h, generator=g) * 3
    kind = torch.arange(n * h).reshape(n, h) % 8
    k7 = kind == 7
    sign = torch.where(torch.randn(n, h, generator=g) > 0, 80.0, -80.0)
    l_old[k7] = (sign + 0.5 * torch.randn(n, h, generator=g))[k7]
    l_new[k7] = (l_old + torch.randn(n, h, generator=g))[k7]
    l_new[kind == 4] = l_old[kind == 4]
    l_new[kind == 5] = l_old[kind == 5] + 100
    l_new[kind == 6] = l_old[kind == 6] - 100
    l_new[(kind == 1) | (kind == 3)] = -INF
    l_old[(kind == 2) | (kind == 3)] = -INF
    o_new[l_new == -INF] = BIG
    o_old[l_old == -INF] = BIG
    return o_old, l_old, o_new, l_new


def _merge_ref(outs, lses):
    """fp64 online-softmax merge of any number of (out, lse) operands. The
    -inf sides are cut out with torch.where, so the expected value does not
    depend on the payload of an absent side."""
    o = torch.stack([x.double() for x in outs])    # [k, n, h, d]
    l = torch.stack([x.double() for x in lses])    # [k, n, h]
    m = l.amax(0)
    dead = m == -INF
    ms = torch.where(dead, torch.zeros_like(m), m)
    lse = torch.where(dead, torch.full_like(m, -INF),
                      ms + torch.log(torch.exp(l - ms).sum(0)))
    ls = torch.where(dead, torch.zeros_like(lse), lse)
    w = torch.where(l == -INF, torch.zeros_like(l), torch.exp(l - ls))
    terms = torch.where((l == -INF).unsqueeze(-1), torch.zeros_like(o),
                        w.unsqueeze(-1) * o)
    return terms.sum(0), lse


def _check_merge(got_o, got_l, ref_o, ref_l, tol=1e-5):
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(got_l), fin)
    assert (got_l[~fin] == -INF).all()
    assert (got_o[~fin] == 0).all(), "both-(-inf) rows must give out == 0"
    assert torch.isfinite(got_o).all()
    print(f"merge: max |d_out| {(got_o.double() - ref_o).abs().max():.3e} "
          f"max |d_lse| {(got_l[fin].double() - ref_l[fin]).abs().max():.3e}")
    torch.testing.assert_close(got_l[fin].double(), ref_l[fin], atol=tol,
                               rtol=tol)
    torch.testing.assert_close(got_o.double(), ref_o, atol=tol, rtol=tol)


@pytest.mark.parametrize("d,h", MERGE_DH, ids=MERGE_IDS)
def test_lse_reduce_skewed_table(d, h):
    """One call, disjoint-output ranges (empty one included) over the skewed
    table: 3000*h row-heads on 502 blocks x 4 waves enters the rh loop."""
    si, di = _pairs(SKEW_RANGES, SKEW_STARTS)
    o_old, l_old, o_new, l_new = _merge_operands(si.numel(), h, d, seed=31)
    src_o = torch.full((SKEW_T_IN, h, d), 3.0)
    src_l = torch.full((SKEW_T_IN, h), 0.5)
    src_o[si], src_l[si] = o_new, l_new
    dst_o0 = torch.full((SKEW_T_OUT, h, d), SENT_F)
    dst_l0 = torch.full((SKEW_T_OUT, h), SENT_LSE)
    dst_o0[di], dst_l0[di] = o_old, l_old

    do, dl = dst_o0.cuda(), dst_l0.cuda()
    r, s = _table(SKEW_RANGES, SKEW_STARTS)
    range_reduce(src_o.cuda(), do, r, s, op="lse", in_lse=src_l.cuda(),
                 out_lse=dl)
    torch.cuda.synchronize()
    do, dl = do.cpu(), dl.cpu()

    untouched = torch.ones(SKEW_T_OUT, dtype=torch.bool)
    untouched[di] = False
    assert untouched[-16:].all()
    _assert_bits_equal(do[untouched], dst_o0[untouched])
    _assert_bits_equal(dl[untouched], dst_l0[untouched])
    ref_o, ref_l = _merge_ref([o_old, o_new], [l_old, l_new])
    _check_merge(do[di], dl[di], ref_o, ref_l)


CORRECT_CASES = [(37, h, d) for d, h in MERGE_DH] + [(5000, 4, 32)]


@pytest.mark.parametrize("t,h,d", CORRECT_CASES,
                         ids=[f"t{t}-d{d}-h{h}" for t, h, d in CORRECT_CASES])
def test_correct_out_lse_edges(t, h, d):
    """t=5000, h=4 is 20000 row-heads > 4096 blocks x 4 waves: grid-stride."""
    o1, l1, o2, l2 = _merge_operands(t, h, d, seed=32)
    o1c, l1c = o1.cuda(), l1.cuda()
    ro, rl = correct_out_lse(o1c, l1c, o2.cuda(), l2.cuda())
    torch.cuda.synchronize()
    assert ro is o1c and rl is l1c
    ref_o, ref_l = _merge_ref([o1, o2], [l1, l2])
    _check_merge(o1c.cpu(), l1c.cpu(), ref_o, ref_l)


def test_lse_reduce_sequenced_partials():
    """Four partials merged into the SAME destination rows by four sequenced
    one-range calls (what group_reduce_out_lse does) equal the fp64 merge of
    all five operands, in either call order, within 4 x the one-merge budget."""
    t, h, d, t_dst, start = 50, 3, 96, 60, 5
    g = torch.Generator().manual_seed(33)
    outs = [torch.randn(t, h, d, generator=g) for _ in range(5)]
    lses = [torch.randn(t, h, generator=g) * 3 for _ in range(5)]
    for k in range(5):
        lses[k][0] = -INF                 # row 0: nobody contributes
        if k != 0:
            lses[k][1] = -INF             # row 1: only the destination
        if k != 3:
            lses[k][2] = -INF             # row 2: only partial 3
    lses[0][3] = -INF                     # row 3: empty destination
    lses[2][4, 1] = -INF                  # row 4: one head of one partial
    for k in range(5):
        outs[k][lses[k] == -INF] = BIG
    ref_o, ref_l = _merge_ref(outs, lses)

    r, s = _table([(0, t)], [start])
    for order in ([1, 2, 3, 4], [4, 3, 2, 1]):
        dst_o0 = torch.full((t_dst, h, d), SENT_F)
        dst_l0 = torch.full((t_dst, h), SENT_LSE)
        dst_o0[start:start + t], dst_l0[start:start + t] = outs[0], lses[0]
        do, dl = dst_o0.cuda(), dst_l0.cuda()
        for k in order:
            range_reduce(outs[k].cuda(), do, r, s, op="lse",
                         in_lse=lses[k].cuda(), out_lse=dl)
        torch.cuda.synchronize()
        do, dl = do.cpu(), dl.cpu()
        _check_merge(do[start:start + t], dl[start:start + t], ref_o, ref_l,
                     tol=4e-5)
        untouched = torch.ones(t_dst, dtype=torch.bool)
        untouched[start:start + t] = False
        _assert_bits_equal(do[untouched], dst_o0[untouched])
        _assert_bits_equal(dl[untouched], dst_l0[untouched])


def test_lse_reduce_ignores_payload_of_empty_destination():
    """range_rows_lse_kernel guards `w_prev > 0` so that a destination row
    whose lse is -inf contributes nothing WHATEVER it holds (an accumulator
    need not be zeroed, only its lse set to -inf). No finite payload can show
    a missing guard (0 * 1e30 == 0), so this one case uses +inf; the expected
    value is the new side alone, weight exactly 1."""
    g = torch.Generator().manual_seed(34)
    t, h, d = 9, 3, 96
    src_o = torch.randn(t, h, d, generator=g)
    src_l = torch.randn(t, h, generator=g) * 3
    dst_o = torch.full((t, h, d), INF)
    dst_l = torch.full((t, h), -INF)
    do, dl = dst_o.cuda(), dst_l.cuda()
    r, s = _table([(0, t)], [0])
    range_reduce(src_o.cuda(), do, r, s, op="lse", in_lse=src_l.cuda(),
                 out_lse=dl)
    torch.cuda.synchronize()
    assert torch.isfinite(do.cpu()).all()
    torch.testing.assert_close(do.cpu(), src_o, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(dl.cpu(), src_l, atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------- 4. sink fold
def _sink_ids(dt, lay, s, hq, d, tq):
    name = "fp32" if dt == FP32 else "bf16"
    return f"{name}-{lay}-s{s}-hq{hq}-d{d}-tq{tq}"


SINK_CASES = [
    (dt, lay, s, hq, d, 37)
    for dt, lay, s, hq, d in itertools.product(
        [FP32, BF16], ["sh", "ssh"], [1, 8], [1, 3], [32, 96, 192])
] + [
    # one per instantiation: 18000 row-heads > 4096 blocks x 4 waves
    (dt, lay, 8, 3, 96, 6000)
    for dt, lay in itertools.product([FP32, BF16], ["sh", "ssh"])
]


def _sink_inputs(dt, lay, s_sink, hq, d, tq, seed, all_dead=False):
    """out, lse, sink with every row kind: row % 7 == 3 has lse = -inf,
    == 2 has lse_sink - lse = +100, == 4 has -100; partly -inf sink logits
    when s_sink = 8; a sink-less (all -inf) head -- "sh": head 2 of 3,
    "ssh": rows with row % 7 == 5 (all_dead: every logit)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(tq, hq, d, generator=g).to(dt)
    lse = torch.randn(tq, hq, generator=g) * 3
    rows = torch.arange(tq)
    if lay == "sh":
        sink = torch.randn(s_sink, hq, generator=g) * 2
        if s_sink == 8:
            sink[[1, 3], 0] = -INF
        if hq == 3:
            sink[:, 2] = -INF
        if all_dead:
            sink[:] = -INF
        ls = torch.logsumexp(sink.double(), 0).expand(tq, hq)
    else:
        sink = torch.randn(tq, s_sink, hq, generator=g) * 2
        if s_sink == 8:
            part = sink[rows % 7 == 1]
            part[:, [1, 3], :] = -INF
            sink[rows % 7 == 1] = part
        sink[rows % 7 == 5] = -INF
        if all_dead:
            sink[:] = -INF
        ls = torch.logsumexp(sink.double(), 1)
    r = rows[:, None].expand(tq, hq)
    has_sink = torch.isfinite(ls)
    up, dn = (r % 7 == 2) & has_sink, (r % 7 == 4) & has_sink
    lse[up] = (ls.float() - 100)[up]
    lse[dn] = (ls.float() + 100)[dn]
    lse[r % 7 == 3] = -INF
    return out, lse, sink, ls.clone(), up


def _run_sink_fold(out, lse, sink, lay):
    from magi_attention.functional.flex_flash_attn import (
        _apply_sink_postprocess,
    )

    tq, hq, d = out.shape
    oc, lc = out.cuda(), lse.cuda()
    _apply_sink_postprocess(oc, lc, sink.cuda(), lay, tq, hq, d)
    torch.cuda.synchronize()
    return oc.cpu(), lc.cpu()


def _check_sink_fold(out, lse, ls, up, got_o, got_l):
    lse64, out64 = lse.double(), out.double()
    ref_l = torch.logsumexp(torch.stack([lse64, ls]), 0)
    empty = lse == -INF
    scale = torch.exp(torch.where(empty, torch.zeros_like(lse64), lse64) -
                      torch.where(torch.isfinite(ref_l), ref_l,
                                  torch.zeros_like(ref_l)))
    ref_o = torch.where(empty.unsqueeze(-1), torch.zeros_like(out64),
                        out64 * scale.unsqueeze(-1))

    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(got_l), fin)
    assert (got_l[~fin] == -INF).all()
    torch.testing.assert_close(got_l[fin].double(), ref_l[fin], atol=1e-5,
                               rtol=1e-5)
    err = (got_o.double() - ref_o).abs()
    if out.dtype == FP32:
        bound = 1e-5 + 1e-5 * ref_o.abs()
    else:
        # one rounding from fp32: one bf16 ulp, plus slack for tiny values
        bound = 2.0 ** -8 * ref_o.abs() + 2.0 ** -8 * 2.0 ** -126
    print(f"sink fold: max err/bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()

    # lse = -inf: out exactly 0, lse = lse_sink (checked above through ref_l)
    assert empty.any() and (got_o[empty] == 0).all()
    # no sink on this (row, head): out and lse come back bit-identical
    keep = (ls == -INF) & ~empty
    _assert_bits_equal(got_o[keep], out[keep])
    _assert_bits_equal(got_l[keep], lse[keep])
    # lse_sink - lse = +100: out collapses, lse ~ lse_sink
    if up.any():
        assert (got_o[up].float().abs() < 1e-37).all()
        torch.testing.assert_close(got_l[up].double(), ls[up], atol=1e-5,
                                   rtol=1e-5)
    return keep


@pytest.mark.parametrize("dt,lay,s_sink,hq,d,tq", SINK_CASES,
                         ids=[_sink_ids(*c) for c in SINK_CASES])
def test_sink_fold(dt, lay, s_sink, hq, d, tq):
    out, lse, sink, ls, up = _sink_inputs(dt, lay, s_sink, hq, d, tq, seed=41)
    got_o, got_l = _run_sink_fold(out, lse, sink, lay)
    keep = _check_sink_fold(out, lse, ls, up, got_o, got_l)
    assert up.any()
    if lay == "ssh" or hq == 3:
        assert keep.any()


@pytest.mark.parametrize("lay", ["sh", "ssh"])
@pytest.mark.parametrize("dt", [FP32, BF16], ids=["fp32", "bf16"])
def test_sink_fold_without_any_sink(dt, lay):
    """Every sink logit -inf (hq = 1 too, where the crossed "sh" cases have no
    sink-less head): the fold is the identity on rows with a finite lse."""
    out, lse, sink, ls, up = _sink_inputs(dt, lay, 8, 1, 96, 37, seed=42,
                                          all_dead=True)
    got_o, got_l = _run_sink_fold(out, lse, sink, lay)
    keep = _check_sink_fold(out, lse, ls, up, got_o, got_l)
    assert keep.sum() == (lse != -INF).sum()


# -------------------------------------------------------------------- 5. dsink
PAD_ROWS = 256  # finite poison behind row tq: a read past the end shows up


def _dsink_inputs(tq, hq, s_sink, ssh, seed):
    g = torch.Generator().manual_seed(seed)
    lse = torch.randn(tq + PAD_ROWS, hq, generator=g)
    dps = torch.randn(tq + PAD_ROWS, hq, generator=g)
    lse[tq:], dps[tq:] = 0.0, 1e6
    idx = torch.arange(tq * hq).reshape(tq, hq)
    lse[:tq][idx % 6 == 3] = -INF      # dead rows: dpsum is never written for
    lse[:tq][idx % 6 == 5] = INF       # them in the product -> NaN here
    dead = ~torch.isfinite(lse[:tq])
    dps[:tq][dead] = float("nan")
    shape = (tq, s_sink, hq) if ssh else (s_sink, hq)
    sink = torch.randn(*shape, generator=g) * 2
    return lse, dps, sink, dead


def _run_dsink(lse, dps, sink, tq, hq, s_sink, ssh):
    """The C ABI call of flex_flash_attn's backward: zeroed dsink, then
    magi_ffa_dsink on (sink, lse, dpsum)."""
    lc, dc, sc = lse.cuda(), dps.cuda(), sink.cuda()
    dsink = torch.zeros_like(sc)
    args = _ffa_lib.MagiSinkArgs(
        lse=_ffa_lib.ptr(lc), sink=_ffa_lib.ptr(sc), dsink=_ffa_lib.ptr(dsink),
        dpsum=_ffa_lib.ptr(dc), total_rows=tq, n_heads=hq, d=64,
        s_sink=s_sink, ssh=int(ssh), stream=_ffa_lib.current_stream_ptr(),
    )
    _ffa_lib.check(_ffa_lib.lib().magi_ffa_dsink(args), "magi_ffa_dsink")
    torch.cuda.synchronize()
    return dsink.cpu()


def _dsink_terms(lse, dps, sink, dead, tq, ssh):
    """fp64 -exp(sink - lse) * dpsum per (row, j, head); dead rows cut out."""
    l = lse[:tq].double().unsqueeze(1)                      # [tq, 1, hq]
    p = dps[:tq].double().unsqueeze(1)
    s = sink.double() if ssh else sink.double().unsqueeze(0)
    dd = dead.unsqueeze(1)
    safe_l = torch.where(dd, torch.zeros_like(l), l)
    safe_p = torch.where(dd, torch.zeros_like(p), p)
    terms = -torch.exp(s - safe_l) * safe_p
    return torch.where(dd.expand_as(terms), torch.zeros_like(terms), terms)


@pytest.mark.parametrize("s_sink", [1, 8])
@pytest.mark.parametrize("hq", [1, 3])
@pytest.mark.parametrize("tq", [1, 255, 256, 257, 1000])
def test_dsink_sh(tq, hq, s_sink):
    """tq: one row, a partial block, one exact block, one row of spill,
    several blocks meeting in the atomic."""
    lse, dps, sink, dead = _dsink_inputs(tq, hq, s_sink, False, seed=51)
    got = _run_dsink(lse, dps, sink, tq, hq, s_sink, False)
    terms = _dsink_terms(lse, dps, sink, dead, tq, False)
    want, bound = terms.sum(0), 1e-5 * terms.abs().sum(0)
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max()
    print(f"dsink sh: max err/bound = {ratio:.3f}")
    assert (err <= bound).all()
    if tq >= 255:
        assert dead.any() and torch.isinf(lse[:tq]).any()


@pytest.mark.parametrize("s_sink", [1, 8])
def test_dsink_ssh(s_sink):
    tq, hq = 1000, 3
    lse, dps, sink, dead = _dsink_inputs(tq, hq, s_sink, True, seed=52)
    got = _run_dsink(lse, dps, sink, tq, hq, s_sink, True)
    want = _dsink_terms(lse, dps, sink, dead, tq, True)
    assert torch.isfinite(got).all()
    dd = dead.unsqueeze(1).expand_as(got)
    assert (lse[:tq] == INF).any() and (lse[:tq] == -INF).any()
    assert (got[dd] == 0).all(), "dead rows must give exactly 0"
    torch.testing.assert_close(got.double(), want, atol=1e-5, rtol=1e-5)
