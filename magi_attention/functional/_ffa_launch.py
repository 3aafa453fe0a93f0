# Host-side launch layer of the FFA kernels: the one place under functional/
# that fills a ctypes argument struct of include/magi_ffa.h (bound in
# magi_attention/_ffa_lib.py) and calls the matching magi_ffa_* entry.
# flex_flash_attn.py (single GPU) and dist_attn.py (context parallel) validate,
# allocate and call in here. Launches go to torch's current stream.
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _ffa_lib, env
from .._ffa_lib import check, current_stream_ptr, ptr

_FP8 = torch.float8_e4m3fn
_side_stream: dict = {}


def _get_side_stream(device) -> torch.cuda.Stream:
    key = device.index or 0
    if key not in _side_stream:
        _side_stream[key] = torch.cuda.Stream(device=device)
    return _side_stream[key]


def maybe_contiguous(x: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return x.contiguous() if x is not None and not x.is_contiguous() else x


def new_max_logits(hq: int, device) -> torch.Tensor:
    """f32 [hq] preset to -inf, the state the forward kernels max into"""
    return torch.full((hq,), float("-inf"), dtype=torch.float32, device=device)


def upcast_fp8(*tensors: torch.Tensor) -> list:
    """The fp8 backward policy: there is no fp8 MFMA backward, so the bf16
    kernels run over bf16 copies of the fp8 tensors (others pass untouched),
    standard mixed-precision practice. Gradients come out in bf16 precision;
    the caller casts them to the input dtype at return, as autograd requires."""
    return [t.to(torch.bfloat16) if t.dtype == _FP8 else t for t in tensors]


# ---------------- disjoint groups (deterministic mode) ----------------
def _color_ranges(ranges: list) -> list:
    """Greedy interval partitioning: split slice indices into groups whose
    ranges are pairwise DISJOINT. Deterministic mode runs one kernel launch
    per group, sequentially on the stream, so reduction order is fixed by
    construction — placement-independent, unlike device-side lock ordering
    (the reference's deterministic.h approach assumes dispatch order, which
    CDNA4 does not guarantee)."""
    order = sorted(range(len(ranges)), key=lambda i: (ranges[i][0], ranges[i][1]))
    groups: list = []   # list of (last_end, [indices])
    for i in order:
        s_, e_ = ranges[i]
        for g in groups:
            if g[0] <= s_:
                g[1].append(i)
                g[0] = e_
                break
        else:
            groups.append([e_, [i]])
    return [sorted(g[1]) for g in groups]


def _subset(t: Optional[torch.Tensor], idx: torch.Tensor) -> Optional[torch.Tensor]:
    return None if t is None else t.index_select(0, idx)


def launch_per_group(args, q_ranges, k_ranges, attn_type_map, passes) -> None:
    """For each pass (fn, what, groups, head_splits) and each group of range
    indices in it: subset the three range tables to the group, point args at
    the subsets and launch fn - once per GQA member j if head_splits > 1, with
    (gqa, j) packed into cu_margin, so no two heads add into one dK/dV row."""
    gqa = args.hq // max(args.hk, 1)
    # the subset tables must outlive the async launches of all passes: the
    # ctypes kernels are invisible to torch's stream-aware allocator
    keep = []
    for fn, what, groups, head_splits in passes:
        for g in groups:
            idx = torch.tensor(g, dtype=torch.long, device=q_ranges.device)
            tables = [_subset(t, idx) for t in (q_ranges, k_ranges, attn_type_map)]
            keep.append(tables)
            args.q_ranges, args.k_ranges, args.attn_type_map = map(ptr, tables)
            args.n_ranges = len(g)
            margin = args.cu_margin
            for j in range(head_splits):
                if head_splits > 1:
                    args.cu_margin = (margin & 0xFFFF) | (gqa << 24) | (j << 16)
                check(fn(args), what)
            args.cu_margin = margin


# ---------------- sink ----------------
def _check_sink(sink, sink_layout, tq, hq):
    assert sink_layout in ("sh", "ssh"), f"unsupported sink_layout {sink_layout}"
    sink = sink.contiguous().float()
    if sink_layout == "sh":
        assert sink.dim() == 2 and sink.shape[1] == hq, "sink must be [s_sink, hq]"
        s_sink = sink.shape[0]
    else:
        assert sink.dim() == 3 and sink.shape[0] == tq and sink.shape[2] == hq, (
            "sink must be [total_q, s_sink, hq]"
        )
        s_sink = sink.shape[1]
    assert 1 <= s_sink <= 8, "seqlen_sink must be in [1, 8] (reference kMaxSeqlenSink)"
    return sink, s_sink


def _apply_sink_postprocess(out, lse, sink, sink_layout, tq, hq, d):
    """Fold the sink logits into (out, lse) ONCE, after all slice merges
    (reference flash_fwd_postprocess_kernel.h:39)."""
    sink, s_sink = _check_sink(sink, sink_layout, tq, hq)
    args = _ffa_lib.MagiSinkArgs(
        out=ptr(out), lse=ptr(lse), sink=ptr(sink),
        total_rows=tq, n_heads=hq, d=d, s_sink=s_sink,
        ssh=int(sink_layout == "ssh"),
        out_is_fp32=int(out.dtype == torch.float32),
        stream=current_stream_ptr(),
    )
    check(_ffa_lib.lib().magi_ffa_sink_postprocess(args), "sink_postprocess")


def bwd_dsink(sink_f, s_sink, ssh, lse, dpsum, dsink=None) -> torch.Tensor:
    """Sink gradient (f32, sink_f's shape; accumulated into dsink if given)
    from (sink, lse, dpsum) alone: q/k/v gradients pick the sink up through
    the sink-corrected lse. The kernels never read the head dim: d stays 0."""
    if dsink is None:
        dsink = torch.zeros_like(sink_f)
    tq, hq = lse.shape
    args = _ffa_lib.MagiSinkArgs(
        lse=ptr(lse), sink=ptr(sink_f), dsink=ptr(dsink), dpsum=ptr(dpsum),
        total_rows=tq, n_heads=hq, s_sink=s_sink, ssh=int(ssh),
        stream=current_stream_ptr(),
    )
    check(_ffa_lib.lib().magi_ffa_dsink(args), "magi_ffa_dsink")
    return dsink


# ---------------- dense forward ----------------
def pack_gqa_active(pack_gqa, dtype: torch.dtype, hq: int, hk: int) -> bool:
    """Whether a forward with this flag runs the packed kernel: there is a GQA
    group to pack and a 16-bit kernel to pack it in (no fp8 pack entry).
    Otherwise the flag is accepted and the unpacked launch runs."""
    return bool(pack_gqa) and hq != hk and dtype != _FP8


def sparse_load_active(sparse_load, dtype: torch.dtype, d: int,
                       qk_starts) -> bool:
    """Whether a forward with this flag runs the sparse kernel: there is a
    merged table whose k segments can be packed (qk_starts) and a kernel built
    for it (16-bit, d = 64 or 128). Otherwise the flag is accepted and the
    segment-loop launch runs."""
    return (bool(sparse_load) and qk_starts is not None and dtype != _FP8
            and d in (64, 128))


def swap_ab_active(swap_ab, dtype: torch.dtype, d: int, pack: bool,
                   sparse: bool) -> bool:
    """Whether a forward with this flag runs the split-k kernel: there is one
    built for it (16-bit, d = 64 or 128) and neither pack_gqa nor sparse_load
    is active (pack, sparse: their *_active results). Where one of them is,
    its kernel runs; otherwise the flag is accepted and the default launch
    runs."""
    return (bool(swap_ab) and dtype in (torch.bfloat16, torch.float16)
            and d in (64, 128) and not pack and not sparse)


def fp8_flex_active(dtype: torch.dtype, softcap, qk_starts,
                    disable_fwd_atomic_reduction) -> bool:
    """Whether an fp8 forward goes to magi_ffa_fwd_fp8_flex: it asks for
    something the plain fp8 entry refuses (softcap, a merged table, the direct
    store). Every other fp8 call keeps the plain entry; 16-bit calls never
    come here."""
    return dtype == _FP8 and (softcap != 0 or qk_starts is not None
                              or bool(disable_fwd_atomic_reduction))


def fwd(q, k, v, out, lse, q_ranges, k_ranges, attn_type_map, *, locks,
        max_logits, qk_starts, max_seqlen_q, softmax_scale, softcap,
        disable_fwd_atomic_reduction, sm_margin, deterministic,
        pack_gqa=False, sparse_load=False, swap_ab=False) -> None:
    """Dense forward into (out, lse): an fp8 entry (the flex one where
    fp8_flex_active) or the 16-bit one (bf16 or fp16 by elem_type) by q.dtype;
    deterministic = fixed merge order, one launch per q-disjoint range group;
    pack_gqa = a workgroup owns a KV head and packs the (token, q head) pairs
    of its group into its q tiles (where pack_gqa_active);
    sparse_load = the k segments of a unique q range are packed into full K/V
    tiles (where sparse_load_active; every segment must be a full block);
    swap_ab = the four waves of a workgroup split the k loop of one or two
    32-row q tiles and merge their softmax states (where swap_ab_active)."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    pack = pack_gqa_active(pack_gqa, q.dtype, hq, hk)
    sparse = sparse_load_active(sparse_load, q.dtype, d, qk_starts)
    splitk = swap_ab_active(swap_ab, q.dtype, d, pack, sparse)
    args = (_ffa_lib.MagiFfaFwdSparseArgs if sparse else
            _ffa_lib.MagiFfaFwdPackArgs if pack else
            _ffa_lib.MagiFfaFwdSplitkArgs if splitk else
            _ffa_lib.MagiFfaFwdArgs)(
        q=ptr(q), k=ptr(k), v=ptr(v), out=ptr(out), lse=ptr(lse),
        q_ranges=ptr(q_ranges), k_ranges=ptr(k_ranges),
        attn_type_map=ptr(attn_type_map), locks=ptr(locks),
        max_logits=ptr(max_logits), qk_starts=ptr(qk_starts),
        n_ranges=q_ranges.shape[0], total_q=tq, total_k=tk,
        hq=hq, hk=hk, d=d, max_seqlen_q=max_seqlen_q,
        softmax_scale=softmax_scale, softcap=softcap,
        out_is_fp32=int(out.dtype == torch.float32),
        disable_atomic_reduction=int(disable_fwd_atomic_reduction),
        cu_margin=sm_margin, stream=current_stream_ptr(),
        elem_type=_ffa_lib.elem_type_of(q.dtype),
    )
    lib = _ffa_lib.lib()
    fn = lib.magi_ffa_fwd_fp8 if q.dtype == _FP8 else lib.magi_ffa_fwd
    if fp8_flex_active(q.dtype, softcap, qk_starts,
                       disable_fwd_atomic_reduction):
        assert not (deterministic and qk_starts is not None), (
            "no deterministic mode over merged tables"
        )
        fn = lib.magi_ffa_fwd_fp8_flex
    if pack:
        args.pack_gqa = 1
        fn = lib.magi_ffa_fwd_pack
    if sparse:
        assert not deterministic, "no deterministic mode over merged tables"
        # running sum of the segment lengths, on the device: no host sync.
        # It must outlive the launch, which torch's allocator cannot see:
        # the same stream reuses the block only behind the kernel.
        k_cum = torch.zeros(k_ranges.shape[0] + 1, dtype=torch.int32,
                            device=k_ranges.device)
        k_cum[1:] = (k_ranges[:, 1] - k_ranges[:, 0]).clamp_min(0).cumsum(0)
        args.k_cum = ptr(k_cum)
        args.sparse_load = 1
        fn = lib.magi_ffa_fwd_sparse
    if splitk:  # looked up only here: a library without the entry still serves
        args.swap_ab = 1
        fn = lib.magi_ffa_fwd_splitk
    if deterministic and q_ranges.shape[0] > 1:
        groups = _color_ranges(q_ranges.cpu().tolist())
        launch_per_group(args, q_ranges, k_ranges, attn_type_map,
                         [(fn, "magi_ffa_fwd[det]", groups, 1)])
    else:
        check(fn(args), "magi_ffa_fwd")


# ---------------- dense backward ----------------
def bwd_args(dout, out, dpsum, *, q=None, k=None, v=None, lse=None,
             dq=None, dk=None, dv=None, q_ranges=None, k_ranges=None,
             attn_type_map=None, max_seqlen_k=0, softmax_scale=0.0,
             softcap=0.0, sm_margin=0,
             cat_gqa=False) -> _ffa_lib.MagiFfaBwdSparseArgs:
    """The backward argument struct. (dout, out, dpsum) are all the dpsum
    preprocess reads; the dq/dk/dv passes need every member. The tensors must
    be contiguous and outlive the launches. dout's dtype (bf16 or fp16) is the
    element type of q/k/v too, and of a 16-bit out. The struct is the one of
    magi_ffa_bwd_dq_sparse, its switch off (run_bwd_passes sets it), which
    starts with the one of the magi_ffa_bwd_*_cat entries (it passes as the
    _direct and the plain one
    too); the dtypes of dq and of dk/dv pick each pass's epilogue there: f32 =
    atomic accumulation, the element type = direct store (the caller vouches
    for disjoint ranges). cat_gqa: a dK/dV workgroup owns a KV head and walks
    the q heads of its group, so each dK/dV row of a k range has one owner."""
    tq, hq, d = dout.shape
    tk, hk = (0, 0) if k is None else k.shape[:2]

    def is_16bit(*grads):
        dtypes = {g.dtype for g in grads if g is not None}
        assert len(dtypes) <= 1, f"dk and dv must share a dtype, got {dtypes}"
        assert dtypes <= {torch.float32, dout.dtype}, (
            f"gradient buffers are float32 or {dout.dtype}, got {dtypes}"
        )
        return int(bool(dtypes) and torch.float32 not in dtypes)

    return _ffa_lib.MagiFfaBwdSparseArgs(
        dout=ptr(dout), q=ptr(q), k=ptr(k), v=ptr(v), out=ptr(out),
        lse=ptr(lse), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv), dpsum=ptr(dpsum),
        q_ranges=ptr(q_ranges), k_ranges=ptr(k_ranges),
        attn_type_map=ptr(attn_type_map),
        n_ranges=0 if q_ranges is None else q_ranges.shape[0],
        total_q=tq, total_k=tk, hq=hq, hk=hk, d=d, max_seqlen_k=max_seqlen_k,
        out_is_fp32=int(out.dtype == torch.float32),
        softmax_scale=softmax_scale, softcap=softcap,
        cu_margin=sm_margin, stream=current_stream_ptr(),
        elem_type=_ffa_lib.elem_type_of(dout.dtype),
        dq_is_16bit=is_16bit(dq), dkv_is_16bit=is_16bit(dk, dv),
        cat_gqa=int(bool(cat_gqa)),
    )


def bwd_preprocess(args: _ffa_lib.MagiFfaBwdArgs) -> None:
    """args.dpsum = rowsum(dout * out)"""
    check(_ffa_lib.lib().magi_ffa_bwd_preprocess(args), "magi_ffa_bwd_preprocess")


def bwd_dpsum(dout, out) -> torch.Tensor:
    """dpsum [tq, hq] f32 = rowsum(dout * out), without a full struct"""
    dout, out = maybe_contiguous(dout), maybe_contiguous(out)
    dpsum = torch.empty(dout.shape[:2], dtype=torch.float32, device=dout.device)
    bwd_preprocess(bwd_args(dout, out, dpsum))
    return dpsum


def _bwd_entries(args) -> tuple:
    """The (dq, dkv, dv, dk) entries that take args: the *_cat ones (dq has
    none: its *_direct one) for the struct bwd_args() builds, the *_direct
    ones for a MagiFfaBwdDirectArgs, the plain f32 ones for a bare
    MagiFfaBwdArgs (the stand-alone probes under tests/ fill one by hand)."""
    lib = _ffa_lib.lib()
    sfx = "_direct" if isinstance(args, _ffa_lib.MagiFfaBwdDirectArgs) else ""
    dkv_sfx = "_cat" if isinstance(args, _ffa_lib.MagiFfaBwdCatArgs) else sfx
    return tuple(getattr(lib, f"magi_ffa_bwd_{n}{s}")
                 for n, s in (("dq", sfx), ("dkv", dkv_sfx), ("dv", dkv_sfx),
                              ("dk", dkv_sfx)))


def run_bwd_deterministic(args, q_ranges, k_ranges, attn_type_map) -> None:
    """Deterministic backward: sequential launches over q-disjoint groups
    (dq pass), k-disjoint groups x GQA head sub-launches (dkv pass) — every
    accumulator element receives its additions in a fixed, stream-ordered
    sequence. Under cat_gqa one workgroup walks the heads of a group in a
    fixed order, so a k group is one launch whatever hq / hk is."""
    bwd_dq, bwd_dkv, bwd_dv, bwd_dk = _bwd_entries(args)
    q_groups = _color_ranges(q_ranges.cpu().tolist())
    k_groups = _color_ranges(k_ranges.cpu().tolist())
    hs = 1 if getattr(args, "cat_gqa", 0) else max(args.hq // args.hk, 1)
    if env.is_bwd_split_dkv(args.max_seqlen_k, args.d):
        dkv = [(bwd_dv, "bwd_dv[det]", k_groups, hs),
               (bwd_dk, "bwd_dk[det]", k_groups, hs)]
    else:
        dkv = [(bwd_dkv, "bwd_dkv[det]", k_groups, hs)]
    launch_per_group(args, q_ranges, k_ranges, attn_type_map,
                     [(bwd_dq, "bwd_dq[det]", q_groups, 1)] + dkv)


def bwd_sparse_load_active(sparse_load, dtype: torch.dtype, d: int,
                           dq_tables) -> bool:
    """Whether a backward with this flag runs the sparse dQ kernel: there are
    merged dq tables whose k segments can be packed and a kernel built for
    them (16-bit, d = 64 or 128). Otherwise the flag is accepted and the
    segment-loop dQ pass runs. The dK/dV passes never look at it."""
    return (bool(sparse_load) and dq_tables is not None
            and dtype in (torch.bfloat16, torch.float16) and d in (64, 128))


def run_bwd_passes(args, device, dq_tables=None, dkv_tables=None,
                   sparse_load=False) -> None:
    """Launch the independent backward passes (dq / fused-dkv by default;
    dq / dv / dk with MAGI_BWD_SPLIT_DKV=1) on two streams so their waves
    co-schedule across the chip. dq_tables / dkv_tables override the range
    tables per pass for auto_range_merge: (ranges_outer, ranges_inner,
    attn_type_map, seg_starts) — outer = the pass's OWN loop dim.
    sparse_load (the caller has applied bwd_sparse_load_active): the dq launch
    alone goes through magi_ffa_bwd_dq_sparse, which packs the k segments of a
    unique q range into full K/V tiles; every slice must be a full block."""
    bwd_dq, bwd_dkv, bwd_dv, bwd_dk = _bwd_entries(args)
    main = torch.cuda.current_stream(device)
    k_cum = None
    if sparse_load:
        assert dq_tables is not None, "sparse_load packs a merged table"
        assert isinstance(args, _ffa_lib.MagiFfaBwdSparseArgs)
        # running sum of the k segment lengths, on the device: no host sync.
        # Built on the main stream BEFORE the side stream takes its wait on
        # it, and referenced until main has waited for side again: the dq
        # kernel may run on the side stream, which torch's allocator cannot
        # see, like the merged tables the caller holds.
        inner = dq_tables[1]
        k_cum = torch.zeros(inner.shape[0] + 1, dtype=torch.int32,
                            device=inner.device)
        k_cum[1:] = (inner[:, 1] - inner[:, 0]).clamp_min(0).cumsum(0)
        bwd_dq = _ffa_lib.lib().magi_ffa_bwd_dq_sparse
    cosched = env.is_bwd_cosched()
    side = _get_side_stream(device) if cosched else main
    if cosched:
        side.wait_stream(main)   # dpsum + inputs ready

    def set_tables(t, outer_is_q):
        if t is None:
            args.seg_starts = None
            return
        outer, inner, tm, starts = t
        args.q_ranges = ptr(outer if outer_is_q else inner)
        args.k_ranges = ptr(inner if outer_is_q else outer)
        args.attn_type_map = ptr(tm)
        args.seg_starts = ptr(starts)

    args.stream = ctypes.c_void_p(side.cuda_stream)
    set_tables(dq_tables, True)
    if k_cum is not None:
        args.k_cum, args.sparse_load = ptr(k_cum), 1
    check(bwd_dq(args), "magi_ffa_bwd_dq")
    if k_cum is not None:  # the dkv entries do not read them; leave none set
        args.k_cum, args.sparse_load = None, 0
    args.stream = ctypes.c_void_p(main.cuda_stream)
    set_tables(dkv_tables, False)
    if env.is_bwd_split_dkv(args.max_seqlen_k, args.d):
        check(bwd_dv(args), "magi_ffa_bwd_dv")
        check(bwd_dk(args), "magi_ffa_bwd_dk")
    else:
        check(bwd_dkv(args), "magi_ffa_bwd_dkv")
    if cosched:
        main.wait_stream(side)
    del k_cum  # main is ordered behind the dq kernel from here on


def bwd_swap_active(swap_bwd_qk_loop, dtype: torch.dtype, d: int) -> bool:
    """Whether a backward with this flag runs the one-pass q-outer kernel:
    there is one built for it (16-bit, d = 64 or 128). Otherwise the flag is
    accepted and the two passes run."""
    return (bool(swap_bwd_qk_loop)
            and dtype in (torch.bfloat16, torch.float16) and d in (64, 128))


def run_bwd_qloop(args, dq_tables=None) -> None:
    """swap_bwd_qk_loop (the caller has applied bwd_swap_active): dq, dk and
    dv from magi_ffa_bwd_qloop alone, on the current stream - no side stream,
    no dK/dV launch. dq_tables: the dq pass's merged table of run_bwd_passes
    under auto_range_merge (the caller keeps it alive), else args' flat one.
    dk and dv are f32 accumulators."""
    if dq_tables is not None:
        outer, inner, tm, starts = dq_tables
        args.q_ranges, args.k_ranges = ptr(outer), ptr(inner)
        args.attn_type_map, args.seg_starts = ptr(tm), ptr(starts)
    else:
        args.seg_starts = None
    args.stream = current_stream_ptr()
    check(_ffa_lib.lib().magi_ffa_bwd_qloop(args), "magi_ffa_bwd_qloop")


def run_bwd(args, q_ranges, k_ranges, attn_type_map, device, *,
            deterministic: bool, merged=None, sparse_load=False,
            swap_qk_loop=False) -> None:
    """The dq/dk/dv passes over a filled, preprocessed args; merged =
    (dq_tables, dkv_tables) of run_bwd_passes under auto_range_merge, and
    sparse_load its switch (merged tables only, which deterministic mode
    refuses, so it never meets the flag). swap_qk_loop (where bwd_swap_active):
    the one-pass kernel in place of them all, over merged[0] if there is one;
    sparse_load configures a pass that then does not run."""
    if swap_qk_loop:
        assert not deterministic, (
            "Deterministic mode is not supported when swap_bwd_qk_loop is "
            "enabled."
        )
        run_bwd_qloop(args, merged[0] if merged else None)
    elif deterministic:
        assert merged is None, "no deterministic mode over merged tables"
        run_bwd_deterministic(args, q_ranges, k_ranges, attn_type_map)
    else:
        run_bwd_passes(args, device, *(merged or ()), sparse_load=sparse_load)


# ---------------- index attention ----------------
def fwd_index(q, k, v, out, lse, indices_2d, softmax_scale, softcap, *,
              sink_f=None, s_sink=0, sink_ssh=False, max_logits=None,
              q_block_size=1, k_block_size=1) -> None:
    """Index (token-gather) forward into (out bf16, lse): the bf16 or the fp8
    entry by q.dtype. sink_f / s_sink come from _check_sink. q_block_size > 1
    (bf16): indices_2d has one row per block of that many q token rows and the
    BLOCK kernels of magi_ffa_fwd_index_block run; 1 is today's entry.
    k_block_size > 1: the entries of indices_2d are ids of blocks of that many
    K rows and the KBLOCK kernels of the *_kblock entries run; 1 is today's
    entries."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    block = q_block_size != 1
    assert not (block and q.dtype == _FP8), "no fp8 index kernel for q_block_size > 1"
    kblock = k_block_size != 1
    if kblock:
        cls = (_ffa_lib.MagiFfaIndexFp8KBlockArgs if q.dtype == _FP8
               else _ffa_lib.MagiFfaIndexKBlockArgs)
    else:
        cls = _ffa_lib.MagiFfaIndexBlockArgs if block else _ffa_lib.MagiFfaIndexArgs
    args = cls(
        q=ptr(q), k=ptr(k), v=ptr(v), out=ptr(out), lse=ptr(lse),
        indices_2d=ptr(indices_2d),
        total_q=tq, total_k=tk, max_topk=indices_2d.shape[1],
        hq=hq, hk=hk, d=d,
        softmax_scale=softmax_scale, softcap=softcap,
        out_is_fp32=0, stream=current_stream_ptr(),
        sink=ptr(sink_f), s_sink=s_sink,
        sink_ssh=int(sink_ssh), max_logits=ptr(max_logits),
    )
    lib = _ffa_lib.lib()
    if kblock:
        args.k_block_size = k_block_size
        if q.dtype == _FP8:
            check(lib.magi_ffa_fwd_index_fp8_kblock(args),
                  "magi_ffa_fwd_index_fp8_kblock")
        else:
            args.q_block_size = q_block_size
            check(lib.magi_ffa_fwd_index_kblock(args),
                  "magi_ffa_fwd_index_kblock")
        return
    if block:
        args.q_block_size = q_block_size
        check(lib.magi_ffa_fwd_index_block(args), "magi_ffa_fwd_index_block")
        return
    fn = lib.magi_ffa_fwd_index_fp8 if q.dtype == _FP8 else lib.magi_ffa_fwd_index
    check(fn(args), "magi_ffa_fwd_index")


def bwd_index(dout, q, k, v, out, lse, indices_2d, dq, dk, dv,
              softmax_scale, softcap, *, sink=None, sink_layout="sh",
              q_block_size=1, k_block_size=1):
    """Index backward: dpsum preprocess, the gather/scatter kernel into
    (dq, dk, dv) and, with a sink, its gradient; returns that or None.
    q_block_size and k_block_size as in fwd_index (magi_ffa_bwd_index_block,
    magi_ffa_bwd_index_kblock); the preprocess and dsink are row-wise and do
    not see them."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    dpsum = bwd_dpsum(dout, out)
    block = q_block_size != 1
    kblock = k_block_size != 1
    args = (_ffa_lib.MagiFfaIndexBwdKBlockArgs if kblock
            else _ffa_lib.MagiFfaIndexBwdBlockArgs if block
            else _ffa_lib.MagiFfaIndexBwdArgs)(
        dout=ptr(dout), q=ptr(q), k=ptr(k), v=ptr(v), lse=ptr(lse),
        dpsum=ptr(dpsum), indices_2d=ptr(indices_2d),
        dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
        total_q=tq, total_k=tk, max_topk=indices_2d.shape[1],
        hq=hq, hk=hk, d=d,
        softmax_scale=softmax_scale, softcap=softcap,
        stream=current_stream_ptr(),
    )
    if kblock:
        args.q_block_size = q_block_size
        args.k_block_size = k_block_size
        check(_ffa_lib.lib().magi_ffa_bwd_index_kblock(args),
              "magi_ffa_bwd_index_kblock")
    elif block:
        args.q_block_size = q_block_size
        check(_ffa_lib.lib().magi_ffa_bwd_index_block(args),
              "magi_ffa_bwd_index_block")
    else:
        check(_ffa_lib.lib().magi_ffa_bwd_index(args), "magi_ffa_bwd_index")
    if sink is None:
        return None
    sink_f, s_sink = _check_sink(sink, sink_layout, tq, hq)
    return bwd_dsink(sink_f, s_sink, sink_layout == "ssh", lse, dpsum)
