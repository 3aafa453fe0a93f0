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
def fwd(q, k, v, out, lse, q_ranges, k_ranges, attn_type_map, *, locks,
        max_logits, qk_starts, max_seqlen_q, softmax_scale, softcap,
        disable_fwd_atomic_reduction, sm_margin, deterministic) -> None:
    """Dense forward into (out, lse): the fp8 entry or the 16-bit one (bf16 or
    fp16 by elem_type) by q.dtype;
    deterministic = fixed merge order, one launch per q-disjoint range group."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    args = _ffa_lib.MagiFfaFwdArgs(
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
             cat_gqa=False) -> _ffa_lib.MagiFfaBwdCatArgs:
    """The backward argument struct. (dout, out, dpsum) are all the dpsum
    preprocess reads; the dq/dk/dv passes need every member. The tensors must
    be contiguous and outlive the launches. dout's dtype (bf16 or fp16) is the
    element type of q/k/v too, and of a 16-bit out. The struct is the one of
    the magi_ffa_bwd_*_cat entries (it passes as the _direct and the plain one
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

    return _ffa_lib.MagiFfaBwdCatArgs(
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


def run_bwd_passes(args, device, dq_tables=None, dkv_tables=None) -> None:
    """Launch the independent backward passes (dq / fused-dkv by default;
    dq / dv / dk with MAGI_BWD_SPLIT_DKV=1) on two streams so their waves
    co-schedule across the chip. dq_tables / dkv_tables override the range
    tables per pass for auto_range_merge: (ranges_outer, ranges_inner,
    attn_type_map, seg_starts) — outer = the pass's OWN loop dim."""
    bwd_dq, bwd_dkv, bwd_dv, bwd_dk = _bwd_entries(args)
    main = torch.cuda.current_stream(device)
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
    check(bwd_dq(args), "magi_ffa_bwd_dq")
    args.stream = ctypes.c_void_p(main.cuda_stream)
    set_tables(dkv_tables, False)
    if env.is_bwd_split_dkv(args.max_seqlen_k, args.d):
        check(bwd_dv(args), "magi_ffa_bwd_dv")
        check(bwd_dk(args), "magi_ffa_bwd_dk")
    else:
        check(bwd_dkv(args), "magi_ffa_bwd_dkv")
    if cosched:
        main.wait_stream(side)


def run_bwd(args, q_ranges, k_ranges, attn_type_map, device, *,
            deterministic: bool, merged=None) -> None:
    """The dq/dk/dv passes over a filled, preprocessed args; merged =
    (dq_tables, dkv_tables) of run_bwd_passes under auto_range_merge."""
    if deterministic:
        assert merged is None, "no deterministic mode over merged tables"
        run_bwd_deterministic(args, q_ranges, k_ranges, attn_type_map)
    else:
        run_bwd_passes(args, device, *(merged or ()))


# ---------------- index attention ----------------
def fwd_index(q, k, v, out, lse, indices_2d, softmax_scale, softcap, *,
              sink_f=None, s_sink=0, sink_ssh=False, max_logits=None) -> None:
    """Index (token-gather) forward into (out bf16, lse): the bf16 or the fp8
    entry by q.dtype. sink_f / s_sink come from _check_sink."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    args = _ffa_lib.MagiFfaIndexArgs(
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
    fn = lib.magi_ffa_fwd_index_fp8 if q.dtype == _FP8 else lib.magi_ffa_fwd_index
    check(fn(args), "magi_ffa_fwd_index")


def bwd_index(dout, q, k, v, out, lse, indices_2d, dq, dk, dv,
              softmax_scale, softcap, *, sink=None, sink_layout="sh"):
    """Index backward: dpsum preprocess, the gather/scatter kernel into
    (dq, dk, dv) and, with a sink, its gradient; returns that or None."""
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    dpsum = bwd_dpsum(dout, out)
    args = _ffa_lib.MagiFfaIndexBwdArgs(
        dout=ptr(dout), q=ptr(q), k=ptr(k), v=ptr(v), lse=ptr(lse),
        dpsum=ptr(dpsum), indices_2d=ptr(indices_2d),
        dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
        total_q=tq, total_k=tk, max_topk=indices_2d.shape[1],
        hq=hq, hk=hk, d=d,
        softmax_scale=softmax_scale, softcap=softcap,
        stream=current_stream_ptr(),
    )
    check(_ffa_lib.lib().magi_ffa_bwd_index(args), "magi_ffa_bwd_index")
    if sink is None:
        return None
    sink_f, s_sink = _check_sink(sink, sink_layout, tq, hq)
    return bwd_dsink(sink_f, s_sink, sink_layout == "ssh", lse, dpsum)
