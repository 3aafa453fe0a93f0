# Single-GPU flex-flash-attention. Reference surface:
# magi_attention/functional/flex_flash_attn.py (merge_ranges:79,
# _flex_flash_attn_forward:334, _flex_flash_attn_backward:594,
# FlexFlashAttnFunc:699, flex_flash_attn_func:1066).
# MI355X-native: the JIT'd CUDA module is replaced by the C-ABI HIP library.
# This file validates, allocates and wires autograd; _ffa_launch.py launches.
from __future__ import annotations

import contextlib
from typing import Optional, Tuple

import torch

from .. import magi_attn_ext
from ..common.forward_meta import AttnForwardMeta
from . import _ffa_launch
from ._ffa_launch import (  # noqa: F401  (re-exported: tests and tools import them here)
    _apply_sink_postprocess,
    _check_sink,
    maybe_contiguous,
    run_bwd_deterministic,
    run_bwd_passes,
)


@contextlib.contextmanager
def maybe_profile_ffa_ctx(name: str, enable: bool = False):
    """Optional named-event timing around an FFA call (reference
    flex_flash_attn.py maybe_profile_ffa_ctx; magi_attn_ext event timers)."""
    if not enable:
        yield
        return
    magi_attn_ext.start_event(name)
    try:
        yield
    finally:
        magi_attn_ext.stop_event(name)


def merge_ranges(
    outer_ranges: torch.Tensor,
    inner_ranges: torch.Tensor,
    attn_type_map: torch.Tensor,
):
    """Sort + deduplicate (outer, inner) attention block pairs (reference
    flex_flash_attn.py:79 merge_ranges, built on the magi_attn_ext ops).
    Returns (merged_outer [n,2] zero-padded, sorted_outer, sorted_inner,
    sorted_attn_type_map, range_map inverse indices, unique_count [1])."""
    idx = magi_attn_ext.argsort_ranges(outer_ranges)
    so, si, st = magi_attn_ext.reorder_ranges_and_attn_type_maps(
        outer_ranges, inner_ranges, attn_type_map, idx
    )
    uniq, inverse, count = magi_attn_ext.unique_consecutive_pairs(so)
    n = outer_ranges.shape[0]
    merged = torch.zeros(n, 2, dtype=torch.int32, device=outer_ranges.device)
    merged[: uniq.shape[0]] = uniq
    return merged, so, si, st, inverse, count


def _seg_starts(inverse: torch.Tensor, n: int) -> torch.Tensor:
    """[n+1] cumulative segment starts from sorted inverse indices; entries
    past the unique count repeat the total, giving EMPTY segments — so the
    kernel grid can stay sized by n with no host sync on unique_count."""
    counts = torch.bincount(inverse.long(), minlength=n)
    starts = torch.zeros(n + 1, dtype=torch.int32, device=inverse.device)
    starts[1:] = counts.cumsum(0).to(torch.int32)
    return starts


def _merged_tables(outer_ranges, inner_ranges, attn_type_map) -> tuple:
    """A kernel's range tables under auto_range_merge: (unique outer ranges,
    inner ranges, attn_type_map, segment starts), outer = its OWN loop dim."""
    merged, _, inner, tm, inverse, _ = merge_ranges(
        outer_ranges, inner_ranges, attn_type_map
    )
    return merged, inner, tm, _seg_starts(inverse, outer_ranges.shape[0])


LOCK_GRAN = 128
_lock_cache: dict[tuple[int, int], torch.Tensor] = {}


def _get_locks(total_q: int, hq: int, device: torch.device) -> torch.Tensor:
    """Lock words for the fwd merge epilogue. Kernel always releases to 0, so
    the buffer can be cached and reused without re-zeroing."""
    slots = (total_q + LOCK_GRAN - 1) // LOCK_GRAN
    key = (device.index or 0, 0)
    buf = _lock_cache.get(key)
    need = slots * hq
    if buf is None or buf.numel() < need:
        buf = torch.zeros(max(need, 1 << 16), dtype=torch.int32, device=device)
        _lock_cache[key] = buf
    return buf


def _max_seqlen_of(ranges: torch.Tensor) -> int:
    if ranges.numel() == 0:
        return 0
    return int((ranges[:, 1] - ranges[:, 0]).amax().item())


def _flex_flash_attn_forward(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    sink: Optional[torch.Tensor],
    sink_layout: str,
    out: Optional[torch.Tensor],
    lse: Optional[torch.Tensor],
    q_ranges: torch.Tensor,
    k_ranges: torch.Tensor,
    attn_type_map: Optional[torch.Tensor],
    softmax_scale: float,
    softcap: float,
    out_type: Optional[torch.dtype],
    disable_fwd_atomic_reduction: bool,
    deterministic: bool,
    sm_margin: int,
    max_seqlen_q: Optional[int] = None,
    max_logits: Optional[torch.Tensor] = None,
    qk_starts: Optional[torch.Tensor] = None,
    **_unused,
) -> tuple[torch.Tensor, AttnForwardMeta]:
    """Dense (range-table) forward into (out, lse). q/k/v are all bf16, all
    fp16 or all fp8-e4m3. In merge mode out is an f32 accumulator; with
    disable_fwd_atomic_reduction it defaults to q's dtype, stored directly by
    the kernel, and a 16-bit out or out_type must be q's own 16-bit type.

    fp16 direct store with a sink: the sink postprocess kernel reads a 16-bit
    out as bf16, so it must never see fp16. That combination therefore runs
    the kernel into an f32 out, applies the sink there, and casts to fp16
    once at the end (into the caller's out if one was given); lse is
    unaffected."""
    is_fp8 = q.dtype == torch.float8_e4m3fn
    assert q.dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn), (
        "bf16, fp16 or fp8-e4m3 inputs"
    )
    # the kernel is picked from q.dtype alone and reads k and v as q's element
    # type: a mixed call would run past the end of the narrower buffers, or
    # read fp16 bits as bf16
    assert k.dtype == q.dtype and v.dtype == q.dtype, (
        "flex_flash_attn q, k and v must all be fp8-e4m3 or all be bf16 (or "
        f"all be fp16), got q={q.dtype}, k={k.dtype}, v={v.dtype}"
    )
    for what, t in (("out", None if out is None else out.dtype),
                    ("out_type", out_type)):
        assert t in (None, torch.float32) or t == (
            torch.bfloat16 if is_fp8 else q.dtype
        ), f"{what} {t} must be float32 or q's own 16-bit type, q={q.dtype}"
    q, k, v, q_ranges, k_ranges, attn_type_map = map(
        maybe_contiguous, (q, k, v, q_ranges, k_ranges, attn_type_map)
    )

    tq, hq, d = q.shape

    dtype = out.dtype if out is not None else out_type or (
        q.dtype if disable_fwd_atomic_reduction else torch.float32
    )
    # fp16 direct store + sink: f32 out through the sink, one cast at the end
    via_f32 = (sink is not None and disable_fwd_atomic_reduction
               and dtype == torch.float16)
    out_f16 = out if via_f32 else None
    if via_f32:
        out = None if out is None else out.float()
        dtype = torch.float32
    if out is None:
        out = torch.zeros(tq, hq, d, dtype=dtype, device=q.device)
    if lse is None:
        lse = torch.full((tq, hq), float("-inf"), dtype=torch.float32, device=q.device)

    out_is_fp32 = out.dtype == torch.float32
    if not disable_fwd_atomic_reduction:
        assert out_is_fp32, "atomic (merge) forward requires an fp32 out accumulator"
        locks = _get_locks(tq, hq, q.device)
    else:
        locks = None

    if max_seqlen_q is None:
        max_seqlen_q = _max_seqlen_of(q_ranges)

    if is_fp8:
        assert not disable_fwd_atomic_reduction and out_is_fp32
    if qk_starts is not None:
        assert not deterministic, (
            "deterministic + auto_range_merge lands in a later round"
        )
        assert not is_fp8, "fp8 + auto_range_merge lands in a later round"
    _ffa_launch.fwd(
        q, k, v, out, lse, q_ranges, k_ranges, attn_type_map,
        locks=locks, max_logits=max_logits, qk_starts=qk_starts,
        max_seqlen_q=max_seqlen_q, softmax_scale=softmax_scale,
        softcap=softcap,
        disable_fwd_atomic_reduction=disable_fwd_atomic_reduction,
        sm_margin=sm_margin, deterministic=deterministic,
    )
    if sink is not None:
        assert out.dtype != torch.float16  # the postprocess reads 16 bits as bf16
        _apply_sink_postprocess(out, lse, sink, sink_layout, tq, hq, d)
    if via_f32:
        out = out.half() if out_f16 is None else out_f16.copy_(out)
    return out, AttnForwardMeta(lse=lse, max_logits=max_logits)


def _flex_flash_attn_forward_index(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    indices_2d: torch.Tensor,
    softmax_scale: float,
    softcap: float,
    *,
    sink: Optional[torch.Tensor] = None,
    sink_layout: str = "sh",
    max_logits: Optional[torch.Tensor] = None,
) -> tuple[torch.Tensor, AttnForwardMeta]:
    """Index-attention (token-gather) forward: the reference's
    index_attn_indices direct-to-kernel path (flex_flash_attn.py:1358-1390).
    indices_2d [total_q, max_topk] int32 lists the GLOBAL K rows each q token
    row attends, shared by all hq query heads; -1 = contiguous tail padding.
    This is the forward pass; _flex_flash_attn_backward_index differentiates
    it (the reference backward receives None for index_attn).

    q/k/v are all bf16 (csrc/ffa_index.hip) or all fp8-e4m3
    (csrc/ffa_index_fp8.hip: raw e4m3 bytes, no descale factors, the fp8
    softmax convention of the dense fp8 forward); out is bf16 either way.

    sink ("sh" [s_sink, hq] or "ssh" [total_q, s_sink, hq], s_sink in [1, 8])
    is folded into out and lse inside the kernel's epilogue, in fp32 before
    out is rounded - there is no separate postprocess launch on this path.
    max_logits (f32 [hq], preset to -inf by the caller) receives the per-head
    maximum scaled (softcapped) logit over valid slots and comes back in the
    meta; sink logits do not enter it."""
    is_fp8 = q.dtype == torch.float8_e4m3fn
    assert q.dtype == torch.bfloat16 or is_fp8, "index_attn requires bf16 inputs"
    assert k.dtype == q.dtype and v.dtype == q.dtype, (
        "index_attn q, k and v must all be fp8-e4m3 or all be bf16, got "
        f"q={q.dtype}, k={k.dtype}, v={v.dtype}"
    )
    q, k, v, indices_2d = [maybe_contiguous(x) for x in (q, k, v, indices_2d)]
    tq, hq, d = q.shape
    tk, hk, _ = k.shape
    assert hk == 1, (
        "index_attn expects KV heads folded into the K row dimension "
        "(k of shape [total_k, 1, d]; global id = (b*S_kv + t)*NHK + h)"
    )
    assert indices_2d.dtype == torch.int32 and indices_2d.dim() == 2
    assert indices_2d.shape[0] == tq, (
        f"indices_2d rows ({indices_2d.shape[0]}) must match q token rows ({tq})"
    )
    sink_f, s_sink = None, 0
    if sink is not None:
        sink_f, s_sink = _check_sink(sink, sink_layout, tq, hq)
    if max_logits is not None:
        assert max_logits.dtype == torch.float32 and max_logits.shape == (hq,), (
            "max_logits must be f32 [hq]"
        )
        assert max_logits.is_contiguous()

    out = torch.zeros(tq, hq, d, dtype=torch.bfloat16, device=q.device)
    lse = torch.full((tq, hq), float("-inf"), dtype=torch.float32, device=q.device)

    _ffa_launch.fwd_index(
        q, k, v, out, lse, indices_2d, softmax_scale, softcap,
        sink_f=sink_f, s_sink=s_sink, sink_ssh=sink_layout == "ssh",
        max_logits=max_logits,
    )
    return out, AttnForwardMeta(lse=lse, max_logits=max_logits)


def _index_head_dim_pad(d: int) -> int:
    """zero columns that take head dim d to its kernel bucket (64 or 128)"""
    if d in (64, 128):
        return 0
    assert d < 128, f"index_attn head_dim {d} > 128 unsupported"
    return (64 if d <= 64 else 128) - d


def _pad_head_dim(t: torch.Tensor, pad: int) -> torch.Tensor:
    """Zero-pad the last dim. fp8 goes through a uint8 view (constant pad is
    not implemented for fp8 on every backend; zero bytes are e4m3 +0)."""
    if pad == 0:
        return t
    if t.dtype == torch.float8_e4m3fn:
        return torch.nn.functional.pad(
            t.contiguous().view(torch.uint8), (0, pad)
        ).view(torch.float8_e4m3fn)
    return torch.nn.functional.pad(t, (0, pad))


def _flex_flash_attn_backward_index(
    dout: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    out: torch.Tensor,
    lse: torch.Tensor,
    indices_2d: torch.Tensor,
    softmax_scale: float,
    softcap: float,
    sink: Optional[torch.Tensor] = None,
    sink_layout: str = "sh",
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Index-attention backward (csrc/ffa_index_bwd.hip): dpsum preprocess,
    then one gather/scatter kernel. Returns (dq bf16, dk fp32, dv fp32, dsink):
    dq has a single owner per row and is stored directly; dk/dv are fp32
    accumulators the kernel scatters into with atomic adds (not deterministic).

    With a sink, lse is the sink-corrected lse the forward saved and out the
    sink-scaled out, so the kernel's recomputed P and dpsum = rowsum(dO * O)
    already account for the sink (the dense path's argument); dsink (f32, the
    sink's shape) comes from magi_ffa_dsink over (sink, lse, dpsum). Without
    one dsink is None."""
    assert q.dtype == torch.bfloat16, "index_attn requires bf16 inputs"
    dout, q, k, v, out, lse, indices_2d = [
        maybe_contiguous(x) for x in (dout, q, k, v, out, lse, indices_2d)
    ]
    dout = dout.to(q.dtype)
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k, dtype=torch.float32)
    dv = torch.zeros_like(v, dtype=torch.float32)
    dsink = _ffa_launch.bwd_index(
        dout, q, k, v, out, lse, indices_2d, dq, dk, dv,
        softmax_scale, softcap, sink=sink, sink_layout=sink_layout,
    )
    return dq, dk, dv, dsink


def _index_attn_forward(ctx, q, k, v, indices_2d, softmax_scale, softcap,
                        sink, sink_layout, return_max_logits):
    """forward shared by IndexAttnFunc and IndexAttnSinkFunc"""
    d = q.shape[-1]
    pad = _index_head_dim_pad(d) if q.dtype == torch.float8_e4m3fn else 0
    max_logits = (_ffa_launch.new_max_logits(q.shape[1], q.device)
                  if return_max_logits else None)
    out, meta = _flex_flash_attn_forward_index(
        _pad_head_dim(q, pad), _pad_head_dim(k, pad), _pad_head_dim(v, pad),
        indices_2d, softmax_scale, softcap,
        sink=sink, sink_layout=sink_layout, max_logits=max_logits,
    )
    ctx.save_for_backward(q, k, v, out, meta.lse, indices_2d, sink)
    ctx.softmax_scale = softmax_scale
    ctx.softcap = softcap
    ctx.pad = pad
    ctx.sink_layout = sink_layout
    # one call: a second mark_non_differentiable would replace the first
    ctx.mark_non_differentiable(
        *(t for t in (meta.lse, max_logits) if t is not None)
    )
    return (out[..., :d] if pad else out), meta.lse, max_logits


def _index_attn_backward(ctx, dout, need_sink):
    """backward shared by IndexAttnFunc and IndexAttnSinkFunc: (dq, dk, dv,
    dsink) in the input dtypes, None where no gradient is needed"""
    q, k, v, out, lse, indices_2d, sink = ctx.saved_tensors
    in_dtype = q.dtype
    d = q.shape[-1]
    # ctx.pad is 0 unless the inputs are fp8
    q, k, v, dout = [
        _pad_head_dim(t, ctx.pad)
        for t in _ffa_launch.upcast_fp8(q, k, v, dout)
    ]
    need_sink = need_sink and sink is not None
    dq, dk, dv, dsink = _flex_flash_attn_backward_index(
        dout, q, k, v, out, lse, indices_2d,
        ctx.softmax_scale, ctx.softcap,
        sink=sink if need_sink else None, sink_layout=ctx.sink_layout,
    )
    need_q, need_k, need_v = ctx.needs_input_grad[:3]
    return (
        dq[..., :d].to(in_dtype) if need_q else None,
        dk[..., :d].to(in_dtype) if need_k else None,
        dv[..., :d].to(in_dtype) if need_v else None,
        dsink.to(sink.dtype) if need_sink else None,
    )


def _input_grads(func_cls, **grads) -> tuple:
    """What func_cls.backward returns: one gradient per forward input, in the
    signature's order - the ones given by input name, None for the rest."""
    code = func_cls.forward.__code__
    names = code.co_varnames[1:code.co_argcount]  # the inputs, ctx left out
    assert set(grads) <= set(names), (func_cls.__name__, names)
    return tuple(grads.get(n) for n in names)


class IndexAttnFunc(torch.autograd.Function):
    """Differentiable index attention: forward = the gather kernel, backward =
    preprocess + the gather/scatter kernel. The index tensor and the scalar
    arguments get no gradient.

    fp8-e4m3 inputs run the fp8 forward kernel; their backward runs the bf16
    kernels over upcast operands with the fp8 forward's out/lse, and the
    gradients are cast back to fp8 (the policy of _ffa_launch.upcast_fp8).
    An odd fp8 head dim is zero-padded here, not by the caller: the forward
    pads the bytes and the backward pads the bf16 upcast.

    This is the node of a call without sink and max_logits (six inputs, out
    and lse); IndexAttnSinkFunc below carries those two."""

    @staticmethod
    def forward(ctx, q, k, v, indices_2d, softmax_scale, softcap):
        out, lse, _ = _index_attn_forward(
            ctx, q, k, v, indices_2d, softmax_scale, softcap, None, "sh", False
        )
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        dq, dk, dv, _ = _index_attn_backward(ctx, dout, False)
        return _input_grads(IndexAttnFunc, q=dq, k=dk, v=dv)


class IndexAttnSinkFunc(torch.autograd.Function):
    """IndexAttnFunc with an attention sink and/or max_logits. The forward
    kernel folds the sink in; the saved lse is the sink-corrected one and the
    saved out the sink-scaled one, so the dQ/dK/dV kernel needs nothing more,
    and dsink comes from magi_ffa_dsink in f32 (for fp8 inputs too), returned
    in the sink's dtype, None when the sink needs no gradient. Returns (out,
    lse, max_logits); lse and max_logits are non-differentiable, max_logits
    is None unless return_max_logits."""

    @staticmethod
    def forward(ctx, q, k, v, indices_2d, softmax_scale, softcap,
                sink, sink_layout, return_max_logits):
        return _index_attn_forward(
            ctx, q, k, v, indices_2d, softmax_scale, softcap,
            sink, sink_layout, return_max_logits,
        )

    @staticmethod
    def backward(ctx, dout, *_):
        dq, dk, dv, dsink = _index_attn_backward(
            ctx, dout, ctx.needs_input_grad[6]
        )
        return _input_grads(IndexAttnSinkFunc, q=dq, k=dk, v=dv, sink=dsink)


def _flex_flash_attn_backward(
    dout: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    sink: Optional[torch.Tensor],
    sink_layout: str,
    out: torch.Tensor,
    lse: torch.Tensor,
    dq: Optional[torch.Tensor],
    dk: Optional[torch.Tensor],
    dv: Optional[torch.Tensor],
    dsink: Optional[torch.Tensor],
    q_ranges: torch.Tensor,
    k_ranges: torch.Tensor,
    attn_type_map: Optional[torch.Tensor],
    softmax_scale: float,
    softcap: float,
    dq_type: Optional[torch.dtype],
    dk_type: Optional[torch.dtype],
    dv_type: Optional[torch.dtype],
    disable_bwd_dkv_atomic_reduction: bool,
    deterministic: bool,
    sm_margin: int,
    max_seqlen_k: Optional[int] = None,
    auto_range_merge: bool = False,
    disable_bwd_dq_atomic_reduction: bool = False,
    cat_gqa: bool = False,
    **_unused,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Dense (range-table) backward; returns (dq, dk, dv, dsink). q/k/v are
    all bf16 or all fp16 (the autograd function upcasts fp8 before it calls).

    By default dq, dk and dv are zeroed f32 buffers that the kernels add
    their register tiles into with atomics, because ranges may overlap and
    the q heads of a GQA group share dK/dV rows.

    disable_bwd_dkv_atomic_reduction (reference flex_flash_attn.py:516,
    :642-647) is the caller's promise that the k ranges are disjoint - under
    auto_range_merge, the distinct ones, since duplicates merge into one
    owner. With hq == hk every dK/dV element then has one owner: dk and dv
    are zero-initialised in dk_type / dv_type, by default k.dtype, stored once
    by the kernel with no atomics, and returned in that dtype. The stored
    value is the f32 path's value cast to 16 bit (the same bits, but for a
    -0 where the f32 path, which adds no zeros, leaves +0). With GQA
    (hq != hk; the reference allows the flag for MHA or catGQA only) several
    q heads still add into one row, so without cat_gqa the flag falls back to
    the f32 atomic path and f32 comes back.

    cat_gqa (reference flex_flash_attn.py:1202) takes effect when hq != hk
    (with hq == hk it is today's launch): a dK/dV workgroup owns (k range, KV
    head, k block) in place of (k range, q head, k block), stages its K/V
    tiles once and walks the hq / hk q heads of its group into one register
    tile - q segments in table order, heads ascending within a segment. The
    epilogue runs once per KV head, so disjoint k ranges have one owner per
    dK/dV element and disable_bwd_dkv_atomic_reduction stores directly under
    GQA too. It composes with auto_range_merge, deterministic (one launch per
    k-disjoint group: no per-head sub-launches), the split and the fused dK/dV
    passes, softcap, sink and padded head dims. The dq pass is not touched.

    disable_bwd_dq_atomic_reduction is the same for dq and disjoint q ranges
    (dq_type, default q.dtype). The reference has no such flag, its dQ is not
    single-owner; here each wave owns its q tile for the whole k loop.

    dq_type / dk_type / dv_type are None, float32 (atomic path whatever the
    flag says) or q's own 16-bit type, which needs the matching flag (and
    hq == hk or cat_gqa for dk/dv); dk and dv share one dtype. Buffers passed in as dq /
    dk / dv are zeroed by the caller, follow the same rules by their dtype and
    are returned as they are. Neither promise is checked, as in the forward:
    that would take a device sync. With overlapping ranges a direct store
    loses all but one contribution.

    The context-parallel runtime (dist_attn.py) keeps f32 partial gradients,
    which it reduces across ranks, and does not use the direct stores."""
    dout, q, k, v, out, q_ranges, k_ranges, attn_type_map = map(
        maybe_contiguous, (dout, q, k, v, out, q_ranges, k_ranges, attn_type_map)
    )
    tq, hq, _ = q.shape
    hk = k.shape[1]
    # the kernels read dout, and a 16-bit out, as q's element type
    assert q.dtype in (torch.bfloat16, torch.float16)
    assert k.dtype == q.dtype and v.dtype == q.dtype
    assert out.dtype in (torch.float32, q.dtype)
    dout = dout.to(q.dtype)

    direct_dq = bool(disable_bwd_dq_atomic_reduction)
    cat_gqa = bool(cat_gqa) and hq != hk
    direct_dkv = bool(disable_bwd_dkv_atomic_reduction) and (
        hq == hk or cat_gqa
    )

    def grad_buffer(what, like, buf, want, direct, flag):
        """zeroed f32 accumulator, or 16-bit direct-store target"""
        dtype = buf.dtype if buf is not None else want or (
            q.dtype if direct else torch.float32
        )
        assert dtype in (torch.float32, q.dtype), (
            f"{what} {dtype} must be float32 or q's own 16-bit type, "
            f"q={q.dtype}"
        )
        assert dtype == torch.float32 or direct, (
            f"a 16-bit {what} ({dtype}) is stored directly and needs {flag}"
        )
        if buf is None:
            buf = torch.zeros_like(like, dtype=dtype)
        return buf

    dkv_flag = (
        "disable_bwd_dkv_atomic_reduction" if cat_gqa else
        f"disable_bwd_dkv_atomic_reduction with hq == hk (hq={hq}, hk={hk})"
    )
    dq = grad_buffer("dq", q, dq, dq_type, direct_dq,
                     "disable_bwd_dq_atomic_reduction")
    dk = grad_buffer("dk", k, dk, dk_type, direct_dkv, dkv_flag)
    dv = grad_buffer("dv", v, dv, dv_type, direct_dkv, dkv_flag)
    assert dk.dtype == dv.dtype, (
        f"dk and dv share one epilogue: dk={dk.dtype}, dv={dv.dtype}"
    )
    dpsum = torch.empty(tq, hq, dtype=torch.float32, device=q.device)

    if max_seqlen_k is None:
        max_seqlen_k = _max_seqlen_of(k_ranges)

    args = _ffa_launch.bwd_args(
        dout, out, dpsum, q=q, k=k, v=v, lse=lse, dq=dq, dk=dk, dv=dv,
        q_ranges=q_ranges, k_ranges=k_ranges, attn_type_map=attn_type_map,
        max_seqlen_k=max_seqlen_k, softmax_scale=softmax_scale,
        softcap=softcap, sm_margin=sm_margin, cat_gqa=cat_gqa,
    )
    _ffa_launch.bwd_preprocess(args)
    if sink is not None:
        sink_f, s_sink = _check_sink(sink, sink_layout, tq, hq)
        dsink = _ffa_launch.bwd_dsink(
            sink_f, s_sink, sink_layout == "ssh", lse, dpsum, dsink
        )
    merged = None
    if deterministic:
        assert not auto_range_merge, (
            "deterministic + auto_range_merge lands in a later round"
        )
    elif auto_range_merge:
        # dq pass: unique q ranges with k segments; dkv pass: unique k
        # ranges with q segments (reference bwd_kq_map)
        merged = (_merged_tables(q_ranges, k_ranges, attn_type_map),
                  _merged_tables(k_ranges, q_ranges, attn_type_map))
    _ffa_launch.run_bwd(
        args, q_ranges, k_ranges, attn_type_map, q.device,
        deterministic=deterministic, merged=merged,
    )
    return dq, dk, dv, dsink


class FlexFlashAttnFunc(torch.autograd.Function):
    @staticmethod
    def forward(
        ctx,
        q, k, v, sink, sink_layout,
        q_ranges, k_ranges, attn_type_map,
        softmax_scale=None, softcap=0.0, deterministic=False, sm_margin=0,
        disable_fwd_atomic_reduction=False,
        disable_bwd_dkv_atomic_reduction=False,
        ref_block_size=None, max_seqlen_q=None,
        auto_range_merge=False, swap_ab=False, pack_gqa=False, cat_gqa=False,
        sparse_load=False, index_attn=False, swap_bwd_qk_loop=False,
        return_max_logits=False, index_attn_indices_2d=None,
        index_attn_max_topk=0, max_seqlen_k=None,
    ):
        softmax_scale = (
            q.shape[-1] ** (-0.5) if softmax_scale is None else softmax_scale
        )
        assert q_ranges is not None and k_ranges is not None
        assert q_ranges.size(0) == k_ranges.size(0)
        fwd_q_ranges, fwd_k_ranges, fwd_tm = q_ranges, k_ranges, attn_type_map
        fwd_qk_starts = None
        if auto_range_merge:
            assert attn_type_map is not None, (
                "auto_range_merge requires an explicit attn_type_map"
            )
            fwd_q_ranges, fwd_k_ranges, fwd_tm, fwd_qk_starts = (
                _merged_tables(q_ranges, k_ranges, attn_type_map)
            )
        max_logits = None
        if return_max_logits:
            assert q.shape[1] <= 128, "num_qheads must be <= 128 (reference cap)"
            max_logits = _ffa_launch.new_max_logits(q.shape[1], q.device)

        out, meta = _flex_flash_attn_forward(
            q=q, k=k, v=v, sink=sink, sink_layout=sink_layout,
            out=None, lse=None,
            q_ranges=fwd_q_ranges, k_ranges=fwd_k_ranges,
            attn_type_map=fwd_tm,
            softmax_scale=softmax_scale, softcap=softcap, out_type=None,
            disable_fwd_atomic_reduction=disable_fwd_atomic_reduction,
            deterministic=deterministic, sm_margin=sm_margin,
            max_seqlen_q=max_seqlen_q, max_logits=max_logits,
            qk_starts=fwd_qk_starts,
        )
        lse = meta.lse
        # fp8 extension returns bf16 out
        out = out.to(torch.bfloat16 if q.dtype == torch.float8_e4m3fn else q.dtype)
        ctx.save_for_backward(q, k, v, out, lse, q_ranges, k_ranges,
                              attn_type_map, sink)
        ctx.softmax_scale = softmax_scale
        ctx.softcap = softcap
        ctx.deterministic = deterministic
        ctx.sm_margin = sm_margin
        ctx.sink_layout = sink_layout
        ctx.auto_range_merge = auto_range_merge
        # the caller's two promises of disjoint ranges: the forward flag says
        # the q ranges are, which is what a direct dQ store needs as well
        ctx.disable_bwd_dq_atomic_reduction = disable_fwd_atomic_reduction
        ctx.disable_bwd_dkv_atomic_reduction = disable_bwd_dkv_atomic_reduction
        # avoid a per-backward device sync to size the bwd grid
        ctx.max_seqlen_k = max_seqlen_k
        ctx.cat_gqa = cat_gqa
        if max_logits is not None:
            ctx.mark_non_differentiable(max_logits)
        return out, lse, max_logits

    @staticmethod
    def backward(ctx, dout, *_):
        (q, k, v, out, lse, q_ranges, k_ranges, attn_type_map,
         sink) = ctx.saved_tensors
        in_dtype = q.dtype
        # fp8 gradients are cast f32 -> fp8 once; a direct bf16 store in
        # between would round twice, so fp8 keeps the f32 accumulators
        direct_ok = in_dtype != torch.float8_e4m3fn
        q, k, v, out, dout = _ffa_launch.upcast_fp8(q, k, v, out, dout)
        dq, dk, dv, dsink = _flex_flash_attn_backward(
            dout=dout, q=q, k=k, v=v, sink=sink, sink_layout=ctx.sink_layout,
            out=out, lse=lse, dq=None, dk=None, dv=None, dsink=None,
            q_ranges=q_ranges, k_ranges=k_ranges, attn_type_map=attn_type_map,
            softmax_scale=ctx.softmax_scale, softcap=ctx.softcap,
            dq_type=None, dk_type=None, dv_type=None,
            disable_bwd_dkv_atomic_reduction=(
                direct_ok and ctx.disable_bwd_dkv_atomic_reduction),
            deterministic=ctx.deterministic, sm_margin=ctx.sm_margin,
            max_seqlen_k=ctx.max_seqlen_k,
            auto_range_merge=ctx.auto_range_merge,
            disable_bwd_dq_atomic_reduction=(
                direct_ok and ctx.disable_bwd_dq_atomic_reduction),
            cat_gqa=ctx.cat_gqa,
        )
        if sink is not None and dsink is not None:
            dsink = dsink.to(sink.dtype)
        return _input_grads(
            FlexFlashAttnFunc, q=dq.to(in_dtype), k=dk.to(in_dtype),
            v=dv.to(in_dtype), sink=dsink,
        )


def flex_flash_attn_func(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    q_ranges: Optional[torch.Tensor] = None,
    k_ranges: Optional[torch.Tensor] = None,
    attn_type_map: Optional[torch.Tensor] = None,
    *,
    index_attn_indices: Optional[torch.Tensor] = None,
    q_block_size: int = 1,
    k_block_size: int = 1,
    sink: Optional[torch.Tensor] = None,
    sink_layout: str = "sh",
    softmax_scale: Optional[float] = None,
    softcap: float = 0.0,
    deterministic: bool = False,
    sm_margin: int = 0,
    disable_fwd_atomic_reduction: bool = False,
    disable_bwd_dkv_atomic_reduction: bool = False,
    ref_block_size: Optional[Tuple[int, int]] = None,
    max_seqlen_q: Optional[int] = None,
    auto_range_merge: bool = False,
    swap_ab: bool = False,
    pack_gqa: bool = False,
    cat_gqa: bool = False,
    sparse_load: bool = False,
    index_attn: bool = False,
    swap_bwd_qk_loop: bool = False,
    return_max_logits: bool = False,
    max_seqlen_k: Optional[int] = None,
) -> tuple[torch.Tensor, AttnForwardMeta]:
    """Single-GPU flex-flash-attention (drop-in for the reference
    flex_flash_attn_func, flex_flash_attn.py:1066; full mask semantics in the
    reference docstring :1247-1341). Returns (out, AttnForwardMeta(lse=...)).

    index_attn_indices (reference :1358-1390): (total_q, num_kv_heads,
    max_topk) int32 GLOBAL K row ids, -1 tail padding, mutually exclusive
    with q_ranges/k_ranges; max_topk must be a multiple of 64 (the MI355X
    staged-tile size; the reference requires 128, so any reference-legal
    input is accepted). Differentiable in q, k and v on the GPU (the
    reference is forward-only here): dK/dV are scattered with fp32 atomic
    adds, so deterministic=True is rejected when a gradient is needed.
    q/k/v may be all bf16 or all float8_e4m3fn (fp8 forward kernel, bf16 out,
    bf16-upcast backward, fp8 gradients).
    sink / sink_layout and return_max_logits take effect on this path as on
    the range path: the sink ("sh" [s_sink, hq] or "ssh" [total_q, s_sink,
    hq], s_sink in [1, 8]) is folded into out and lse in the kernel's
    epilogue (a token whose list is all -1 gets out = 0, lse = lse_sink) and
    is differentiable (dsink in sink.dtype, f32 math, fp8 inputs included);
    meta.max_logits is the per-head f32 [hq] maximum scaled (softcapped)
    logit over valid slots (-inf if there is none), hq <= 128, and the sink
    logits do not enter it.

    On the range path q/k/v may also be all float16: out and the gradients
    come back in fp16, lse / max_logits / dsink math stays f32, and every
    option of the bf16 path applies (padded head dims, sink, softcap,
    deterministic, auto_range_merge, direct store). P and dS are rounded to
    fp16 before their MFMAs and accumulate in fp32. Mixed 16-bit dtypes are
    rejected; index_attn_indices stays bf16 / fp8 only.

    Backward stores (range path, bf16 / fp16). By default dq, dk and dv are
    accumulated with atomics in f32 buffers and cast once at the end.
    disable_bwd_dkv_atomic_reduction=True is the promise that the k ranges
    are disjoint (with auto_range_merge: the distinct k ranges); with
    hq == hk the dK/dV kernels then store their tiles directly in the input
    dtype - no f32 buffers, no atomics, no cast pass - and the gradients are
    equal to the default path's element for element (an exact -0 aside, which
    the default path returns as +0). With GQA (hq != hk) and no cat_gqa the
    flag is accepted and the f32 atomic path runs (the reference allows it for
    MHA or catGQA only). cat_gqa=True (it acts when hq != hk) makes each dK/dV
    workgroup own a KV head: it stages K/V once and walks the hq / hk q heads
    of the group into one register tile, in place of hq / hk workgroups that
    stage the same tiles and add into the same rows. dK/dV then get one add
    per KV head, deterministic=True needs no per-head sub-launches, and
    with the dkv flag the direct store runs under GQA as well, equal element
    for element to the cat_gqa f32 gradients cast to the input dtype. It
    cannot be combined with pack_gqa; whether it pays is measured in
    profiles/bwd_cat_gqa.md. disable_fwd_atomic_reduction=True, the promise that the q
    ranges are disjoint, makes the dQ kernel store directly in the same way
    (the reference has no direct dQ). Neither promise is checked; ranges
    that do overlap lose contributions. fp8 inputs keep f32 accumulators
    whatever the flags say, and so does the context-parallel runtime, whose
    partial gradients are reduced across ranks in f32. What the direct
    stores save is measured in profiles/bwd_direct_store.md."""
    assert not (pack_gqa and cat_gqa), "pack_gqa and cat_gqa cannot be both True"
    # ── sparse-input validation (mirrors reference :1344-1384) ──
    _has_ranges = q_ranges is not None
    _has_index = index_attn_indices is not None
    assert int(_has_ranges) + int(_has_index) == 1, (
        "Exactly one of (q_ranges + k_ranges) or index_attn_indices must be "
        "provided"
    )
    assert not (sparse_load and _has_index), (
        "sparse_load and index_attn_indices are mutually exclusive"
    )
    if _has_index:
        assert index_attn_indices.dim() == 3, (
            f"index_attn_indices must be 3D (total_q, num_kv_heads, max_topk), "
            f"got shape {tuple(index_attn_indices.shape)}"
        )
        assert q_block_size == 1 and k_block_size == 1, (
            "only q_block_size=1 / k_block_size=1 (token granularity) is "
            "supported for index_attn"
        )
        max_topk = index_attn_indices.shape[2]
        assert max_topk % 64 == 0, (
            f"index_attn max_topk={max_topk} must be a multiple of 64 "
            f"(pad with -1)"
        )
        # the differentiable path is taken only when a gradient can flow; the
        # no-grad call below is the plain forward launch
        needs_grad = torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (q, k, v, sink)
        )
        if needs_grad:
            assert q.is_cuda and k.is_cuda and v.is_cuda, (
                "index_attn backward needs GPU tensors (the gather/scatter "
                "kernel takes device pointers only)"
            )
            assert not deterministic, (
                "index_attn backward has no deterministic mode: dK/dV are "
                "scattered with fp32 atomic adds, whose order is not fixed; "
                "pass deterministic=False"
            )
        if softmax_scale is None:
            softmax_scale = q.shape[-1] ** (-0.5)
        indices_2d = index_attn_indices.reshape(-1, max_topk)
        if return_max_logits:
            assert q.shape[1] <= 128, "num_qheads must be <= 128 (reference cap)"

        def _index_call(q_, k_, v_):
            if needs_grad:
                if sink is None and not return_max_logits:
                    out_, lse_ = IndexAttnFunc.apply(
                        q_, k_, v_, indices_2d, softmax_scale, softcap
                    )
                    return out_, AttnForwardMeta(lse=lse_, max_logits=None)
                out_, lse_, ml_ = IndexAttnSinkFunc.apply(
                    q_, k_, v_, indices_2d, softmax_scale, softcap,
                    sink, sink_layout, return_max_logits,
                )
                return out_, AttnForwardMeta(lse=lse_, max_logits=ml_)
            ml_ = (_ffa_launch.new_max_logits(q_.shape[1], q_.device)
                   if return_max_logits else None)
            return _flex_flash_attn_forward_index(
                q_, k_, v_, indices_2d, softmax_scale, softcap,
                sink=sink, sink_layout=sink_layout, max_logits=ml_,
            )

        d = q.shape[-1]
        if d not in (64, 128):
            # zero-pad odd head dims into the next bucket (same scheme as the
            # dense path below; exact for attention, and autograd slices the
            # gradients back through the pad)
            pad = _index_head_dim_pad(d)
            if needs_grad and q.dtype == torch.float8_e4m3fn:
                # fp8 under autograd: IndexAttnFunc pads inside (a byte-view
                # pad is not differentiable)
                return _index_call(q, k, v)
            out, meta = _index_call(
                _pad_head_dim(q, pad), _pad_head_dim(k, pad),
                _pad_head_dim(v, pad),
            )
            return out[..., :d], meta
        return _index_call(q, k, v)
    d = q.shape[-1]
    if d not in (64, 128, 192):
        # arbitrary head dims run in the next bucket with zero feature
        # padding — exact for attention (padding contributes 0 to scores;
        # padded V columns are sliced off; gradients slice back through the
        # autograd pad). Reference buckets head_size <=64/<=128/<=192
        # (flash_api.cpp:322-334); the 192 bucket lands with a D=192 kernel.
        assert d < 192, f"head_dim {d} > 192 is beyond the reference's buckets"
        assert q.dtype in (torch.bfloat16, torch.float16), (
            "padded head dims require bf16 or fp16"
        )
        bucket = 64 if d <= 64 else (128 if d <= 128 else 192)
        if softmax_scale is None:
            softmax_scale = d ** (-0.5)  # scale from the REAL head dim
        pad = bucket - d
        qp = torch.nn.functional.pad(q, (0, pad))
        kp = torch.nn.functional.pad(k, (0, pad))
        vp = torch.nn.functional.pad(v, (0, pad))
        out, meta = flex_flash_attn_func(
            qp, kp, vp, q_ranges, k_ranges, attn_type_map,
            sink=sink, sink_layout=sink_layout, softmax_scale=softmax_scale,
            softcap=softcap, deterministic=deterministic, sm_margin=sm_margin,
            disable_fwd_atomic_reduction=disable_fwd_atomic_reduction,
            disable_bwd_dkv_atomic_reduction=disable_bwd_dkv_atomic_reduction,
            max_seqlen_q=max_seqlen_q, max_seqlen_k=max_seqlen_k,
            auto_range_merge=auto_range_merge,
            return_max_logits=return_max_logits,
            pack_gqa=pack_gqa, cat_gqa=cat_gqa,
        )
        return out[..., :d], meta
    out, lse, max_logits = FlexFlashAttnFunc.apply(
        q, k, v, sink, sink_layout, q_ranges, k_ranges, attn_type_map,
        softmax_scale, softcap, deterministic, sm_margin,
        disable_fwd_atomic_reduction, disable_bwd_dkv_atomic_reduction,
        ref_block_size, max_seqlen_q, auto_range_merge, swap_ab, pack_gqa,
        cat_gqa, sparse_load, index_attn, swap_bwd_qk_loop, return_max_logits,
        None, 0, max_seqlen_k,
    )
    return out, AttnForwardMeta(lse=lse, max_logits=max_logits)
