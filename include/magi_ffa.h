/* magi_ffa.h — C-ABI boundary of the MI355X-native flex-flash-attention engine.
 *
 * These entry points are the drop-in replacement for the reference's JIT'd FFA
 * kernel module surface (reference: magi_attention/functional/flex_flash_attn.py:261-290
 * `mod.fwd`, :527-554 `mod.bwd`, resolved by _flex_flash_attn_jit.py:456
 * `get_ffa_jit_mod`). The host side (magi_attention/functional/flex_flash_attn.py
 * in THIS repo) binds them via ctypes; INTEGRATION.md shows the binding a
 * maintainer would add.
 *
 * Conventions: all device pointers; q/k/v row-major [tokens, heads, dim], bf16
 * unless an entry says otherwise: the dense entries (magi_ffa_fwd,
 * magi_ffa_bwd*) take bf16 or fp16 by the elem_type member of their args,
 * the *_fp8 entries raw e4m3 bytes; the index entries are bf16 only;
 * ranges int32 [n,2] half-open; attn_type_map int32 (0=full, 1=causal,
 * 2=inv_causal, 3=bi_causal; semantics = reference flex_flash_attn.py:1247-1341);
 * stream is a hipStream_t. All functions return 0 on success, nonzero hipError_t
 * or negative validation error otherwise.
 */
#ifndef MAGI_FFA_H
#define MAGI_FFA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Element type of the dense entries' 16-bit tensors (elem_type members). */
#define MAGI_FFA_ELEM_BF16 0
#define MAGI_FFA_ELEM_FP16 1

typedef struct magi_ffa_fwd_args {
  const void* q;            /* elem_type [total_q, hq, d] */
  const void* k;            /* elem_type [total_k, hk, d] */
  const void* v;            /* elem_type [total_k, hk, d] */
  void* out;                /* f32 (accumulate/merge mode) or elem_type
                               [total_q, hq, d] */
  float* lse;               /* f32 [total_q, hq], caller-initialised to -inf */
  const int32_t* q_ranges;  /* [n, 2] */
  const int32_t* k_ranges;  /* [n, 2] */
  const int32_t* attn_type_map; /* [n] or NULL (= all full) */
  int32_t* locks;           /* zeroed int32 [ceil(total_q/128) * hq]; NULL iff
                               disable_atomic_reduction */
  float* max_logits;        /* f32 [hq] init -inf, atomic-max of the scaled
                               (softcapped) logits per head; NULL = off
                               (reference return_max_logits) */
  const int32_t* qk_starts; /* auto_range_merge: [n_ranges+1]; q_ranges are
                               UNIQUE, k segments per unique q range; NULL =
                               one k range per q range */
  int64_t n_ranges;
  int64_t total_q;
  int64_t total_k;
  int32_t hq;
  int32_t hk;
  int32_t d;                /* head dim: 64 or 128 */
  int32_t max_seqlen_q;     /* upper bound on max q-range length */
  float softmax_scale;
  float softcap;            /* 0 = disabled; else score=softcap*tanh(s*scale/softcap),
                               softmax scale becomes softcap (reference
                               mainloop_fwd...hpp:466-489) */
  int32_t out_is_fp32;      /* 1: out is f32 accumulator (merge into it);
                               0: elem_type direct store (requires
                               disable_atomic_reduction) */
  int32_t disable_atomic_reduction; /* 1: q_ranges disjoint, skip lock/merge */
  int32_t cu_margin;        /* CUs left free for comm kernels (sm_margin analogue) */
  void* stream;             /* hipStream_t */
  int32_t elem_type;        /* MAGI_FFA_ELEM_*: type of q/k/v, and of out when
                               out_is_fp32 == 0; a zero-filled struct is bf16 */
} magi_ffa_fwd_args;

/* Validation of magi_ffa_fwd, in this order, all before any HIP call: -1 null
 * pointer, -2 d not in {64, 128, 192}, -3 hq % hk != 0, -9 elem_type not one
 * of MAGI_FFA_ELEM_*; then n_ranges <= 0 returns 0 without a launch; -4 merge
 * mode without locks, -5 more than 65535 ranges, -10 merge mode into a 16-bit
 * out. magi_ffa_fwd_fp8 (raw e4m3 q/k/v) ignores elem_type. */
int magi_ffa_fwd(const magi_ffa_fwd_args* args);

typedef struct magi_ffa_bwd_args {
  const void* dout;         /* elem_type [total_q, hq, d] */
  const void* q;            /* elem_type [total_q, hq, d] */
  const void* k;            /* elem_type [total_k, hk, d] */
  const void* v;            /* elem_type [total_k, hk, d] */
  const void* out;          /* elem_type or f32 [total_q, hq, d] (forward output) */
  const float* lse;         /* f32 [total_q, hq] */
  void* dq;                 /* [total_q, hq, d], zeroed: f32, atomic-accumulated
                               (elem_type through the *_direct entries below) */
  void* dk;                 /* [total_k, hk, d], as dq */
  void* dv;                 /* [total_k, hk, d], as dq */
  float* dpsum;             /* f32 [total_q, hq] workspace = rowsum(dO*O) */
  const int32_t* q_ranges;  /* [n, 2] */
  const int32_t* k_ranges;  /* [n, 2] */
  const int32_t* attn_type_map; /* [n] or NULL */
  const int32_t* seg_starts;    /* auto_range_merge: [n_ranges+1] segment map
                                   (dq: q->k segments; dkv: k->q segments);
                                   NULL = one segment per range */
  int64_t n_ranges;
  int64_t total_q;
  int64_t total_k;
  int32_t hq;
  int32_t hk;
  int32_t d;
  int32_t max_seqlen_k;     /* upper bound on max k-range length */
  int32_t out_is_fp32;      /* dtype of `out` above */
  float softmax_scale;
  float softcap;
  int32_t cu_margin;
  void* stream;
  int32_t elem_type;        /* MAGI_FFA_ELEM_*: type of dout/q/k/v, and of out
                               when out_is_fp32 == 0; zero-filled = bf16 */
} magi_ffa_bwd_args;

/* Every backward entry below (_preprocess, _dq, _dkv, _dv, _dk and
 * magi_ffa_bwd) returns -9 for an elem_type that is not one of
 * MAGI_FFA_ELEM_*, after its null-pointer (-1), head-dim (-2) and GQA (-3)
 * checks and before any HIP call; then n_ranges <= 0 returns 0 without a
 * launch. Through these entries dq/dk/dv are f32 for both element types. */

/* dPsum preprocess: dpsum[t,h] = sum_d dout[t,h,d] * out[t,h,d]
 * (reference flash_bwd_preprocess_kernel.h:42). */
int magi_ffa_bwd_preprocess(const magi_ffa_bwd_args* args);

/* 5-matmul backward (reference flash_bwd_kernel_sm90.h:41), split into two
 * INDEPENDENT passes so the host may run them on separate streams
 * concurrently: the dq pass (q-outer, dQ register-accumulated) and the dkv
 * pass (k-outer, dK/dV register-accumulated). Both require dpsum filled.
 * magi_ffa_bwd runs both sequentially on args->stream. */
int magi_ffa_bwd_dq(const magi_ffa_bwd_args* args);
int magi_ffa_bwd_dkv(const magi_ffa_bwd_args* args);
/* dv/dk pass split of magi_ffa_bwd_dkv: each half re-derives S but fits
 * 2 waves/SIMD on gfx950; launching both is result-identical to the fused
 * kernel up to fp32 atomic-add ordering. */
int magi_ffa_bwd_dv(const magi_ffa_bwd_args* args);
int magi_ffa_bwd_dk(const magi_ffa_bwd_args* args);
int magi_ffa_bwd(const magi_ffa_bwd_args* args);

/* Direct 16-bit gradient stores for disjoint ranges. magi_ffa_bwd_args keeps
 * its size and its last member (bindings check both), so the two switches
 * ride behind an embedded copy of it, and the passes that honour them are
 * entries of their own. With both members 0 an entry is its namesake above,
 * bit for bit.
 *   dq_is_16bit   1: args.dq is a zeroed elem_type buffer and the q ranges
 *                 (the unique ones under seg_starts) are disjoint: the dq pass
 *                 stores each register tile once, rounded to nearest even,
 *                 with no atomics.
 *   dkv_is_16bit  1: the same for args.dk and args.dv, the k ranges and the
 *                 dkv / dv / dk passes; needs hq == hk.
 * The direct stores write every row of a range that a live tile covers, zeros
 * included, and nothing else: rows outside every range keep the caller's
 * zeros, as with f32. The promised disjointness is not checked; where ranges
 * do overlap the last writer wins. On single-owner input the stored value is
 * numerically the f32 path's value cast to elem_type: the same bits, except
 * that an exact -0 tile value is stored as -0 where the f32 path, which adds
 * no zeros, leaves the caller's +0.
 * Validation, in this order, all before any HIP call: -1 null pointer, -2
 * head dim, -3 hq % hk != 0, -9 elem_type; then, in _dkv_direct, _dv_direct
 * and _dk_direct with dkv_is_16bit set and whatever n_ranges is: -11 hq != hk
 * (several q heads add into one dK/dV row), -12 a deterministic GQA head
 * split packed into cu_margin's top 16 bits; then n_ranges <= 0 returns 0
 * without a launch. magi_ffa_bwd_direct_args_size is sizeof of the struct as
 * compiled (magi_ffa_args_size keeps its list). */
typedef struct magi_ffa_bwd_direct_args {
  magi_ffa_bwd_args args;
  int32_t dq_is_16bit;
  int32_t dkv_is_16bit;
} magi_ffa_bwd_direct_args;

int magi_ffa_bwd_dq_direct(const magi_ffa_bwd_direct_args* args);
int magi_ffa_bwd_dkv_direct(const magi_ffa_bwd_direct_args* args);
int magi_ffa_bwd_dv_direct(const magi_ffa_bwd_direct_args* args);
int magi_ffa_bwd_dk_direct(const magi_ffa_bwd_direct_args* args);
int magi_ffa_bwd_direct_args_size(void);

/* cat_gqa (reference flex_flash_attn_func cat_gqa: "concatenate the Q heads
 * sharing one KV head to optimise the backward under GQA"). magi_ffa_bwd_dkv,
 * _dv and _dk run one workgroup per (k range, q head, k block), so under GQA
 * the hq / hk heads of a group each stage the same K/V tiles and all add into
 * the same dK/dV rows. The entries below take the direct struct embedded
 * first (a pointer to the new one passes to the older entries) and one more
 * switch:
 *   cat_gqa   0: exactly the _direct entry of the same pass, its codes -11
 *             and -12 included; reserved is not read.
 *             1: one workgroup per (k range, KV head, k block). It stages its
 *             K/V tiles once, walks the hq / hk q heads of its group - q
 *             segments in table order, within a segment q heads ascending -
 *             into one register tile, and runs the epilogue once. With
 *             disjoint k ranges every dK/dV element then has a single owner
 *             for any hq % hk == 0, so dkv_is_16bit is accepted with
 *             hq != hk. With hq == hk this is the cat_gqa = 0 launch.
 *   reserved  must be 0.
 * Validation with cat_gqa = 1, in this order, all before any HIP call: -1,
 * -2, -3, -9 as above; with dkv_is_16bit set, -12 as above (-11 does not
 * apply); then -13 a deterministic GQA head split packed into cu_margin's top
 * 16 bits (the split launches each q head of a group on its own, cat_gqa
 * walks them in one workgroup: one or the other); -14 reserved != 0; then
 * n_ranges <= 0 returns 0 without a launch. The dq pass has no cat form: use
 * magi_ffa_bwd_dq_direct on &args->direct. */
typedef struct magi_ffa_bwd_cat_args {
  magi_ffa_bwd_direct_args direct;
  int32_t cat_gqa;
  int32_t reserved;
} magi_ffa_bwd_cat_args;

int magi_ffa_bwd_dkv_cat(const magi_ffa_bwd_cat_args* args);
int magi_ffa_bwd_dv_cat(const magi_ffa_bwd_cat_args* args);
int magi_ffa_bwd_dk_cat(const magi_ffa_bwd_cat_args* args);
int magi_ffa_bwd_cat_args_size(void);

/* ------------------------------------------------------------------ *
 * Range row ops (reference common/range_op/_range_*.py — Triton there,
 * hand-written HIP here; pack/unpack engine of the group collectives). *
 * ------------------------------------------------------------------ */

typedef struct magi_range_op_args {
  const void* input;        /* [T_in, row_elems] */
  void* output;             /* [T_out, row_elems] */
  const int32_t* in_ranges;   /* [n,2] rows of input  */
  const int32_t* out_starts;  /* [n]   start row in output for each range */
  const float* in_lse;      /* optional [T_in, h] (lse-weighted reduce) */
  float* out_lse;           /* optional [T_out, h] */
  int64_t n_ranges;
  int64_t row_elems;        /* elements per row (h*d) */
  int64_t total_rows;       /* total rows moved (sum of range lengths) */
  int32_t elem_size;        /* bytes per element: 1 (fp8/u8), 2 (bf16) or 4 (f32);
                               copies take any row byte count, sum needs f32 rows
                               of a multiple of 16 bytes (else rc -2) */
  int32_t n_heads;          /* for lse variant: row_elems = n_heads*d */
  int32_t reduce_op;        /* 0=copy(gather/scatter), 1=sum, 2=lse-weighted */
  void* stream;
} magi_range_op_args;

/* output[out_starts[i] + j] = input[in_ranges[i].start + j] (copy), or
 * output rows += / lse-merge input rows (reduce). */
int magi_range_gather(const magi_range_op_args* args);
int magi_range_reduce(const magi_range_op_args* args);

/* Attention-sink postprocess (reference flash_fwd_postprocess_kernel.h:39
 * FlashAttnFwdPostprocess / flash_bwd_preprocess_kernel.h dsink path):
 * value-less learnable logits folded into (out, lse) AFTER the (possibly
 * multi-slice, atomic-merged) forward, so they enter the softmax denominator
 * exactly once. Layouts: ssh=0 -> sink[s_sink, h]; ssh=1 -> sink[T, s_sink, h].
 */
typedef struct magi_sink_args {
  void* out;            /* [T, h, d] bf16 (out_is_fp32=0) or f32, in/out */
  float* lse;           /* [T, h], in/out (fwd) / in (bwd) */
  const float* sink;    /* sink logits, f32 */
  float* dsink;         /* same shape as sink, f32, zero-initialised (bwd) */
  const float* dpsum;   /* [T, h] (bwd) */
  int64_t total_rows;   /* T */
  int32_t n_heads;
  int32_t d;
  int32_t s_sink;       /* <= 8 */
  int32_t ssh;          /* 0 = "sh", 1 = "ssh" */
  int32_t out_is_fp32;
  void* stream;
} magi_sink_args;

/* fwd: lse_sink = log(sum_j exp(sink_j)); live rows: out *= exp(lse-lse'),
 * lse' = log(exp(lse)+exp(lse_sink)); empty rows (lse=-inf): out=0, lse=lse_sink. */
int magi_ffa_sink_postprocess(const magi_sink_args* args);
/* bwd: dsink_j (+)= -exp(sink_j - lse_row) * dpsum_row (summed over rows for
 * "sh", per row for "ssh"). */
int magi_ffa_dsink(const magi_sink_args* args);

/* Fused merge of two partial (out, lse) sets (reference functional/utils.py:371
 * correct_out_lse_kernel): out1/lse1 updated in place with out2/lse2 merged in. */
typedef struct magi_correct_args {
  void* out1;               /* f32 [T, h, d], in/out */
  float* lse1;              /* f32 [T, h], in/out */
  const void* out2;         /* f32 [T, h, d] */
  const float* lse2;        /* f32 [T, h] */
  int64_t total_rows;       /* T */
  int32_t n_heads;
  int32_t d;
  void* stream;
} magi_correct_args;

int magi_correct_out_lse(const magi_correct_args* args);

/* ------------------------------------------------------------------ *
 * magi_attn_ext surface helpers (reference csrc/extensions/)           *
 * ------------------------------------------------------------------ */

/* GPU spin barrier (reference extensions/kernel_barrier.cu:103): counter in
 * device memory; produce() increments from one stream, synchronize() launches
 * a 1-thread spin kernel on another stream that waits counter >= target. */
int magi_kernel_barrier_produce(int32_t* counter, void* stream);
int magi_kernel_barrier_synchronize(const int32_t* counter, int32_t target,
                                    void* stream);

/* native range utilities (reference csrc/extensions/
   sort_and_reorder_ranges.cu, unique_consecutive_pairs.cu): single-WG HIP
   kernels for the planner regime (N <= 8192); rc=2 => caller falls back */
int magi_argsort_ranges(const void* ranges, void* out_idx, int n,
                        void* stream);
int magi_reorder_ranges(const void* q_ranges, const void* k_ranges,
                        const void* attn_type_map, const void* order,
                        void* q_out, void* k_out, void* t_out, int n,
                        void* stream);
int magi_unique_pairs(const void* sorted_ranges, void* uniq, void* inverse,
                      void* count, int n, void* stream);

/* native grpcoll transport (HIP-IPC pull over xGMI; csrc/grpcoll.hip) */
int magi_ipc_get_handle(const void* dev_ptr, void* out_handle64);
int magi_ipc_open(const void* handle64, void** out_ptr);
int magi_ipc_close(void* ptr);
int magi_ipc_base(const void* dev_ptr, void** base, unsigned long long* size);
int magi_grpcoll_signal(void* flag_ptr, int value, void* stream);
int magi_grpcoll_wait(const void* flag_ptr, int value, void* stream);
int magi_grpcoll_ack(void* const* ack_ptrs, int n, void* stream);
struct magi_grpcoll_pull_args;
int magi_grpcoll_pull(const struct magi_grpcoll_pull_args* args);

/* Index-attention (token-gather) forward — the reference's
 * index_attn_indices direct-to-kernel path (flex_flash_attn.py:1358-1390).
 * indices_2d[i] lists the GLOBAL K rows attended by q token row i, shared
 * by all hq query heads of that row; -1 = contiguous tail padding. KV heads
 * are folded into the K row dimension (hk must be 1). The reference is
 * forward-only here; magi_ffa_bwd_index below adds the backward.
 *
 * Optional trailing fields (null / zero = off, and then out and lse are
 * bit-identical to a call without them):
 *   sink       f32 attention-sink logits folded into the kernel's epilogue in
 *              fp32, before the single rounding of out: with lse_sink =
 *              logsumexp_j sink[.., j, head], a live row stores lse' =
 *              logaddexp(lse, lse_sink) and out * exp(lse - lse'); a row whose
 *              list is all -1 stores lse = lse_sink and leaves out at the
 *              caller's zero. Layouts as magi_sink_args: sink_ssh=0 ->
 *              sink[s_sink, hq]; sink_ssh=1 -> sink[total_q, s_sink, hq].
 *   max_logits f32 [hq], caller-initialised to -inf: per-head atomic max over
 *              all tokens of the scaled (softcapped, if on) logits of valid
 *              slots. All-padding rows and sink logits do not enter it.
 * Validation, in this order, all before any HIP call: -1 null pointer, -2 d
 * not in {64, 128}, -3 hk != 1, -4 max_topk not a positive multiple of 64,
 * -5 sink != NULL with s_sink outside [1, 8]; then total_q <= 0 returns 0
 * without a launch. */
typedef struct magi_ffa_index_args {
  const void* q;              /* bf16 [total_q, hq, d] */
  const void* k;              /* bf16 [total_k, 1, d] */
  const void* v;              /* bf16 [total_k, 1, d] */
  void* out;                  /* bf16 or f32 [total_q, hq, d], zero-init */
  float* lse;                 /* f32 [total_q, hq], caller-initialised -inf */
  const int32_t* indices_2d;  /* [total_q, max_topk] global K row ids, -1 pad */
  int64_t total_q;
  int64_t total_k;
  int32_t max_topk;           /* multiple of 64 */
  int32_t hq;
  int32_t hk;                 /* must be 1 */
  int32_t d;                  /* 64 or 128 */
  float softmax_scale;
  float softcap;
  int32_t out_is_fp32;
  void* stream;               /* hipStream_t */
  const float* sink;          /* f32 sink logits, NULL = no sink */
  int32_t s_sink;             /* 1..8 when sink != NULL */
  int32_t sink_ssh;           /* 0 = "sh" [s_sink, hq], 1 = "ssh" [total_q, s_sink, hq] */
  float* max_logits;          /* f32 [hq] init -inf, NULL = off */
} magi_ffa_index_args;

int magi_ffa_fwd_index(const magi_ffa_index_args* args);

/* fp8 (OCP e4m3) index-attention forward (csrc/ffa_index_fp8.hip). Same args
 * struct, but for this entry q, k and v hold raw e4m3 BYTES (1 byte per
 * element, rows of d bytes, no descale factors); out is bf16 (or f32 with
 * out_is_fp32) and lse f32, zero / -inf initialised by the caller as above.
 * Numerics are the fp8 convention of magi_ffa_fwd_fp8 (P in [0, 256] packed
 * to e4m3, fp32 accumulate); softcap is supported. Validation order and
 * codes are those of magi_ffa_fwd_index, all returned before any HIP call:
 * -1 null pointer, -2 d not in {64, 128}, -3 hk != 1, -4 max_topk not a
 * positive multiple of 64, -5 sink != NULL with s_sink outside [1, 8];
 * total_q <= 0 or hq <= 0 returns 0 without a launch. sink and max_logits
 * behave as for magi_ffa_fwd_index; the sink is folded after the lse has left
 * the 2^8-offset domain of the fp8 running sum. */
int magi_ffa_fwd_index_fp8(const magi_ffa_index_args* args);

/* Index-attention backward (beyond the reference, whose autograd returns None
 * for index_attn): gathers K/V rows as the forward does, keeps dQ in
 * registers (single owner, stored once as bf16) and scatters dK/dV with fp32
 * atomic adds at row indices_2d[i][j] - padding and out-of-range slots issue
 * no atomic. Not deterministic (fp32 atomics reorder). dpsum must hold
 * rowsum(dO * O): run magi_ffa_bwd_preprocess first (it reads only
 * dout/out/dpsum/total_q/hq/d/out_is_fp32/stream of magi_ffa_bwd_args).
 * Validation codes mirror magi_ffa_fwd_index: -1 null pointer, -2 d not in
 * {64, 128}, -3 hk != 1, -4 max_topk not a positive multiple of 64;
 * total_q <= 0 returns 0 without a launch. */
typedef struct magi_ffa_index_bwd_args {
  const void* dout;           /* bf16 [total_q, hq, d] */
  const void* q;              /* bf16 [total_q, hq, d] */
  const void* k;              /* bf16 [total_k, 1, d] */
  const void* v;              /* bf16 [total_k, 1, d] */
  const float* lse;           /* f32 [total_q, hq] (forward output) */
  const float* dpsum;         /* f32 [total_q, hq] = rowsum(dO * O) */
  const int32_t* indices_2d;  /* [total_q, max_topk] global K row ids, -1 pad */
  void* dq;                   /* bf16 [total_q, hq, d], zero-init, plain stores */
  float* dk;                  /* f32 [total_k, 1, d], zeroed, atomic-accumulated */
  float* dv;                  /* f32 [total_k, 1, d], zeroed, atomic-accumulated */
  int64_t total_q;
  int64_t total_k;
  int32_t max_topk;           /* multiple of 64 */
  int32_t hq;
  int32_t hk;                 /* must be 1 */
  int32_t d;                  /* 64 or 128 */
  float softmax_scale;
  float softcap;
  void* stream;               /* hipStream_t */
} magi_ffa_index_bwd_args;

int magi_ffa_bwd_index(const magi_ffa_index_bwd_args* args);

/* Version/identity probe so tests can verify the native library is loaded. */
int magi_ffa_abi_version(void);

/* sizeof of a public args struct as the library was compiled, for a binding
 * to check its own mirror against before it passes one in (a mismatch would
 * make a kernel read garbage pointers). which: 0 magi_ffa_fwd_args,
 * 1 magi_ffa_bwd_args, 2 magi_range_op_args, 3 magi_sink_args,
 * 4 magi_correct_args, 5 magi_ffa_index_args, 6 magi_ffa_index_bwd_args;
 * anything else returns -1. */
int magi_ffa_args_size(int which);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MAGI_FFA_H */
