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

/* Dense fp8 forward: q/k/v are raw e4m3 bytes, no descale factors; P is
 * scaled to [0, 256] and packed to e4m3, accumulation is fp32.
 * magi_ffa_fwd_fp8 is the plain launch: f32 out in merge mode, one k range per
 * q range, no softcap. It returns -6 for a 16-bit out or
 * disable_atomic_reduction and -7 for softcap != 0 or qk_starts != NULL.
 * magi_ffa_fwd_fp8_flex takes the same struct with every member in its
 * meaning for magi_ffa_fwd (elem_type and cu_margin are not read):
 *   softcap > 0       score = softcap * tanh(s * scale / softcap); max_logits
 *                     then holds the softcapped value. 0 = off.
 *   qk_starts         merged tables: the workgroup of a unique q range walks
 *                     its k segments in table order and runs one epilogue.
 *                     Segments may overlap, repeat (a key listed twice counts
 *                     twice), be empty, or come in any k order. A q block
 *                     that no segment gives a key leaves out and lse alone.
 *   disable_atomic_reduction = 1
 *                     the (unique) q ranges are disjoint: no locks, no read
 *                     of the previous out / lse, one store per element - bf16
 *                     rounded to nearest even with out_is_fp32 = 0, f32 with
 *                     out_is_fp32 = 1. Rows with no key are not written
 *                     (caller presets out = 0, lse = -inf). locks may be NULL.
 * With softcap = 0, qk_starts = NULL and merge mode it is magi_ffa_fwd_fp8's
 * launch, bit for bit. Validation of the flex entry, in this order, all
 * before any pointer is touched: -1 null struct or q/k/v/out/lse, -2 d not in
 * {64, 128}, -3 hq % hk != 0, -6 out_is_fp32 == 0 without
 * disable_atomic_reduction, -7 softcap < 0; then n_ranges <= 0 returns 0
 * without a launch; -4 merge mode without locks, -5 more than 65535 ranges. */
int magi_ffa_fwd_fp8(const magi_ffa_fwd_args* args);
int magi_ffa_fwd_fp8_flex(const magi_ffa_fwd_args* args);

/* pack_gqa (reference flex_flash_attn_func pack_gqa: "pack the Q heads that
 * share one KV head into one q tile"). magi_ffa_fwd runs one workgroup per
 * (q range, q head, block of q rows), a wave owning 32 consecutive tokens of
 * one head: on block-sparse and short-document masks, where q ranges are
 * short, most of each wave is empty and the hq / hk heads of a group each
 * stage the same K/V rows. magi_ffa_fwd_args keeps its size and its last
 * member (bindings check both), so the switch rides behind an embedded copy:
 *   pack_gqa  0: exactly magi_ffa_fwd(&args), bit for bit; reserved is not
 *             read.
 *             1: one workgroup per (q range, KV head, block of packed rows).
 *             With G = hq / hk (any value, a power of two or not), q range
 *             [qs, qe) has (qe - qs) * G packed rows; row r is token
 *             qs + r / G, q head kh * G + r % G. K/V is staged once per
 *             workgroup for all G heads. out, lse and max_logits have the
 *             usual layout and meaning; every member of args keeps its
 *             meaning (qk_starts, softcap, both element types, d = 64 / 128 /
 *             192, merge / direct 16-bit / direct f32 out, max_logits,
 *             cu_margin). In merge mode a workgroup takes the locks of all G
 *             heads, ordered so that packed and unpacked launches may
 *             accumulate into one out. Results are within rounding of
 *             magi_ffa_fwd's, not bit-equal: packing changes which rows share
 *             a wave, and the deferred-max decision is per wave. With
 *             hq == hk this is the pack_gqa = 0 launch. The launcher takes 4
 *             waves when max_seqlen_q * G <= 128 and 8 otherwise (d = 192:
 *             always 4); MAGI_FWD_WAVES overrides as for magi_ffa_fwd,
 *             MAGI_FWD_NBUF is not read (each width runs its default ring).
 *   reserved  must be 0.
 * Validation with pack_gqa = 1, in this order, all before any HIP call: -1
 * null pointer, -2 head dim, -3 hq % hk != 0, -9 elem_type, -14 reserved != 0;
 * then n_ranges <= 0 returns 0 without a launch; -4 merge mode without locks,
 * -5 more than 65535 ranges, -10 merge mode into a 16-bit out. There is no
 * fp8 pack entry. magi_ffa_fwd_pack_args_size is sizeof of the struct as
 * compiled (magi_ffa_args_size keeps its list). */
typedef struct magi_ffa_fwd_pack_args {
  magi_ffa_fwd_args args;
  int32_t pack_gqa;
  int32_t reserved;         /* must be 0 */
} magi_ffa_fwd_pack_args;

int magi_ffa_fwd_pack(const magi_ffa_fwd_pack_args* args);
int magi_ffa_fwd_pack_args_size(void);

/* sparse_load (reference flex_flash_attn_func sparse_load: "k_range size is
 * small (< 64)", to be used with auto_range_merge). Under qk_starts the
 * forward serves a unique q range's k segments one after another, each with
 * whole 64-row K/V stages of its own, a ring restart, a drain and a barrier:
 * with k blocks of 16 or 32 rows most of every stage and MFMA tile is
 * padding. The switch rides behind an embedded copy of the pack struct, as
 * pack_gqa rides behind magi_ffa_fwd_args:
 *   sparse_load 0: exactly magi_ffa_fwd_pack(&pack), bit for bit; k_cum and
 *             reserved are not read.
 *             1: the k rows of unique q range ri are one virtual axis, the
 *             segments k_ranges[qk_starts[ri] .. qk_starts[ri + 1]) laid end
 *             to end in table order: L = sum of (ke - ks) rows. Empty
 *             segments add nothing, segments may come in any k order and
 *             length (1 included), and a segment listed twice counts twice,
 *             as it does with sparse_load = 0. The k loop stages 64 virtual
 *             rows at a time through a row map the workgroup keeps in LDS
 *             (2048 rows; longer axes are walked in chunks), so every K/V
 *             stage and every MFMA tile but a chunk's last is full.
 *             Every segment is a full block (type 0): attn_type_map is NOT
 *             read, and the caller vouches for it as it does for disjoint
 *             ranges. qk_starts is required. A range with L = 0 leaves out
 *             and lse untouched. out, lse and max_logits have the usual
 *             layout and meaning and are within rounding of the
 *             sparse_load = 0 result, not bit-equal (the tile composition
 *             changes). pack.pack_gqa, softcap, both element types, merge /
 *             direct 16-bit / direct f32 out, max_logits and cu_margin
 *             compose with it. Built for d = 64 and 128; d = 192 runs the
 *             sparse_load = 0 launch (k_cum unread) and is not an error. The
 *             launcher takes 4 waves when the longest q range has at most
 *             128 (packed) rows and 8 otherwise; MAGI_FWD_WAVES overrides,
 *             MAGI_FWD_NBUF is not read.
 *   k_cum     int32 [n_segments + 1], n_segments = qk_starts[n_ranges]:
 *             k_cum[0] = 0, k_cum[s + 1] = k_cum[s] + max(ke_s - ks_s, 0)
 *             over k_ranges (a device cumsum; no host sync). A k_cum that
 *             disagrees with k_ranges gives wrong results; mapped rows are
 *             clamped to [0, total_k).
 *   reserved  must be 0, like pack.reserved.
 * Validation with sparse_load = 1, in this order, all before any HIP call:
 * -1 null pointer, -2 head dim, -3 hq % hk != 0, -9 elem_type, -14 reserved
 * or pack.reserved != 0, -15 qk_starts == NULL, -1 k_cum == NULL; then
 * n_ranges <= 0 returns 0 without a launch; -4 merge mode without locks, -5
 * more than 65535 ranges, -10 merge mode into a 16-bit out. There is no fp8
 * sparse entry. magi_ffa_fwd_sparse_args_size is sizeof of the struct as
 * compiled. */
typedef struct magi_ffa_fwd_sparse_args {
  magi_ffa_fwd_pack_args pack;
  const int32_t* k_cum;
  int32_t sparse_load;
  int32_t reserved;         /* must be 0 */
} magi_ffa_fwd_sparse_args;

int magi_ffa_fwd_sparse(const magi_ffa_fwd_sparse_args* args);
int magi_ffa_fwd_sparse_args_size(void);

/* swap_ab (reference flex_flash_attn_func swap_ab: fill the matrix units when
 * q blocks are small, 8 to 64 rows). In magi_ffa_fwd a wave owns 32 q rows and
 * a workgroup 32 * waves rows of ONE q range, so a range of 32 rows or fewer
 * has one computing wave per workgroup. pack_gqa fills the rest with the
 * group's heads; with hq == hk there is no group. This entry fills it with
 * the k loop. The switch rides behind an embedded copy, as pack_gqa does:
 *   swap_ab   0: exactly magi_ffa_fwd(&args), bit for bit; reserved is not
 *             read.
 *             1: the split-k forward. A 4-wave workgroup owns QT q tiles of 32
 *             rows of a range (QT = 2; MAGI_FWD_SPLITK_QT = 1 | 2 overrides for
 *             the A/B, both are correct for any range length; QT = 1 measured
 *             slower even on 16-row ranges). The KS = 4 / QT waves of a tile split every
 *             staged K/V image of 32 * KS rows between them, 32 rows each,
 *             keep a softmax state each and merge the states once per
 *             (unique) q range, in LDS, in ascending wave order: the result
 *             repeats run to run. out, lse and max_logits have the usual
 *             layout and meaning and are within rounding of magi_ffa_fwd's,
 *             not bit-equal (the summation order over k differs). Every
 *             member of args keeps its meaning: qk_starts (the states are
 *             carried across a range's k segments), all four mask types,
 *             softcap, both element types, GQA (kh = h / (hq / hk), unpacked),
 *             merge / direct 16-bit / direct f32 out, max_logits, cu_margin.
 *             Built for d = 64 and 128; d = 192 runs the swap_ab = 0 launch
 *             and is not an error. MAGI_FWD_WAVES and MAGI_FWD_NBUF are not
 *             read (4 waves, a 2-slot ring); MAGI_FWD_HEADMAJOR is.
 *   reserved  must be 0.
 * Validation with swap_ab = 1, in this order, all before any HIP call: -1
 * null pointer, -2 head dim, -3 hq % hk != 0, -9 elem_type, -14 reserved != 0;
 * then n_ranges <= 0 returns 0 without a launch; -4 merge mode without locks,
 * -5 more than 65535 ranges, -10 merge mode into a 16-bit out. There is no
 * fp8, pack_gqa or sparse_load combination. magi_ffa_fwd_splitk_args_size is
 * sizeof of the struct as compiled. */
typedef struct magi_ffa_fwd_splitk_args {
  magi_ffa_fwd_args args;
  int32_t swap_ab;
  int32_t reserved;         /* must be 0 */
} magi_ffa_fwd_splitk_args;

int magi_ffa_fwd_splitk(const magi_ffa_fwd_splitk_args* args);
int magi_ffa_fwd_splitk_args_size(void);

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

/* sparse_load for the dq pass (the backward twin of magi_ffa_fwd_sparse).
 * Under seg_starts magi_ffa_bwd_dq serves a unique q range's k segments one
 * after another, each with whole 64-row K/V stages of its own, a ring
 * restart, a drain and a barrier: with k blocks of 16 or 32 rows most of every
 * stage and MFMA tile is padding. The switch rides behind an embedded copy of
 * the cat struct (a pointer to the new one passes to the older entries; the
 * dkv / dv / dk passes take &args->cat and know nothing of the new members):
 *   sparse_load 0: exactly magi_ffa_bwd_dq_direct(&cat.direct), bit for bit;
 *             k_cum and reserved are not read.
 *             1: the k rows of unique q range ri are one virtual axis, the
 *             segments k_ranges[seg_starts[ri] .. seg_starts[ri + 1]) laid
 *             end to end in table order: L = sum of (ke - ks) rows. Empty
 *             segments add nothing, segments may come in any k order and
 *             length (1 included), and a segment listed twice counts twice,
 *             as it does with sparse_load = 0. The k loop stages 64 virtual
 *             rows at a time through a row map the workgroup keeps in LDS
 *             (2048 rows; longer axes are walked in chunks), so every K/V
 *             stage and every MFMA tile but a chunk's last is full.
 *             Every segment is a full block (type 0): attn_type_map is NOT
 *             read, and the caller vouches for it as it does for disjoint
 *             ranges. seg_starts is required. A range with L = 0 leaves its
 *             dq rows untouched. dq has the usual layout and meaning and is
 *             within rounding of the sparse_load = 0 result, not bit-equal
 *             (the tile composition changes). cat.direct.dq_is_16bit,
 *             softcap, both element types, GQA and cu_margin compose with
 *             it; cat.cat_gqa and cat.reserved belong to the dkv passes and
 *             are not read. Built for d = 64 and 128; d = 192 runs the
 *             sparse_load = 0 launch (k_cum unread) and is not an error. The
 *             launcher picks 4 or 8 waves as magi_ffa_bwd_dq does
 *             (max_seqlen_k against MAGI_BWD_DQ_BIGSEQ).
 *   k_cum     int32 [n_segments + 1], n_segments = seg_starts[n_ranges], as
 *             magi_ffa_fwd_sparse_args.k_cum: k_cum[0] = 0, k_cum[s + 1] =
 *             k_cum[s] + max(ke_s - ks_s, 0) over k_ranges (a device cumsum;
 *             no host sync). A k_cum that disagrees with k_ranges gives wrong
 *             results; mapped rows are clamped to [0, total_k).
 *   reserved  must be 0.
 * Validation with sparse_load = 1, in this order, all before any HIP call:
 * -1 null pointer, -2 head dim, -3 hq % hk != 0, -9 elem_type, -14 reserved
 * != 0, -15 seg_starts == NULL, -1 k_cum == NULL; then n_ranges <= 0 returns
 * 0 without a launch; -5 more than 65535 ranges.
 * magi_ffa_bwd_sparse_args_size is sizeof of the struct as compiled. */
typedef struct magi_ffa_bwd_sparse_args {
  magi_ffa_bwd_cat_args cat;
  const int32_t* k_cum;     /* int32 [n_segments + 1], as magi_ffa_fwd_sparse */
  int32_t sparse_load;
  int32_t reserved;         /* must be 0 */
} magi_ffa_bwd_sparse_args;

int magi_ffa_bwd_dq_sparse(const magi_ffa_bwd_sparse_args* args);
int magi_ffa_bwd_sparse_args_size(void);

/* swap_bwd_qk_loop (reference flex_flash_attn_func: "Q for outer-loop and K
 * for inner-loop" in the backward): ONE q-outer pass in place of the dq pass
 * and the dkv pass. A workgroup owns what a dq workgroup owns, (q range - the
 * unique one under seg_starts -, q head, block of 128 q rows), walks the k
 * segments of that unit once and produces all three gradients: S and dP are
 * recomputed once per tile (5 matmuls where the two passes spend 3 + 4), dQ
 * stays in registers and is stored once, and dK / dV go out with one f32
 * atomic add per non-zero element and 32-row k tile, reduced over the 128 q
 * rows of the workgroup first, into row k and KV head h / (hq / hk). Needs
 * dpsum filled (magi_ffa_bwd_preprocess).
 *   args.dq          zeroed f32, or with dq_is_16bit a zeroed elem_type buffer
 *                    stored directly (disjoint q ranges), as in
 *                    magi_ffa_bwd_dq_direct.
 *   args.dk, dv      zeroed f32 accumulators: dkv_is_16bit must be 0. Several
 *                    workgroups add into one row, whatever the ranges are.
 *   args.seg_starts  optional: NULL = one k segment per q range (the flat
 *                    table), else the dq pass's merged table.
 *   attn_type_map    is read, all four types; softcap, both element types,
 *                    GQA and cu_margin's low 16 bits (the strided grid) apply
 *                    as in the dq pass. k rows and q rows in no range keep the
 *                    caller's zeros. Results agree with the two passes within
 *                    rounding, not bit for bit; f32 atomics reorder, so there
 *                    is no deterministic mode.
 * Built for d = 64 and 128; any other head dim is an error here (the caller
 * falls back to the two passes). Validation, in this order, all before any
 * HIP call: -1 null struct or null dout / q / k / v / lse / dq / dk / dv /
 * dpsum, -2 head dim not 64 or 128, -3 hk <= 0 or hq % hk != 0, -9 elem_type,
 * -12 a deterministic GQA head split packed into cu_margin's top 16 bits, -16
 * dkv_is_16bit != 0; then n_ranges <= 0 returns 0 without a launch; -5 more
 * than 65535 ranges. */
int magi_ffa_bwd_qloop(const magi_ffa_bwd_direct_args* args);

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

/* q_block_size on the index path (the reference declares it on
 * flex_flash_attn_func): one index row per block of q_block_size q token
 * rows. Rows [b*B, min((b+1)*B, total_q)) of q, with all their hq heads,
 * attend the K rows listed in indices_2d[b], so indices_2d is
 * [ceil(total_q / B), max_topk] for these entries (the last block may be
 * partial); -1 tail padding, 64 | max_topk, hk == 1 and global row ids are as
 * above. With KV heads folded into q rows, arranging rows so that a block
 * belongs to one KV head is the caller's business. The switch rides behind an
 * embedded copy of the base struct, as pack_gqa rides behind
 * magi_ffa_fwd_args; the base entries and their kernels are untouched.
 *
 * The kernels are BLOCK instantiations of ffa_index.hip / ffa_index_bwd.hip:
 * q is [total_q, hq, d], so a block's B*hq (token, head) rows are one
 * contiguous slab of flat rows and take the place of the hq heads of a token -
 * a workgroup is (block, chunk of 32*W packed rows), W from B*hq as the base
 * entries take it from hq (4 waves above 64 rows, 2 above 32, else 1). The
 * MFMA tiles fill with B*hq rows, K/V are gathered once per workgroup and not
 * once per token, and the backward issues one dK/dV atomic per (workgroup,
 * gathered row) for all the tokens of the chunk. A block whose list is all -1
 * leaves out at 0 and writes lse = lse_sink for its live rows with a sink,
 * else leaves -inf. sink (sink_ssh 0 and 1, by the row's own token and head),
 * max_logits ([hq], by the row's head), softcap and out_is_fp32 act as in the
 * base entries; magi_ffa_bwd_preprocess and magi_ffa_dsink are row-wise and
 * serve both. Results agree with the base entry over lists expanded to one per
 * token within rounding, not bit for bit: packing changes which rows share a
 * wave, and the deferred-max decision is per wave. q_block_size = 1 computes
 * what the base entry computes, through the BLOCK kernels; a q_block_size
 * beyond total_q is one block.
 *   reserved  not read.
 * Validation is the base entry's, same order and codes, all before any HIP
 * call, then the next code for q_block_size < 1: -6 for
 * magi_ffa_fwd_index_block (after -1 .. -5), -5 for magi_ffa_bwd_index_block
 * (after -1 .. -4); then total_q <= 0 returns 0 without a launch. A null
 * struct is -1. There is no fp8 block entry. The *_args_size functions return
 * sizeof of the structs as compiled (magi_ffa_args_size keeps its list). */
typedef struct magi_ffa_index_block_args {
  magi_ffa_index_args args;   /* indices_2d: [ceil(total_q / B), max_topk] */
  int32_t q_block_size;       /* B >= 1 */
  int32_t reserved;
} magi_ffa_index_block_args;

int magi_ffa_fwd_index_block(const magi_ffa_index_block_args* args);
int magi_ffa_fwd_index_block_args_size(void);

typedef struct magi_ffa_index_bwd_block_args {
  magi_ffa_index_bwd_args args;
  int32_t q_block_size;       /* B >= 1 */
  int32_t reserved;
} magi_ffa_index_bwd_block_args;

int magi_ffa_bwd_index_block(const magi_ffa_index_bwd_block_args* args);
int magi_ffa_bwd_index_block_args_size(void);

/* k_block_size on the index path (the reference declares it and leaves it
 * unimplemented): list entries are K BLOCK ids. With Bk = k_block_size, id j
 * stands for rows [j*Bk, min((j+1)*Bk, total_k)) of k / v as passed
 * ([total_k, 1, d], hk == 1); -1 is contiguous tail padding as above. When
 * total_k % Bk != 0 the last block is short; it may sit anywhere in a list and
 * its missing rows contribute nothing (no logit, no max_logits, no atomic). An
 * id outside [0, ceil(total_k / Bk)) is handled like an out-of-range row id of
 * the base entries: loads are clamped, the entry is masked. With KV heads
 * folded into the row dimension a block is Bk consecutive rows of the tensor;
 * laying rows out so that a block belongs to one KV head is the caller's
 * business. Shapes of indices_2d are those of the embedded entry:
 * [ceil(total_q / q_block_size), max_topk].
 *
 * The kernels are KBLOCK instantiations of ffa_index.hip, ffa_index_fp8.hip
 * and ffa_index_bwd.hip: their k loop runs over row positions
 * 0 .. count_blocks*Bk, position pos -> list slot pos / Bk, row id*Bk +
 * pos % Bk; nothing is expanded on the host or into a buffer. Where a staged
 * group of rows lies inside one block the id is read once per wave and lane
 * addresses are base + offset. Results agree with the embedded entry over
 * lists expanded to row ids within rounding, not bit for bit.
 *   q_block_size  (bf16 entries) as in magi_ffa_index_block_args; 1 runs the
 *                 per-token kernels' KBLOCK build, > 1 the BLOCK ones'.
 *   k_block_size  Bk, a power of two >= 2.
 *   reserved      not read.
 * Validation is the embedded entry's, same order and codes, all before any
 * HIP call, with two changes: -4 is max_topk <= 0 or (max_topk * Bk) % 64 != 0
 * (so Bk = 64 allows any max_topk; a bad Bk is judged as 1 here), and the next
 * free code is returned for k_block_size not a power of two >= 2 or
 * max_topk * Bk not fitting int32: -7 for magi_ffa_fwd_index_kblock (after
 * -1 .. -6), -6 for magi_ffa_fwd_index_fp8_kblock (after -1 .. -5; it embeds
 * the base struct and has no q_block_size: there is no fp8 q-block kernel),
 * -6 for magi_ffa_bwd_index_kblock (after -1 .. -5). Then total_q <= 0
 * returns 0 without a launch. A null struct is -1. */
typedef struct magi_ffa_index_kblock_args {
  magi_ffa_index_block_args block;  /* indices_2d entries: K block ids */
  int32_t k_block_size;             /* Bk: power of two >= 2 */
  int32_t reserved;
} magi_ffa_index_kblock_args;

int magi_ffa_fwd_index_kblock(const magi_ffa_index_kblock_args* args);
int magi_ffa_fwd_index_kblock_args_size(void);

typedef struct magi_ffa_index_fp8_kblock_args {
  magi_ffa_index_args args;         /* q, k, v: raw e4m3 bytes */
  int32_t k_block_size;             /* Bk: power of two >= 2 */
  int32_t reserved;
} magi_ffa_index_fp8_kblock_args;

int magi_ffa_fwd_index_fp8_kblock(const magi_ffa_index_fp8_kblock_args* args);
int magi_ffa_fwd_index_fp8_kblock_args_size(void);

typedef struct magi_ffa_index_bwd_kblock_args {
  magi_ffa_index_bwd_block_args block;
  int32_t k_block_size;             /* Bk: power of two >= 2 */
  int32_t reserved;
} magi_ffa_index_bwd_kblock_args;

int magi_ffa_bwd_index_kblock(const magi_ffa_index_bwd_kblock_args* args);
int magi_ffa_bwd_index_kblock_args_size(void);

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
