// ffa_bwd_common.h — what the dense backward translation units share
// (ffa_bwd.hip: the dQ and dK/dV passes; ffa_bwd_qloop.hip: the one-pass
// q-outer kernel): tile sizes, the kernel argument struct, and the host side
// that validates a magi_ffa_bwd_args, fills the struct and caps a grid. The
// host functions are static: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/magi_ffa.h"
#include "ffa_device.h"

#define BWD_BN 32    // k rows per wave
#define BWD_BM 32    // q rows per tile

DEV_INLINE bool wave_alive(int m0, int qe) { return m0 < qe; }

// ET: element type of dout/q/k/v and of a 16-bit out, bf16_t or f16_t
// (ElemTraits, ffa_device.h); P and dS are rounded to ET before their MFMAs
template <class ET>
struct BwdParams {
  const ET* dout;
  const ET* q;
  const ET* k;
  const ET* v;
  const void* out;
  const float* lse;
  void* dq;   // f32 (atomic epilogue) or ET (direct epilogue), as dk and dv
  void* dk;
  void* dv;
  float* dpsum;
  const int* q_ranges;
  const int* k_ranges;
  const int* attn_type_map;
  int hq, hk, gqa;
  float scale;
  float softcap;
  int cat;           // q heads one dkv workgroup walks: 1, or gqa (cat_gqa);
                     // here it takes the padding in front of total_q and
                     // moves no other member
  long long total_q, total_k;
  int head_major;    // 1: blockIdx.x = head (XCD-affine); 0: work-major
  int work_nx, work_ny, work_nz;  // flattened work space (strided-grid mode)
  int head_mult;     // deterministic GQA split: real head = off + idx*mult
  int head_off;
  int n_heads_launch;
  const int* seg_starts;  // auto_range_merge: dq pass: ri = unique q range,
                          // k segments; dkv pass: ri = unique k range, q
                          // segments (reference bwd_kq_map). NULL = 1:1.
};

// ---------------- host side ----------------
// Every entry is a template over the element type behind one extern "C"
// function that picks the instantiation from args->elem_type.
#define BY_ELEM_TYPE(a, fn, ...)                                       \
  ((a) && (a)->elem_type == MAGI_FFA_ELEM_FP16 ? fn<f16_t>(a, ##__VA_ARGS__) \
                                               : fn<bf16_t>(a, ##__VA_ARGS__))

// What the _direct and _cat entries add to a dkv pass over magi_ffa_bwd_args
struct DkvOpts {
  bool direct;   // dkv_is_16bit: the direct-store epilogue
  bool cat;      // cat_gqa: one workgroup walks the q heads of a kv head
  int reserved;  // magi_ffa_bwd_cat_args.reserved, 0 from the other entries
};

// Validation shared by the dq and dkv entries, in the order magi_ffa.h
// documents; no HIP call before it. o.direct adds the rules of the direct
// dK/dV store, which has no other head or launch adding into its rows: that
// is hq == hk, or cat_gqa, whose workgroup is the only one of its kv head.
static int check_bwd_args(const magi_ffa_bwd_args* a, const DkvOpts& o) {
  if (!a || !a->dout || !a->q || !a->k || !a->v || !a->lse) return -1;
  if (a->d != 64 && a->d != 128 && a->d != 192) return -2;
  if (a->hq % a->hk != 0) return -3;
  if (!elem_type_known(a->elem_type)) return -9;
  if (o.direct) {
    if (a->hq != a->hk && !o.cat) return -11;
    if (a->cu_margin & 0xFFFF0000) return -12;
  }
  if (o.cat) {
    // the head split gives each q head of a group a launch of its own;
    // cat_gqa walks them in one workgroup
    if (a->cu_margin & 0xFFFF0000) return -13;
    if (o.reserved != 0) return -14;
  }
  return 0;
}

template <class ET>
static int fill_bwd_params(const magi_ffa_bwd_args* a, BwdParams<ET>* p,
                           const DkvOpts& o) {
  if (const int rc = check_bwd_args(a, o)) return rc;
  if (a->n_ranges <= 0) return 1;  // caller treats >0 as "nothing to do"
  p->dout = (const ET*)a->dout;
  p->q = (const ET*)a->q;
  p->k = (const ET*)a->k;
  p->v = (const ET*)a->v;
  p->out = a->out;
  p->lse = a->lse;
  p->dq = a->dq;
  p->dk = a->dk;
  p->dv = a->dv;
  p->dpsum = a->dpsum;
  p->q_ranges = a->q_ranges;
  p->k_ranges = a->k_ranges;
  p->attn_type_map = a->attn_type_map;
  p->hq = a->hq;
  p->hk = a->hk;
  p->gqa = a->hq / a->hk;
  // cat_gqa over a group of one head is the plain kernel
  p->cat = (o.cat && p->gqa > 1) ? p->gqa : 1;
  p->scale = a->softmax_scale;
  p->softcap = a->softcap;
  p->total_q = a->total_q;
  p->total_k = a->total_k;
  p->seg_starts = a->seg_starts;
  // deterministic-mode GQA split: cu_margin's top bits carry (mult<<8)|off;
  // 0 = all heads in one launch (default)
  p->head_mult = 1;
  p->head_off = 0;
  p->n_heads_launch = a->hq;
  if (a->cu_margin & 0xFFFF0000) {
    p->head_mult = (a->cu_margin >> 24) & 0xFF;
    p->head_off = (a->cu_margin >> 16) & 0xFF;
    p->n_heads_launch = a->hq / p->head_mult;
  }
  if (p->cat > 1) p->n_heads_launch = a->hk;  // the head index is the kv head
  return 0;
}

// A/B knobs are read at EVERY launch: the head-major A/B scripts
// (tests/gpu_headmajor_ab*.py) toggle them inside one process.
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// CU-margin (see ffa_fwd.hip): cap the grid below the resident-WG count;
// each WG then walks the flattened work space p.work_n*.
static dim3 cap_grid(dim3 grid, int margin, int wg_per_cu) {
  if (margin <= 0) return grid;
  const long long total = (long long)grid.x * grid.y * grid.z;
  long long cap = (long long)(256 - margin) * wg_per_cu;
  if (cap < 1) cap = 1;
  if (cap > total) cap = total;
  return dim3((unsigned)cap, 1, 1);
}

struct BwdKnobs {
  int head_major;  // grid order: 1 = blockIdx.x is the head
  int bigseq;      // k range length from which 8 waves run
};

static BwdKnobs dq_knobs(const magi_ffa_bwd_args* a) {
  // head-major pays when one head's K+V (bf16) fits a 4 MB XCD L2
  // late-r2 A/B (profiles/r2_headmajor_ab.md): dq wins head-major up to
  // ~16 MB of per-head K+V (1.20x at 16k) and loses beyond (0.93x at 64k,
  // 0.91x at 128k) — same shape as the fwd kernel.
  const int hm = ((long long)a->total_k * a->d * 4 <= (16 << 20)) ? 1 : 0;
  // 8 waves share one staged K/V image (one 512-thread WG/CU, 2 waves/SIMD)
  // for LONG ranges: halves staging+barrier cost per MFMA (measured
  // 67->63 ms at 64k). Short ranges keep 4 waves — dq's q-outer 256-row
  // blocks over-iterate masked causal k windows on 2k varlen docs (r2 A/B:
  // 0.79 -> 1.61 ms at W8).
  return {env_int("MAGI_BWD_HEAD_MAJOR", hm),
          env_int("MAGI_BWD_DQ_BIGSEQ", 8192)};
}
