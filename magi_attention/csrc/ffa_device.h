// ffa_device.h — code shared by the FFA kernels (gfx950, wave64); the device
// helpers are force-inlined. Sections, with the files that use them:
//   pipeline    pipe_barrier, glds16_untracked, drain_vm, pin_vgpr
//               (ffa_fwd, ffa_bwd)
//   lanes       warp_xor32 (all kernels)
//   index rows  index_valid_count (index forwards and backward),
//               index_sink_lse, index_sink_fold, head_atomic_max
//               (ffa_index, ffa_index_fp8)
//   fragments   pack_bf16_pair, fast_exp2, crow, tr16_frag, cframe_to_afrag
//               (the bf16 kernels), to_fp8, cframe_to_afrag_fp8 (the fp8 ones)
//   softmax     FP8_MAX_OFFSET, softmax_step_fp8 (ffa_fwd_fp8, ffa_index_fp8)
//   index host  IdxFwdParams<T>, index_fwd_entry: the one host path of
//               magi_ffa_fwd_index and magi_ffa_fwd_index_fp8
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/magi_ffa.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16_t = __bf16;

#define DEV_INLINE __device__ __forceinline__

// Software-pipelined LDS-DMA barrier: waits until at most VM vector-memory
// ops are outstanding (= exactly the NEXT prefetch group, leaving the current
// tile's group retired), makes LDS reads visible, then syncs the block.
// vmcnt retires in issue order, so a constant distance works as long as every
// iteration issues the same number of vector-memory ops and the loop issues
// NO other vector-memory ops — the staging lambdas are therefore called
// unconditionally with clamped addresses past the end.
// __syncthreads() would insert s_waitcnt vmcnt(0) and collapse the pipeline
// to depth one (measured: 34-42% SQ_WAIT in both backward kernels).
template <int VM>
DEV_INLINE void pipe_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier"
               :: "n"(VM) : "memory");
}

// 16-byte-per-lane LDS-DMA (global_load_lds_dwordx4) issued from inline asm,
// so the compiler's waitcnt pass does not track it. The builtin form leaves a
// "pending LDS write" on the VM counter in that pass, and it then puts
// `s_waitcnt vmcnt(0)` in front of the first ds_read_b64_tr_b16 that follows
// (the tr16 builtin is not marked read-only, so it is ordered against the
// DMA) — in a prefetch pipeline that drains the next tile's DMA in the
// middle of the compute phase meant to cover it. Callers own the ordering:
// the staged image may only be read after a pipe_barrier that retires it,
// and a kernel that restages or leaves LDS must drain with drain_vm() first —
// no compiler-placed wait covers these loads.
// lds_byte is the wave-uniform LDS byte address of the destination; lane l
// lands at lds_byte + 16 * l.
DEV_INLINE void glds16_untracked(const void* gsrc, int lds_byte) {
  const int m0v = __builtin_amdgcn_readfirstlane(lds_byte);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :: "s"(m0v), "v"(gsrc) : "memory", "m0");
}

// Explicit full drain of the vector-memory counter: the wait the compiler
// would have placed for tracked loads, owned by hand for the untracked ones.
DEV_INLINE void drain_vm() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Forces the compiler's own wait for whatever load produced x to this point
// (and keeps x in a VGPR): used to keep such waits out of a loop whose
// vmcnt distance is owned by hand.
template <class T>
DEV_INLINE void pin_vgpr(T& x) {
  asm volatile("" : "+v"(x));
}

DEV_INLINE float warp_xor32(float v) { return __shfl_xor(v, 32, 64); }

// ---- index rows ----

// Valid count of an index row (ffa_index.hip, ffa_index_fp8.hip,
// ffa_index_bwd.hip): the -1 padding is contiguous at the tail, so a
// wave-uniform binary search (same address every lane -> broadcast loads)
// finds it in log2(max_topk) dwords.
DEV_INLINE int index_valid_count(const int* irow, int max_topk) {
  int count = max_topk;
  if (irow[max_topk - 1] < 0) {
    int lo = 0, hic = max_topk - 1;
    while (lo < hic) {
      const int mid = (lo + hic) >> 1;
      if (irow[mid] < 0)
        hic = mid;
      else
        lo = mid + 1;
    }
    count = lo;
  }
  return count;
}

// ---- index-attention epilogue helpers (ffa_index.hip, ffa_index_fp8.hip) ----

// lse over the s_sink (1..8, checked by the host entry) attention-sink logits
// of (token, head), fp32 with the max subtracted — the arithmetic of
// sink_postprocess_kernel in range_ops.hip. Layouts of magi_sink_args:
// ssh = 0 -> sink[j * hq + head], ssh = 1 -> sink[(tok * s_sink + j) * hq +
// head]. The 8 predicated loads are unrolled so the logits stay in registers
// (a runtime-indexed array would go to scratch); an absent slot is -inf and
// adds an exact 0. All logits -inf gives -inf.
DEV_INLINE float index_sink_lse(const float* sink, int s_sink, int ssh,
                                long long tok, int hq, int head) {
  const float* sp = sink + (ssh ? tok * s_sink * (long long)hq : 0ll) + head;
  float sv[8];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sv[j] = (j < s_sink) ? sp[(long long)j * hq] : -INFINITY;
    mx = fmaxf(mx, sv[j]);
  }
  if (mx == -INFINITY) return -INFINITY;
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) l += expf(sv[j] - mx);
  return mx + logf(l);
}

// Folds lse_sink into a row's (lse, output scale): live row -> lse' =
// logaddexp(lse, lse_sink) and the output scale times exp(lse - lse'); empty
// row (lse = -inf) -> lse = lse_sink, scale untouched (its output is never
// stored). lse_sink = -inf changes nothing, bit for bit.
DEV_INLINE void index_sink_fold(float lse_sink, float& lse, float& out_scale) {
  if (lse_sink == -INFINITY) return;
  if (lse == -INFINITY) {
    lse = lse_sink;
    return;
  }
  const float m = fmaxf(lse, lse_sink);
  const float lse2 = m + logf(expf(lse - m) + expf(lse_sink - m));
  out_scale *= expf(lse - lse2);
  lse = lse2;
}

// Per-head running maximum. In the index kernels a lane owns one query head,
// so there is nothing to reduce across the wave beyond the two 32-lane halves
// (the caller's row max already is). The maximum only grows, so a plain read
// that is stale can only be too small: it filters out almost every atomic
// (all tokens hit the same hq addresses) and never drops a needed one.
DEV_INLINE void head_atomic_max(float* dst, float v) {
  if (v != -INFINITY &&
      v > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    unsafeAtomicMax(dst, v);
}

// one packed convert (RNE, same as the scalar bf16 cast) — the C version
// lowers to 2 cvt + shift + or, 4x the issue slots (guide: cvt_pk idiom)
DEV_INLINE unsigned pack_bf16_pair(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// raw v_exp_f32: the libm exp2f expands to ~5 instructions of denormal-range
// guards; specials (inf/NaN) behave identically, only sub-denormal precision
// differs (P < 1e-38 ~ 0)
DEV_INLINE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// C/D fragment row for v_mfma_f32_32x32x16_bf16: reg r, lane-half hi
DEV_INLINE int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ds_read_b64_tr_b16 pair -> one MFMA B-fragment (8 bf16).
// Probed semantics (tests/gpu_probe_tr16.py): within each 16-lane group, the
// addresses of lanes =0 (mod 4) give four ROW base addresses; lane l receives
// element (row_j_base + (l&15)) for j=0..3. Two reads cover 8 rows. The rows'
// 32-B runs must be physically contiguous, hence the 32-B-granular swizzle
// of the staged row images.
// The clang builtin rather than inline asm: an asm read forces
// `s_waitcnt lgkmcnt(0)` + a sched fence per fragment — a full ~50-cycle
// LDS-latency park before every second MFMA of the output matmuls. The
// builtin is the same instruction but scheduler-visible: reads pipeline
// across fragments and waits batch.
DEV_INLINE bf16x8 tr16_frag(int a0, int a1) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_;
  bf16x4_ v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_*)(unsigned)a0);
  bf16x4_ v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_*)(unsigned)a1);
  union {
    bf16x4_ h[2];
    bf16x8 v;
  } r;
  r.h[0] = v0;
  r.h[1] = v1;
  return r.v;
}

// Half (tt = 0/1) of a 32x32 C/D fragment (16 fp32 per lane) -> bf16 MFMA
// A-fragment of the same matrix: packed converts + two permlane32 swaps,
// no LDS round trip.
DEV_INLINE bf16x8 cframe_to_afrag(const float* val, int tt) {
  unsigned c0 = pack_bf16_pair(val[8 * tt + 0], val[8 * tt + 1]);
  unsigned c1 = pack_bf16_pair(val[8 * tt + 2], val[8 * tt + 3]);
  unsigned c2 = pack_bf16_pair(val[8 * tt + 4], val[8 * tt + 5]);
  unsigned c3 = pack_bf16_pair(val[8 * tt + 6], val[8 * tt + 7]);
  {
    auto r2 = __builtin_amdgcn_permlane32_swap(c0, c2, false, false);
    c0 = r2[0];
    c2 = r2[1];
  }
  {
    auto r2 = __builtin_amdgcn_permlane32_swap(c1, c3, false, false);
    c1 = r2[0];
    c3 = r2[1];
  }
  union {
    unsigned u[4];
    bf16x8 v;
  } cvt;
  cvt.u[0] = c0;
  cvt.u[1] = c1;
  cvt.u[2] = c2;
  cvt.u[3] = c3;
  return cvt.v;
}

// ---- element type of the dense kernels (ffa_fwd.hip, ffa_bwd.hip) ----
// Everything that differs between bf16 and fp16 q/k/v/dout: the fragment
// vector, the 32x32x16 MFMA, the packed f32 -> 16-bit convert and the scalar
// converts of the epilogues. Staging, swizzles and LDS layouts work in bytes
// and the softmax in fp32, so they are shared. The bf16 members are the
// helpers above, unchanged.
using f16_t = _Float16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// RNE like pack_bf16_pair (the mode register's default rounding); results
// below the smallest fp16 subnormal (2^-24) flush to zero
DEV_INLINE unsigned pack_f16_pair(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

template <class T>
struct ElemTraits;

template <>
struct ElemTraits<bf16_t> {
  using x8 = bf16x8;
  static DEV_INLINE f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static DEV_INLINE unsigned pack_pair(float lo, float hi) {
    return pack_bf16_pair(lo, hi);
  }
  static DEV_INLINE x8 tr16(int a0, int a1) { return tr16_frag(a0, a1); }
  static DEV_INLINE x8 afrag(const float* val, int tt) {
    return cframe_to_afrag(val, tt);
  }
  static DEV_INLINE float to_f32(bf16_t x) { return (float)x; }
  static DEV_INLINE bf16_t from_f32(float x) { return (bf16_t)x; }
};

template <>
struct ElemTraits<f16_t> {
  using x8 = f16x8;
  static DEV_INLINE f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static DEV_INLINE unsigned pack_pair(float lo, float hi) {
    return pack_f16_pair(lo, hi);
  }
  // ds_read_b64_tr_b16 moves 16-bit lanes whatever they hold
  static DEV_INLINE x8 tr16(int a0, int a1) {
    return __builtin_bit_cast(x8, tr16_frag(a0, a1));
  }
  // cframe_to_afrag with the fp16 packed convert
  static DEV_INLINE x8 afrag(const float* val, int tt) {
    unsigned c0 = pack_f16_pair(val[8 * tt + 0], val[8 * tt + 1]);
    unsigned c1 = pack_f16_pair(val[8 * tt + 2], val[8 * tt + 3]);
    unsigned c2 = pack_f16_pair(val[8 * tt + 4], val[8 * tt + 5]);
    unsigned c3 = pack_f16_pair(val[8 * tt + 6], val[8 * tt + 7]);
    auto r02 = __builtin_amdgcn_permlane32_swap(c0, c2, false, false);
    auto r13 = __builtin_amdgcn_permlane32_swap(c1, c3, false, false);
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;
    const u32x4_ u = {r02[0], r13[0], r02[1], r13[1]};
    return __builtin_bit_cast(x8, u);
  }
  static DEV_INLINE float to_f32(f16_t x) { return (float)x; }
  // The empty asm keeps x a finished f32: left visible, the compiler folds
  // the epilogue's `acc * (1 / l)` into the convert as one v_fma_mixlo_f16,
  // which rounds the exact product once. The direct store would then differ
  // in the last bit from the f32 merge path cast to fp16, which rounds twice.
  static DEV_INLINE f16_t from_f32(float x) {
    asm("" : "+v"(x));
    return (f16_t)x;
  }
};

// elem_type of magi_ffa_fwd_args / magi_ffa_bwd_args names one of the two
// (host side: the entries check it before any HIP call)
static inline bool elem_type_known(int elem_type) {
  return elem_type == MAGI_FFA_ELEM_BF16 || elem_type == MAGI_FFA_ELEM_FP16;
}

// ---- fp8 (OCP e4m3) helpers shared by ffa_fwd_fp8.hip / ffa_index_fp8.hip ----

// f32 -> e4m3 via the packed convert (lower byte)
DEV_INLINE unsigned char to_fp8(float x) {
  union {
    short s;
    unsigned char b[2];
  } r;
  r.s = __builtin_amdgcn_cvt_pk_fp8_f32(x, 0.f, 0, false);
  return r.b[0];
}

// Half (tt = 0/1) of a 32x32 C/D fragment -> fp8 MFMA A-fragment (8 e4m3
// bytes) of the same matrix: pack 4 + 4 bytes, ONE permlane32 swap per 16-k.
DEV_INLINE long cframe_to_afrag_fp8(const float* val, int tt) {
  union {
    unsigned char b[4];
    unsigned u;
  } A, B;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A.b[j] = to_fp8(val[8 * tt + j]);
    B.b[j] = to_fp8(val[8 * tt + 4 + j]);
  }
  auto r2 = __builtin_amdgcn_permlane32_swap(A.u, B.u, false, false);
  return ((long)(unsigned)r2[1] << 32) | (unsigned)r2[0];
}

// fp8 softmax offset in the exp2 domain (reference softmax.h:151): P =
// exp2(t - m + 8) lands in [0, 256], inside the e4m3 range (max 448). l_run
// and acc_o carry the 2^8; the epilogues subtract it from the lse again.
constexpr float FP8_MAX_OFFSET = 8.f;

// One online-softmax step of the fp8 forwards, swapped-QK layout: a lane owns
// the 16 scores t[] of ONE q row (the other 16 sit in lane ^ 32), already
// scaled into the exp2 domain, masked slots -inf; mx is their lane-local max.
// Updates m_run, l_run and acc_o and leaves P in pr[] (a masked slot is
// exactly 0).
// No defer-max: a deferred maximum would let P exceed 256. The O rescale sits
// under a wave-uniform condition: ds_bpermute reads other lanes' registers,
// so every lane must be active whenever any lane needs it.
template <int DT>
DEV_INLINE void softmax_step_fp8(const float (&t)[16], float mx, int hi,
                                 float& m_run, float& l_run,
                                 f32x16 (&acc_o)[DT], float (&pr)[16]) {
  mx = fmaxf(mx, warp_xor32(mx));
  const float m_new = fmaxf(m_run, mx);
  const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
  const float alpha = (m_run == -INFINITY) ? 0.f : fast_exp2(m_run - m_use);
  m_run = m_new;

  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    pr[r] = fast_exp2(t[r] - m_use + FP8_MAX_OFFSET);
    psum += pr[r];
  }
  l_run = l_run * alpha + (psum + warp_xor32(psum));

  if (__any(alpha != 1.f)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int src = crow(r, hi);
      const float aq = __uint_as_float(
          __builtin_amdgcn_ds_bpermute(src << 2, __float_as_uint(alpha)));
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc_o[dt][r] *= aq;
    }
  }
}

// ---- index forward, host side (ffa_index.hip: T = bf16_t, ffa_index_fp8.hip:
// T = unsigned char) ----

template <class T>
struct IdxFwdParams {
  const T* q;
  const T* k;
  const T* v;
  float* out_f32;    // used when OUT_BF16 == false
  bf16_t* out_bf16;  // used when OUT_BF16 == true
  float* lse;
  const int* idx2d;  // [total_q, max_topk]
  int max_topk;
  int hq;
  float scale;
  float softcap;
  long long total_q, total_k;
  const float* sink;  // null = no sink
  int s_sink;
  int sink_ssh;
  float* max_logits;  // [hq], null = off
};

// Body of magi_ffa_fwd_index / magi_ffa_fwd_index_fp8: checks, params, launch
// shape and dispatch. launch(D, W, HAS_SOFTCAP, OUT_BF16, grid, block, stream,
// p) gets the four template arguments as std::integral_constant values and
// launches its kernel. Nothing before that call touches the HIP runtime.
template <class T, class Launch>
static int index_fwd_entry(const magi_ffa_index_args* a, Launch launch) {
  if (!a || !a->q || !a->k || !a->v || !a->out || !a->lse || !a->indices_2d)
    return -1;
  if (a->d != 64 && a->d != 128) return -2;
  if (a->hk != 1) return -3;  // kv heads are folded into K rows (magi_ffa.h)
  if (a->max_topk <= 0 || (a->max_topk & 63) != 0) return -4;
  if (a->sink && (a->s_sink < 1 || a->s_sink > 8)) return -5;
  if (a->total_q <= 0 || a->hq <= 0) return 0;

  IdxFwdParams<T> p;
  p.q = (const T*)a->q;
  p.k = (const T*)a->k;
  p.v = (const T*)a->v;
  p.out_f32 = (float*)a->out;
  p.out_bf16 = (bf16_t*)a->out;
  p.lse = a->lse;
  p.idx2d = a->indices_2d;
  p.max_topk = a->max_topk;
  p.hq = a->hq;
  p.scale = a->softmax_scale;
  p.softcap = a->softcap;
  p.total_q = a->total_q;
  p.total_k = a->total_k;
  p.sink = a->sink;
  p.s_sink = a->s_sink;
  p.sink_ssh = a->sink_ssh;
  p.max_logits = a->max_logits;

  // head-block = 32*W query heads; pick W so one wave-set covers hq (DiT
  // ratio 128 -> 4 waves; small-ratio MHA shapes keep lanes busy at W=1)
  const int w = (a->hq > 64) ? 4 : (a->hq > 32 ? 2 : 1);
  const int span = 32 * w;
  const dim3 grid((unsigned)a->total_q, (unsigned)((a->hq + span - 1) / span),
                  1);
  const dim3 block(64 * w);
  const hipStream_t stream = (hipStream_t)a->stream;
  const bool sc = a->softcap > 0.f;
  const bool obf16 = !a->out_is_fp32;
  auto with_dw = [&](auto D, auto W) {
    auto go = [&](auto SC, auto OB) {
      launch(D, W, SC, OB, grid, block, stream, p);
    };
    if (sc) {
      if (obf16) go(std::true_type{}, std::true_type{});
      else go(std::true_type{}, std::false_type{});
    } else {
      if (obf16) go(std::false_type{}, std::true_type{});
      else go(std::false_type{}, std::false_type{});
    }
  };
  auto with_d = [&](auto D) {
    if (w == 4) with_dw(D, std::integral_constant<int, 4>{});
    else if (w == 2) with_dw(D, std::integral_constant<int, 2>{});
    else with_dw(D, std::integral_constant<int, 1>{});
  };
  if (a->d == 64) with_d(std::integral_constant<int, 64>{});
  else with_d(std::integral_constant<int, 128>{});
  return (int)hipGetLastError();
}
