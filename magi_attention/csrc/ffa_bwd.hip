// ffa_bwd.hip — MI355X-native flex-flash-attention BACKWARD (gfx950).
//
// Behaviour: reference flash_bwd_kernel_sm90.h:41 /
// mainloop_bwd_sm90_tma_gmma_ws.hpp (5-matmul recompute backward, fp32 atomic
// dQ/dK/dV accumulation; preprocess dPsum = rowsum(dO*O),
// flash_bwd_preprocess_kernel.h:42).
//
// Three kernels, launched as separate passes by the host:
//   bwd_preprocess_kernel  dpsum = rowsum(dO * O), one wave per (row, head).
//   ffa_bwd_dq_kernel      q-outer: a workgroup of WAVES (4 or 8) waves owns
//     WAVES x 32 q rows of one range+head; each wave keeps its Q/dO fragments
//     and its dQ accumulator in registers and loops over the k range. K/V
//     tiles (64 rows per barrier) are staged once per workgroup into
//     XOR-swizzled LDS by global_load_lds and consumed by all waves:
//       S^T = K Q^T ; dP^T = V dO^T ; dS^T (base-2 recompute, like the fwd)
//       dQ += dS K   (dS^T -> A-frag in-register via permlane, K B-frags by
//                     tr16 reads off the staged row image)
//     dQ is atomic-added once at the end. The stage loads are issued outside
//     the compiler's waitcnt tracking (glds16_untracked, as in the fused
//     dK/dV mode below): the barrier's counted vmcnt is the only
//     vector-memory wait in the k loop, the kernel drains by hand at the end
//     of every k segment, and the LDS fragment reads of all three matmuls run
//     one step ahead of their MFMA.
//   ffa_bwd_dkv_kernel     k-outer: a workgroup owns WAVES x 32 k rows; each
//     wave accumulates its dK and/or dV tile in registers over the q loop and
//     atomic-adds it once at the end. Q/dO tiles are staged per iteration:
//       S = Q K^T ; dP = dO V^T ; P, dS
//       dV += P^T dO ; dK += dS^T Q   (P/dS -> A-frags in-register, dO/Q
//                                      B-frags by tr16 reads)
//     MODE 0 computes both (fused: K and V tiles live in LDS), MODE 1 only dV,
//     MODE 2 only dK (split: K/V fragments live in registers).
//     lse / dpsum of the staged q rows: the split modes stage them into LDS
//     by LDS-DMA next to the Q/dO image. The fused mode has no LDS left for
//     them: each lane loads the lse and dpsum of one row per 32-row subtile
//     into registers, one staged tile AHEAD and before that tile's prefetch,
//     and compute selects rows with ds_bpermute. The fused mode also issues
//     its Q/dO prefetch outside the compiler's waitcnt tracking
//     (glds16_untracked), so its subtile loop holds no vector-memory wait and
//     the prefetch flies for the whole iteration.
// 8 waves (one 512-thread workgroup per CU, 2 waves/SIMD) serve long ranges,
// 4 waves short ranges and D=192; the launchers at the end of the file pick.
// The staging ring depth (NBUF) is fixed by (MODE, WAVES) inside each kernel.
// Both mainloop kernels end in one of two epilogues, chosen at compile time:
// DIRECT = false adds the register tile into a zeroed f32 buffer with atomics
// (ranges may overlap, GQA heads share dK/dV rows); DIRECT = true rounds it to
// the element type and stores it once with plain stores, for callers that
// promise a single owner per element (the *_direct entries, magi_ffa.h).

#include <hip/hip_runtime.h>
#include <math.h>
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

// ---------------- preprocess: dpsum = rowsum(dO * O) ----------------
template <class ET, bool OUT_F32>
__global__ __launch_bounds__(256) void bwd_preprocess_kernel(BwdParams<ET> p,
                                                             int d,
                                                             long long n_rows) {
  using Tr = ElemTraits<ET>;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const int per = d / 64;
  const ET* do_p = p.dout + row * d;
  float acc = 0.f;
  for (int e = 0; e < per; ++e) {
    const int idx = lane * per + e;
    const float dov = Tr::to_f32(do_p[idx]);
    float ov;
    if (OUT_F32)
      ov = ((const float*)p.out)[row * d + idx];
    else
      ov = Tr::to_f32(((const ET*)p.out)[row * d + idx]);
    acc += dov * ov;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if (lane == 0) p.dpsum[row] = acc;
}


// ---------------- mainloop ----------------
// MODE 0: fused dK+dV — r2 redesign: V fragments live in a per-wave LDS tile
// (staged once per block) instead of 32 persistent VGPRs, which brings the
// fused kernel under the 256-reg budget of 2 waves/SIMD (r1's fused version
// was 437 regs = 1 wave/SIMD, or 65 scratch spills RELOADED EVERY ITERATION
// when forced to 256). Shares S, P, exp2 and the staged Q/dO image between
// the dV and dK matmuls: 32 MFMAs per subtile vs the split modes' 40.
// MODE 1: dV only / MODE 2: dK only — the r1 split, kept selectable.
// WAVES: k-tiles per workgroup sharing ONE staged Q/dO image (4 or 8; the
// D=192 builds spill at 8 waves' 256-register cap and exist at 4 only).
// NBUF: LDS staging ring depth. 2 = barrier drains vmcnt(0), prefetch has
// one compute phase to land. 3 = constant-distance vmcnt(G) barrier:
// prefetch has TWO compute phases, and the barrier only waits for the one
// stage it needs — attacks the 34-42% SQ_WAIT_ANY of the r1 PMC. The split
// 8-wave kernels run the 3-ring; the fused mode keeps 2 (its K/V tiles + a
// 3-ring exceed the 160 KB LDS), and so do 4-wave workgroups (3 buffers
// exceed the 80 KB/WG budget of 2 blocks/CU).
// DIRECT: the epilogue (see the head of the file); nothing before it differs.
// CAT (cat_gqa): the head index of a work item is the KV head, and the
// workgroup walks the p.cat = gqa q heads h = kh * gqa + j of that group into
// the one dK/dV register tile, so K/V are staged once per group and every
// dK/dV row has one owner per k range. Visiting order, a function of the
// tables alone: q segments in order, and within a segment j ascending. Each
// (segment, head) pass is a whole pass of the segment loop: fresh ring state
// and prologue stages, the segment's closing barrier, nothing staged or
// prefetched carried from one head to the next. CAT is a template parameter,
// not a runtime p.cat, so that the CAT = false kernels stay the code they
// were (profiles/bwd_cat_gqa.md has both resource tables).
template <class ET, int D, bool HAS_SOFTCAP, int MODE, int WAVES, bool DIRECT,
          bool CAT>
__global__ __launch_bounds__(64 * WAVES, WAVES == 8 ? 2 : 1)
void ffa_bwd_dkv_kernel(BwdParams<ET> p) {
  using Tr = ElemTraits<ET>;
  using vec8 = typename Tr::x8;
  static_assert(WAVES == 4 || (WAVES == 8 && D != 192), "unsupported shape");
  constexpr int NBUF = (MODE != 0 && WAVES == 8) ? 3 : 2;
  constexpr bool WANT_DV = MODE != 2;
  constexpr bool WANT_DK = MODE != 1;
  constexpr bool V_IN_LDS = MODE == 0;
  constexpr int DF = D / 16;
  constexpr int DT = D / 32;
  // LDS rows padded to a power of two (D=192 -> 512-byte rows; see
  // ffa_fwd.hip note on the swizzle bijection)
  constexpr int ROWB = (D == 192) ? 512 : D * 2;
  constexpr int ROWE = ROWB / 2;
  constexpr int VSLOTS = D / 8;
  // XOR swizzle within one LDS row: spreads a b128 lane group over the row's
  // 16-B slots (T2/G4); mask keeps the XOR inside the row for D=64 too.
  // 32-B-granular XOR swizzle: spreads b128 lane groups over the row's 16-B
  // slot pairs (<=2-way) while keeping every 32-B run physically contiguous,
  // which the tr16 row reads require; mask scales with row size (D=64 rows
  // are 128 B).
  constexpr int SW32M = ROWB / 32 - 1;
  auto swz = [](int row, int byte_off) {
    return byte_off ^ ((row & SW32M) << 5);
  };
  // Adaptive grid (see fwd kernel): head-major = XCD-affine atomics + K/V
  // L2 locality per head; work-major when one head's operands overflow an
  // XCD's L2.
  // CU-margin strided-grid mode (see ffa_fwd.hip): margin>0 caps the grid
  // below the resident-WG count; each WG walks the flattened work space.
  // MODE 0 sits at exactly the 256-reg budget and the loop backedge costs it
  // 41 scratch spills — its launcher never caps the grid, so the loop is
  // made provably single-iteration there and dissolves at compile time.
  const long long work_total =
      (long long)p.work_nx * p.work_ny * p.work_nz;
  const long long grid_span = (long long)gridDim.x * gridDim.y * gridDim.z;
  const long long w_first = blockIdx.x +
      (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * blockIdx.z);
  for (long long w = w_first; w < work_total; w += grid_span) {
  const int wx = (int)(w % p.work_nx);
  const long long w2 = w / p.work_nx;
  const int wy = (int)(w2 % p.work_ny);
  const int wz = (int)(w2 / p.work_ny);
  const int ri = wz;
  const int hidx = p.head_major ? wx : wy;
  // CAT: the kv head; the q head h is set per pass of the segment loop
  const int hsel = p.head_off + hidx * p.head_mult;
  int h = CAT ? hsel * p.gqa : hsel;
  const int wb = p.head_major ? wy : wx;
  const int ks = p.k_ranges[2 * ri], ke = p.k_ranges[2 * ri + 1];
  const int nblk0 = ks + wb * (BWD_BN * WAVES);
  if (nblk0 >= ke) continue;
  const int seg0 = p.seg_starts ? p.seg_starts[ri] : ri;
  const int seg1 = p.seg_starts ? p.seg_starts[ri + 1] : ri + 1;
  int qs, qe, atype;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // static priority for the second-dispatched half of an 8-wave WG: the
  // younger waves are the VALU-arbitration losers on every segment
  // (MI355X guide, two-waves-per-SIMD item 4)
  if (WAVES == 8 && wave >= 4) asm volatile("s_setprio 1");

  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  const int n0 = nblk0 + wave * BWD_BN;  // this wave's k tile
  const bool wave_live = n0 < ke;

  const float sl2 = HAS_SOFTCAP ? p.softcap * 1.4426950408889634f
                                : p.scale * 1.4426950408889634f;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;
  const float log2e = 1.4426950408889634f;

  const int kh = CAT ? hsel : h / p.gqa;
  const size_t k_pitch = (size_t)p.hk * D;
  const size_t q_pitch = (size_t)p.hq * D;

  // LDS: double-buffered Q/dO tiles (XOR-swizzled rows, filled by
  // global_load_lds with the swizzle on the SOURCE address — rule 21) +
  // per-wave P/dS transpose tiles. One barrier per iteration; the glds for
  // tile t+1 flies under tile t's compute and is drained by the next
  // barrier's implicit vmcnt(0).
  // ONE shared object only: a second __shared__ array makes hipcc drain
  // vmcnt(0) before every ds_read, destroying the glds pipeline (guide §5
  // ".s-level traps" (a)).
  // NBUF x 64-row Q/dO images: one barrier per 64 q rows — the doubled
  // compute phase covers the prefetch latency a 32-row phase could not.
  // MODE 0 (fused, r2-v2): BOTH the K and V tiles of every wave live in LDS
  // (2 x 64 KB) and the Q/dO ring shrinks to 32-row images (32 KB) — that
  // is the LDS budget to the byte, so lse/dpsum move from LDS to lane
  // registers + ds_bpermute. This removes the per-subtile K re-reads that
  // made the previous fused kernel fabric-bound (PMC: 172 GB/launch of
  // L2-miss fetch vs the split kernels' ~70) AND leaves ~36 registers of
  // scheduler slack below the 256 cap.
  // (the 32-row ring is only needed at D=128, where the K/V tiles take
  // 128 KB; at D=64 everything fits beside a 64-row ring)
  // Ring rows: the fused mode's K/V tiles crowd the 64-row ring out of LDS
  // at D=128 when the WG spans 256 k rows (W8).
  constexpr int QITER =
      (V_IN_LDS && D == 128 && WAVES == 8) ? BWD_BM : 2 * BWD_BM;
  constexpr int NSUB = QITER / BWD_BM;
  constexpr int KVLDS = V_IN_LDS ? 2 * WAVES * BWD_BN * ROWB : 0;
  constexpr int LSELDS = V_IN_LDS ? 0 : NBUF * 2 * QITER * 4;
  static_assert(NBUF * 2 * QITER * ROWB + LSELDS + KVLDS <= 163840,
                "LDS budget");
  __shared__ __attribute__((aligned(16))) char smem[
      NBUF * 2 * QITER * ROWB + LSELDS + KVLDS];
  auto lds_q = [&](int buf) -> ET* {
    return (ET*)(smem + (2 * buf) * QITER * ROWB);
  };
  auto lds_do = [&](int buf) -> ET* {
    return (ET*)(smem + (2 * buf + 1) * QITER * ROWB);
  };
  // lse / dpsum, staged by LDS-DMA (one dword per lane: lanes 0-31 lse,
  // 32-63 dpsum), one call per 32-row group: layout per buffer is
  // [lse g0 (32) | dps g0 (32) | lse g1 (32) | dps g1 (32)]
  auto lds_lse = [&](int buf) -> float* {
    return (float*)(smem + NBUF * 2 * QITER * ROWB + buf * 2 * QITER * 4);
  };
  // MODE 0: per-wave K and V tiles (BWD_BN rows x D, same 32-B XOR swizzle
  // as the Q/dO images so the A-fragment reads reuse the qf addressing)
  ET* lds_kt = (ET*)(smem + NBUF * 2 * QITER * ROWB + LSELDS) +
                   wave * BWD_BN * ROWE;
  ET* lds_vt = (ET*)(smem + NBUF * 2 * QITER * ROWB + LSELDS +
                             KVLDS / 2) +
                   wave * BWD_BN * ROWE;

  // K fragments (A-layout), loaded once per block; V fragments likewise in
  // the split dK mode — the fused mode stages V into LDS instead (register
  // budget).
  const int krow = n0 + lo32;
  const int kcl = min(krow, ke - 1);
  // MODE 0 does NOT keep K fragments live across the q loop — that was what
  // pushed the first fused kernel to 437 regs / scratch spills. It reads no K
  // from global memory in the loop either: each subtile takes its K (and V)
  // fragments off the wave's LDS tile staged below, so the registers are
  // subtile-local. kp_row serves the split modes only.
  const ET* kp_row = p.k + (size_t)kcl * k_pitch + (size_t)kh * D + hi * 8;
  vec8 kfA[V_IN_LDS ? 1 : DF], vfA[(WANT_DK && !V_IN_LDS) ? DF : 1];
  if constexpr (!V_IN_LDS) {
    const ET* vp = p.v + (size_t)kcl * k_pitch + (size_t)kh * D;
#pragma unroll
    for (int dd = 0; dd < DF; ++dd) {
      kfA[dd] = *(const vec8*)(kp_row - hi * 8 + dd * 16 + hi * 8);
      if constexpr (WANT_DK)
        vfA[dd] = *(const vec8*)(vp + dd * 16 + hi * 8);
    }
  }
  constexpr int ROWS_PER_GLDS_V = 1024 / ROWB;
  if constexpr (V_IN_LDS) {
#pragma unroll
    for (int gi = 0; gi < BWD_BN / ROWS_PER_GLDS_V; ++gi) {
      const int r0v = ROWS_PER_GLDS_V * gi;
      const int r = r0v + lane / (ROWB / 16);
      const int c = lane % (ROWB / 16);
      const int kr = min(n0 + r, ke - 1);
      int cs = c ^ ((r & SW32M) << 1);
      if (cs >= VSLOTS) cs = 0;
      const int csw = cs * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              p.k + (size_t)kr * k_pitch + (size_t)kh * D + csw),
          (__attribute__((address_space(3))) unsigned int*)&lds_kt[r0v * ROWE],
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              p.v + (size_t)kr * k_pitch + (size_t)kh * D + csw),
          (__attribute__((address_space(3))) unsigned int*)&lds_vt[r0v * ROWE],
          16, 0, 0);
    }
  }

  // block + wave q loop bounds (recomputed per q segment)
  const int nlast = min(nblk0 + BWD_BN * WAVES, ke) - 1;
  int q_lo = 0, q_hi = 0, wq_lo = 0, wq_hi = 0;
  auto seg_bounds = [&]() {
    q_lo = qs; q_hi = qe;
    if (atype == 1 || atype == 3) q_lo = max(q_lo, nblk0 - (ke - qe));
    if (atype == 2 || atype == 3) q_hi = min(q_hi, nlast - (ks - qs) + 1);
    wq_lo = qs; wq_hi = qe;
    if (atype == 1 || atype == 3) wq_lo = max(wq_lo, n0 - (ke - qe));
    if (atype == 2 || atype == 3)
      wq_hi = min(wq_hi, (n0 + BWD_BN - 1) - (ks - qs) + 1);
  };

  f32x16 acc_dk[WANT_DK ? DT : 1], acc_dv[WANT_DV ? DT : 1];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    if constexpr (WANT_DK) acc_dk[dt] = (f32x16)(0.f);
    if constexpr (WANT_DV) acc_dv[dt] = (f32x16)(0.f);
  }

  // each wave's glds covers 4 rows (64 lanes x 16B = 1 KiB = 4 rows at D=128);
  // glds issues are dealt round-robin over the waves (wave-strided), so any
  // WAVES count works; the NBUF=3 constant-distance barrier needs a UNIFORM
  // per-wave issue count, so it requires divisibility.
  constexpr int ROWS_PER_GLDS = 1024 / ROWB;
  constexpr int GLDS_TOTAL = QITER / ROWS_PER_GLDS;
  static_assert(NBUF == 2 || GLDS_TOTAL % WAVES == 0, "uniform stage count");
  constexpr int GLDS_PER_WAVE =
      (GLDS_TOTAL % WAVES == 0) ? GLDS_TOTAL / WAVES : 0;  // 0 = non-uniform
  // block-uniform operands of the staging addresses (scalar registers)
  // (CAT: re-pointed at each head of the group by the segment loop)
  const ET* q_head = p.q + (size_t)h * D;
  const ET* do_head = p.dout + (size_t)h * D;
  const int smem_byte = (int)(unsigned long long)(
      (__attribute__((address_space(3))) const char*)smem);
  auto stage_glds = [&](int buf, int m0x) {
#pragma unroll
    for (int gi0 = 0; gi0 < (GLDS_TOTAL + WAVES - 1) / WAVES; ++gi0) {
      const int gi = gi0 * WAVES + wave;
      if (GLDS_TOTAL % WAVES != 0 && gi >= GLDS_TOTAL) break;
      const int r0 = ROWS_PER_GLDS * gi;
      const int r = r0 + lane / (ROWB / 16);
      const int c = lane % (ROWB / 16);
      const int qrow = min(m0x + r, qe - 1);
      int cs = c ^ ((r & SW32M) << 1);
      if (cs >= VSLOTS) cs = 0;
      const int csw = cs * 8;
      // ONE per-lane element offset for both tensors, added to the
      // block-uniform head pointers: written as p.q + row + (head, slot) the
      // compiler hoists a per-lane 64-bit pointer per tensor out of the q
      // loop, and at the fused kernel's register cap spills them — each
      // reload's vmcnt(0) then serialises the loads issued here
      const size_t eoff = (size_t)qrow * q_pitch + (unsigned)csw;
      if constexpr (V_IN_LDS) {
        // fused mode: keep the prefetch out of the compiler's waitcnt
        // bookkeeping (see glds16_untracked) — every read of a staged
        // image already sits behind the pipe_barrier that retires it
        const int lq = smem_byte + (2 * buf * QITER + r0) * ROWB;
        glds16_untracked(q_head + eoff, lq);
        glds16_untracked(do_head + eoff, lq + QITER * ROWB);
        continue;
      }
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(q_head + eoff),
          (__attribute__((address_space(3))) unsigned int*)&lds_q(buf)[r0 * ROWE],
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              do_head + eoff),
          (__attribute__((address_space(3))) unsigned int*)&lds_do(buf)[r0 * ROWE],
          16, 0, 0);
    }
    // lse (lanes 0-31) / dpsum (lanes 32-63), one LDS-DMA per 32-row group
    // (MODE 0 has no LDS lse region: compute reads them into lane registers
    // and cross-lane-selects with ds_bpermute)
    if constexpr (!V_IN_LDS) {
#pragma unroll
      for (int sg = 0; sg < NSUB; ++sg) {
        const int qr = min(m0x + sg * BWD_BM + lo32, qe - 1);
        const float* src = (lane < 32) ? p.lse + (size_t)qr * p.hq + h
                                       : p.dpsum + (size_t)qr * p.hq + h;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)src,
            (__attribute__((address_space(3))) unsigned int*)(
                lds_lse(buf) + sg * 2 * BWD_BM),
            4, 0, 0);
      }
    }
  };

  // vm ops per stage call per wave (glds pairs + lse groups) — the NBUF=3
  // constant-distance barrier counts on EVERY stage issuing exactly this many
  constexpr int GOPS = 2 * GLDS_PER_WAVE + 2;
  // MODE 0 has no LDS room for lse/dpsum: lane l holds the lse and the dpsum
  // of row (l & 31) of each 32-row subtile and compute cross-lane-selects
  // with ds_bpermute (both through the same row index; both halves of the
  // wave load the same 32 rows from the uniform base pointers, which costs
  // no per-lane pointer register). The values are register-prefetched ONE
  // staged tile ahead, issued BEFORE that tile's stage_glds: vector-memory
  // loads retire in order, so a load issued after the prefetch could only be
  // awaited with vmcnt(0), which also waits out the whole Q/dO prefetch in
  // the middle of the compute phase it was meant to hide under. Issued one
  // tile early, the values land by the next pipe_barrier<0> and the subtile
  // loop contains no vector-memory wait. Rows clamp to qe-1 like the staged
  // rows; nothing is carried across a q segment.
  float lse_nxt[V_IN_LDS ? NSUB : 1] = {}, dps_nxt[V_IN_LDS ? NSUB : 1] = {};
  auto load_lsedp = [&](int m0x) {
#pragma unroll
    for (int sg = 0; sg < NSUB; ++sg) {
      const int qr = min(m0x + sg * BWD_BM + lo32, qe - 1);
      const size_t roff = (size_t)qr * p.hq + h;
      lse_nxt[sg] = p.lse[roff];
      dps_nxt[sg] = p.dpsum[roff];
    }
  };
  int cur = 0;
  // CAT folds (segment, head of the group) into this one loop: j counts the
  // heads of the current segment and seg moves on when j wraps
  for (int seg = seg0, j = 0; seg < seg1;
       (CAT && ++j < p.cat) ? 0 : (j = 0, ++seg)) {
  qs = p.q_ranges[2 * seg];
  qe = p.q_ranges[2 * seg + 1];
  atype = p.attn_type_map ? p.attn_type_map[seg] : 0;
  if (qe <= qs) continue;  // uniform across block
  seg_bounds();
  if (q_lo >= q_hi) continue;
  if constexpr (CAT) {
    h = kh * p.gqa + j;
    q_head = p.q + (size_t)h * D;
    do_head = p.dout + (size_t)h * D;
  }
  cur = 0;
  if constexpr (V_IN_LDS) load_lsedp(q_lo);
  stage_glds(0, q_lo);
  if constexpr (NBUF == 3) stage_glds(1, q_lo + QITER);  // rows clamp to qe-1

  for (int m0 = q_lo; m0 < q_hi; m0 += QITER) {
    // NBUF=3: wait ONLY for buf[cur] (leave the next stage in flight), then
    // prefetch two stages ahead — always, with clamped rows, so the vmcnt
    // distance stays constant. NBUF=2: full drain (prefetch had one phase).
    pipe_barrier<NBUF == 3 ? GOPS : 0>();
    // MODE 0: this tile's lse/dpsum were loaded one tile ago and the barrier
    // above drained them. The empty asm pins the compiler's own wait for the
    // loads HERE, where nothing is outstanding, so none lands in the subtile
    // loop behind the prefetch issued below.
    float lse_cur[V_IN_LDS ? NSUB : 1] = {}, dps_cur[V_IN_LDS ? NSUB : 1] = {};
    if constexpr (V_IN_LDS) {
#pragma unroll
      for (int sg = 0; sg < NSUB; ++sg) {
        lse_cur[sg] = lse_nxt[sg];
        dps_cur[sg] = dps_nxt[sg];
        asm volatile("" : "+v"(lse_cur[sg]), "+v"(dps_cur[sg]));
      }
    }
    if constexpr (NBUF == 3) {
      stage_glds(cur == 0 ? 2 : cur - 1, m0 + 2 * QITER);
    } else {
      if (m0 + QITER < q_hi) {
        if constexpr (V_IN_LDS) load_lsedp(m0 + QITER);
        stage_glds(cur ^ 1, m0 + QITER);
      }
    }
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
    const int ms = m0 + sub * BWD_BM;
    if (ms >= q_hi) break;  // q_hi is block-uniform
    const ET* lqb = lds_q(cur) + sub * BWD_BM * ROWE;
    const ET* ldb = lds_do(cur) + sub * BWD_BM * ROWE;
    const float* lse_t = nullptr;
    const float* dps_t = nullptr;
    // MODE0: row (lane & 31) of this subtile (bpermute)
    const float lse_reg = lse_cur[V_IN_LDS ? sub : 0];
    const float dps_reg = dps_cur[V_IN_LDS ? sub : 0];
    if constexpr (!V_IN_LDS) {
      lse_t = lds_lse(cur) + sub * 2 * BWD_BM;
      dps_t = lse_t + BWD_BM;
    }
    auto lse_at = [&](int rl) -> float {
      if constexpr (!V_IN_LDS) return lse_t[rl];
      return __uint_as_float(__builtin_amdgcn_ds_bpermute(
          rl << 2, __float_as_uint(lse_reg)));
    };
    auto dps_at = [&](int rl) -> float {
      if constexpr (!V_IN_LDS) return dps_t[rl];
      return __uint_as_float(__builtin_amdgcn_ds_bpermute(
          rl << 2, __float_as_uint(dps_reg)));
    };

    if (wave_live && ms + BWD_BM > wq_lo && ms < wq_hi) {
      // ---- S = Q K^T ; dP = dO V^T, UN-swapped: C layout [q=crow][k=lo32],
      // so the dV/dK A-fragments come from the in-register permlane transform
      // (cframe) instead of an LDS round-trip ----
      f32x16 s = (f32x16)(0.f), dp = (f32x16)(0.f);
      if constexpr (V_IN_LDS) {
        // fused mode: K and V fragments come straight off the wave's LDS
        // tiles (staged once per block) — identical addressing to qf. The
        // two independent MFMA streams cover each other's LDS read latency.
        const char* kt_c = (const char*)lds_kt;
        const char* vt_c = (const char*)lds_vt;
#pragma unroll
        for (int dd = 0; dd < DF; ++dd) {
          const int off = swz(lo32, lo32 * ROWB + dd * 32 + hi * 16);
          vec8 dof = *(const vec8*)((const char*)ldb + off);
          vec8 vf = *(const vec8*)(vt_c + off);
          dp = Tr::mfma(dof, vf, dp);
          vec8 qf = *(const vec8*)((const char*)lqb + off);
          vec8 kf = *(const vec8*)(kt_c + off);
          s = Tr::mfma(qf, kf, s);
        }
      } else {
#pragma unroll
      for (int dd = 0; dd < DF; ++dd) {
        const int off = swz(lo32, lo32 * ROWB + dd * 32 + hi * 16);
        vec8 qf = *(const vec8*)((const char*)lqb + off);
        s = Tr::mfma(qf, kfA[dd], s);
        if constexpr (WANT_DK) {
          vec8 dof = *(const vec8*)((const char*)ldb + off);
          dp = Tr::mfma(dof, vfA[dd], dp);
        }
      }
      }

      const int kk = n0 + lo32;  // this lane's k column
      // S is dead once P is computed, dP once dS is — reuse their registers
      // (all indices are compile-time constants after unrolling, so the
      // pointer cast stays in VGPRs; checked: ScratchSize 0)
      float* pv = (float*)&s;
      float* dsv = (float*)&dp;
      const bool interior =
          (ms + BWD_BM <= wq_hi) && (ms >= qs) && (n0 + BWD_BN <= ke) &&
          !((atype == 1 || atype == 3) && (n0 + BWD_BN - 1 > ms + (ke - qe))) &&
          !((atype == 2 || atype == 3) && (n0 < ms + BWD_BM - 1 + (ks - qs)));
      // each row's lse is fetched once and shared by the all_live check and
      // the exponent (MODE 0: one ds_bpermute per row instead of two)
      float lqv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) lqv[r] = lse_at(crow(r, hi));
      bool all_live = interior;
      if (interior) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float lq = lqv[r];
          all_live = all_live && (lq != INFINITY) && (lq != -INFINITY);
        }
      }
      if (__all(all_live) && !HAS_SOFTCAP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = crow(r, hi);
          const float pij = fast_exp2(s[r] * sl2 - lqv[r] * log2e);
          if constexpr (WANT_DV) pv[r] = pij;
          if constexpr (WANT_DK)
            dsv[r] = pij * (dp[r] - dps_at(rl)) * p.scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qrow = ms + crow(r, hi);
          const float lq = (qrow < qe) ? lqv[r] : INFINITY;
          bool ok = (qrow < wq_hi) && (qrow >= qs) && lq != INFINITY &&
                    lq != -INFINITY && kk < ke;
          if (atype == 1 || atype == 3) ok = ok && (kk - qrow <= ke - qe);
          if (atype == 2 || atype == 3) ok = ok && (kk - qrow >= ks - qs);
          float sv = s[r];
          float dscale = p.scale;
          float t;
          if (HAS_SOFTCAP) {
            const float th = tanhf(sv * cap_pre);
            t = th * sl2;
            dscale = p.scale * (1.f - th * th);
          } else {
            t = sv * sl2;
          }
          const float pij = ok ? fast_exp2(t - lq * log2e) : 0.f;
          if constexpr (WANT_DV) pv[r] = pij;
          if constexpr (WANT_DK)
            dsv[r] = pij * (dp[r] - dps_at(crow(r, hi))) * dscale;
        }
      }

      // ---- dV += P^T dO ; dK += dS^T Q ----
      // B-fragments read straight off the ROW images with ds_read_b64_tr_b16:
      // per 16-lane group, q-row bases rd*4+j supply the transpose; the 32-B
      // runs stay contiguous under the 32-B-granular swizzle. Per (dt, rd):
      //   addr = lds_base + row*ROWB + ((dcol*2) ^ ((row&7)<<5)) + (l&3)*8
      // (the XOR distributes because the swizzle bits live inside dcol*2).
      {
        const int qhalf = (lane >> 4) & 1;       // which 16-d column half
        const int jrow = (lane & 15) >> 2;       // canonical row for this lane
        const int row0 = 8 * hi + jrow;          // rd = 0 rows
        const int row1 = 8 * hi + 4 + jrow;      // rd = 1 rows
        const int q_base = (int)(unsigned long long)(
            (__attribute__((address_space(3))) const char*)lqb);
        const int do_base = (int)(unsigned long long)(
            (__attribute__((address_space(3))) const char*)ldb);
        const int lane8 = (lane & 3) * 8;
        const int sw0 = (row0 & SW32M) << 5;
        const int sw1 = (row1 & SW32M) << 5;
        const int rb0 = row0 * ROWB + lane8;
        const int rb1 = row1 * ROWB + lane8;
        // q rows 16..31 (second kk sub-tile)
        const int sw2 = ((row0 + 16) & SW32M) << 5;
        const int sw3 = ((row1 + 16) & SW32M) << 5;
        const int rb2 = (row0 + 16) * ROWB + lane8;
        const int rb3 = (row1 + 16) * ROWB + lane8;
        // software-pipelined B-frag matmul: step j+1's fragment reads issue
        // under step j's MFMA (see dq kernel note)
        auto pipe_mm = [&](int tbase, vec8 a0, vec8 a1, f32x16* acc) {
          vec8 bcur = Tr::tr16(tbase + rb0 + ((16 * qhalf * 2) ^ sw0),
                                  tbase + rb1 + ((16 * qhalf * 2) ^ sw1));
#pragma unroll
          for (int j = 0; j < 2 * DT; ++j) {
            vec8 bnext = bcur;
            if (j + 1 < 2 * DT) {
              const int dcoln = (((j + 1) >> 1) * 32 + 16 * qhalf) * 2;
              if ((j + 1) & 1)
                bnext = Tr::tr16(tbase + rb2 + (dcoln ^ sw2),
                                  tbase + rb3 + (dcoln ^ sw3));
              else
                bnext = Tr::tr16(tbase + rb0 + (dcoln ^ sw0),
                                  tbase + rb1 + (dcoln ^ sw1));
            }
            acc[j >> 1] = Tr::mfma((j & 1) ? a1 : a0, bcur, acc[j >> 1]);
            bcur = bnext;
          }
        };
        if constexpr (MODE == 1) {
          pipe_mm(do_base, Tr::afrag(pv, 0), Tr::afrag(pv, 1),
                  acc_dv);
        } else if constexpr (MODE == 2) {
          pipe_mm(q_base, Tr::afrag(dsv, 0), Tr::afrag(dsv, 1),
                  acc_dk);
        } else {
          // MODE 0 (fused dK+dV): INTERLEAVE the two independent MFMA
          // streams — each fragment load's LDS latency is covered by the
          // OTHER stream's in-flight MFMA, which a single serialized stream
          // cannot do (the allocator coalesces any explicit double-buffer
          // at this register pressure).
          vec8 pa0 = Tr::afrag(pv, 0);
          vec8 pa1 = Tr::afrag(pv, 1);
          vec8 da0 = Tr::afrag(dsv, 0);
          vec8 da1 = Tr::afrag(dsv, 1);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const int dcol = (dt * 32 + 16 * qhalf) * 2;
            vec8 bdo = Tr::tr16(do_base + rb0 + (dcol ^ sw0),
                                   do_base + rb1 + (dcol ^ sw1));
            acc_dv[dt] = Tr::mfma(pa0, bdo, acc_dv[dt]);
            vec8 bq = Tr::tr16(q_base + rb0 + (dcol ^ sw0),
                                  q_base + rb1 + (dcol ^ sw1));
            acc_dk[dt] = Tr::mfma(da0, bq, acc_dk[dt]);
            vec8 bdo1 = Tr::tr16(do_base + rb2 + (dcol ^ sw2),
                                    do_base + rb3 + (dcol ^ sw3));
            acc_dv[dt] = Tr::mfma(pa1, bdo1, acc_dv[dt]);
            vec8 bq1 = Tr::tr16(q_base + rb2 + (dcol ^ sw2),
                                   q_base + rb3 + (dcol ^ sw3));
            acc_dk[dt] = Tr::mfma(da1, bq1, acc_dk[dt]);
          }
        }
      }
    }
    }  // sub
    cur = (NBUF == 3) ? (cur == 2 ? 0 : cur + 1) : (cur ^ 1);
  }
  __syncthreads();  // this segment's LDS reads retired before restaging
  }  // seg

  // ---- write dK/dV ----
  if (wave_live) {
  if constexpr (DIRECT) {
    // single owner (disjoint k ranges; hq == hk, or CAT): the rounded tile
    // IS the row, zeros included - the number the atomic add into a zeroed f32
    // buffer followed by a cast gives. from_f32 rounds the finished f32
    // value. pin_vgpr on the dK tile in front of each row's converts changes
    // no value; it steers the register allocator: without it the 8-wave
    // d-128 dK-only kernel, which spills at the 256 cap, spills one dword
    // more than its atomic twin (profiles/bwd_direct_store.md).
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = n0 + crow(r, hi);
      if (kr >= ke) continue;
      ET* dkp = (ET*)p.dk + (size_t)kr * k_pitch + (size_t)kh * D + lo32;
      ET* dvp = (ET*)p.dv + (size_t)kr * k_pitch + (size_t)kh * D + lo32;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if constexpr (WANT_DK) pin_vgpr(acc_dk[dt]);
        if constexpr (WANT_DK) dkp[dt * 32] = Tr::from_f32(acc_dk[dt][r]);
        if constexpr (WANT_DV) dvp[dt * 32] = Tr::from_f32(acc_dv[dt][r]);
      }
    }
  } else {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kr = n0 + crow(r, hi);
    if (kr >= ke) continue;
    float* dkp = (float*)p.dk + (size_t)kr * k_pitch + (size_t)kh * D;
    float* dvp = (float*)p.dv + (size_t)kr * k_pitch + (size_t)kh * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if constexpr (WANT_DK) {
        if (acc_dk[dt][r] != 0.f)
          unsafeAtomicAdd(dkp + dt * 32 + lo32, acc_dk[dt][r]);
      }
      if constexpr (WANT_DV) {
        if (acc_dv[dt][r] != 0.f)
          unsafeAtomicAdd(dvp + dt * 32 + lo32, acc_dv[dt][r]);
      }
    }
  }
  }
  }  // wave_live store
  if constexpr (MODE == 0) break;  // single trip: kills the backedge (regs)
  }  // strided work loop
}


// ---------------- dQ pass ----------------
// q-outer: each wave owns a 32-row q tile and accumulates its dQ across the
// whole k loop IN REGISTERS, storing once at the end (atomicAdd only for the
// slice-overlap case) — eliminates the per-k-tile dq atomic storm, which the
// ablation measured at ~45% of a fused backward. K/V tiles are staged
// cooperatively per iteration (row-major swizzled for the S^T/dP^T A-frags,
// plus a transposed copy for the dQ B-frags).
// WAVES: q tiles per workgroup sharing ONE staged K/V image (4 or 8; the
// D=192 builds spill at 8 waves' 256-register cap and exist at 4 only).
// 8 waves run the 3-slot staging ring (see the dkv kernel note); 4 waves keep
// 2 slots (3 buffers exceed the 80 KB/WG budget of 2 blocks/CU).
// DIRECT: the epilogue (see the head of the file); nothing before it differs.
template <class ET, int D, bool HAS_SOFTCAP, int WAVES, bool DIRECT>
__global__ __launch_bounds__(64 * WAVES, WAVES == 8 ? 1 : 2)
void ffa_bwd_dq_kernel(BwdParams<ET> p) {
  using Tr = ElemTraits<ET>;
  using vec8 = typename Tr::x8;
  static_assert(WAVES == 4 || (WAVES == 8 && D != 192), "unsupported shape");
  constexpr int NBUF = WAVES == 8 ? 3 : 2;
  constexpr int DF = D / 16;
  constexpr int DT = D / 32;
  constexpr int ROWB = (D == 192) ? 512 : D * 2;  // padded pow2 LDS rows
  constexpr int ROWE = ROWB / 2;
  constexpr int VSLOTS = D / 8;
  constexpr int SW32M = ROWB / 32 - 1;  // 32-B-granular swizzle (tr16 reads)
  auto swz = [](int row, int byte_off) {
    return byte_off ^ ((row & SW32M) << 5);
  };
  // CU-margin strided-grid mode (see ffa_fwd.hip): margin>0 caps the grid
  // below the resident-WG count; each WG walks the flattened work space.
  const long long work_total =
      (long long)p.work_nx * p.work_ny * p.work_nz;
  const long long grid_span = (long long)gridDim.x * gridDim.y * gridDim.z;
  for (long long w = blockIdx.x +
           (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * blockIdx.z);
       w < work_total; w += grid_span) {
  const int wx = (int)(w % p.work_nx);
  const long long w2 = w / p.work_nx;
  const int wy = (int)(w2 % p.work_ny);
  const int wz = (int)(w2 / p.work_ny);
  const int ri = wz;
  const int h = p.head_major ? wx : wy;
  const int wb_lin = p.head_major ? wy : wx;
  const int qs = p.q_ranges[2 * ri], qe = p.q_ranges[2 * ri + 1];
  const int nqb = (qe - qs + BWD_BM * WAVES - 1) / (BWD_BM * WAVES);
  if (wb_lin >= nqb) continue;
  const int seg0 = p.seg_starts ? p.seg_starts[ri] : ri;
  const int seg1 = p.seg_starts ? p.seg_starts[ri + 1] : ri + 1;
  // causal / bi-causal: a q block's k loop grows with its row index, so hand
  // the range's blocks out last-first — longest work first leaves the short
  // blocks to fill the final, uneven round (the dkv pass gets this order by
  // construction). Keyed on the range's first k segment.
  const int at0 = p.attn_type_map ? p.attn_type_map[seg0] : 0;
  const int wb = (at0 == 1 || at0 == 3) ? nqb - 1 - wb_lin : wb_lin;
  const int mblk0 = qs + wb * (BWD_BM * WAVES);
  int ks, ke, atype;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // static priority for the second-dispatched half of an 8-wave WG: the
  // younger waves are the VALU-arbitration losers on every segment
  // (MI355X guide, two-waves-per-SIMD item 4)
  if (WAVES == 8 && wave >= 4) asm volatile("s_setprio 1");

  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  const int m0 = mblk0 + wave * BWD_BM;  // this wave's q tile
  const int qrow = m0 + lo32;
  const bool qvalid = qrow < qe && m0 < qe;
  const int qcl = qvalid ? qrow : (qe - 1);

  const float sl2 = HAS_SOFTCAP ? p.softcap * 1.4426950408889634f
                                : p.scale * 1.4426950408889634f;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;
  const float log2e = 1.4426950408889634f;

  const int kh = h / p.gqa;
  const size_t k_pitch = (size_t)p.hk * D;
  const size_t q_pitch = (size_t)p.hq * D;

  // single shared object (glds-pipeline trap, see dkv kernel).
  // 2 buffers x 64-row K/V images: one barrier per 64 k rows — the doubled
  // compute phase covers the prefetch latency a 32-row phase could not, with
  // HALF the barrier parking (PMC: SQ_WAIT_ANY 36% at 32-row iterations).
  constexpr int KITER = 2 * BWD_BN;
  static_assert(NBUF * 2 * KITER * ROWB <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * KITER * ROWB];
  auto lds_k = [&](int buf) -> ET* {
    return (ET*)(smem + (2 * buf) * KITER * ROWB);
  };
  auto lds_v = [&](int buf) -> ET* {
    return (ET*)(smem + (2 * buf + 1) * KITER * ROWB);
  };

  // persistent per-wave operands: Q and dO fragments (B-layout rows)
  vec8 qf[DF], dof[DF];
  {
    const ET* qp = p.q + (size_t)qcl * q_pitch + (size_t)h * D;
    const ET* dp = p.dout + (size_t)qcl * q_pitch + (size_t)h * D;
#pragma unroll
    for (int dd = 0; dd < DF; ++dd) {
      qf[dd] = *(const vec8*)(qp + dd * 16 + hi * 8);
      dof[dd] = *(const vec8*)(dp + dd * 16 + hi * 8);
    }
  }
  float lse_q = qvalid ? p.lse[(size_t)qrow * p.hq + h] : INFINITY;
  float dpsum_q = qvalid ? p.dpsum[(size_t)qrow * p.hq + h] : 0.f;
  const bool row_live = qvalid && lse_q != INFINITY && lse_q != -INFINITY;

  // block + wave k-loop bounds (recomputed per k segment)
  const int mlast = min(mblk0 + BWD_BM * WAVES, qe) - 1;
  int k_lo = 0, k_hi = 0, wk_lo = 0, wk_hi = 0;
  auto seg_bounds = [&]() {
    k_lo = ks; k_hi = ke;
    if (atype == 1 || atype == 3) k_hi = min(k_hi, mlast + (ke - qe) + 1);
    if (atype == 2 || atype == 3) k_lo = max(k_lo, mblk0 + (ks - qs));
    wk_lo = ks; wk_hi = ke;
    if (atype == 1 || atype == 3)
      wk_hi = min(wk_hi, min(m0 + BWD_BM, qe) - 1 + (ke - qe) + 1);
    if (atype == 2 || atype == 3) wk_lo = max(wk_lo, m0 + (ks - qs));
  };

  f32x16 acc_dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_dq[dt] = (f32x16)(0.f);

  constexpr int ROWS_PER_GLDS = 1024 / ROWB;
  static_assert(KITER / WAVES >= ROWS_PER_GLDS, "stage rows per wave");
  constexpr int GLDS_PER_WAVE = (KITER / WAVES) / ROWS_PER_GLDS;
  const int smem_byte = (int)(unsigned long long)(
      (__attribute__((address_space(3))) const char*)smem);
  // Issued outside the compiler's waitcnt tracking (glds16_untracked): the
  // counted wait of pipe_barrier is the ONLY thing that orders the ring, and
  // drain_vm() at the end of each k segment owns the drain.
  auto stage_glds = [&](int buf, int n0x) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (KITER / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + lane / (ROWB / 16);
      const int c = lane % (ROWB / 16);
      const int kr = min(n0x + r, ke - 1);
      int cs = c ^ ((r & SW32M) << 1);
      if (cs >= VSLOTS) cs = 0;
      const int csw = cs * 8;
      const int lk = smem_byte + (2 * buf * KITER + r0) * ROWB;
      glds16_untracked(p.k + (size_t)kr * k_pitch + (size_t)kh * D + csw, lk);
      glds16_untracked(p.v + (size_t)kr * k_pitch + (size_t)kh * D + csw,
                       lk + KITER * ROWB);
    }
  };

  constexpr int GOPS = 2 * GLDS_PER_WAVE;  // vm ops per stage per wave
  int cur = 0;
  for (int seg = seg0; seg < seg1; ++seg) {
  ks = p.k_ranges[2 * seg];
  ke = p.k_ranges[2 * seg + 1];
  atype = p.attn_type_map ? p.attn_type_map[seg] : 0;
  if (ke <= ks) continue;  // uniform across block
  seg_bounds();
  if (k_lo >= k_hi) continue;
  cur = 0;
  stage_glds(0, k_lo);
  if constexpr (NBUF == 3) stage_glds(1, k_lo + KITER);  // rows clamp to ke-1
  // Q/dO fragments, lse and dpsum are the only compiler-tracked vector-memory
  // loads of a work item. Pin the compiler's wait for them HERE, outside the
  // k loop: placed at their first use it would sit inside the loop as a
  // vmcnt(0) per iteration. (It also drains the two prologue stages, which
  // the first barrier is about to wait for anyway.)
#pragma unroll
  for (int dd = 0; dd < DF; ++dd) {
    pin_vgpr(qf[dd]);
    pin_vgpr(dof[dd]);
  }
  pin_vgpr(lse_q);
  pin_vgpr(dpsum_q);

  for (int n0 = k_lo; n0 < k_hi; n0 += KITER) {
    // vmcnt accounting (per wave; the counter retires in issue order): after
    // stage(cur) this wave has issued exactly one more stage, GOPS ops, and
    // nothing else — the k loop holds no other vector-memory op, and the dq
    // atomics of the previous strided work item are older than both stages.
    // NBUF=3: vmcnt(GOPS) therefore retires buf[cur] and keeps the next
    // stage in flight; prefetch two ahead (clamped). NBUF=2: full drain.
    pipe_barrier<NBUF == 3 ? GOPS : 0>();
    if constexpr (NBUF == 3) {
      stage_glds(cur == 0 ? 2 : cur - 1, n0 + 2 * KITER);
    } else {
      if (n0 + KITER < k_hi) stage_glds(cur ^ 1, n0 + KITER);
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
    const int ns = n0 + sub * BWD_BN;
    if (ns >= k_hi) break;  // k_hi is block-uniform
    const ET* lkb = lds_k(cur) + sub * BWD_BN * ROWE;
    const ET* lvb = lds_v(cur) + sub * BWD_BN * ROWE;

    if (wave_alive(m0, qe) && ns + BWD_BN > wk_lo && ns < wk_hi) {
      // ---- S^T = K Q^T ; dP^T = V dO^T (K/V A-frags from LDS rows) ----
      // software-pipelined: the K/V fragment pair of step dd+1 is issued
      // under the two MFMAs of step dd; the sched_group_barriers hold that
      // order against the scheduler
      f32x16 sA = (f32x16)(0.f), dpA = (f32x16)(0.f);
      {
        const int off0 = swz(lo32, lo32 * ROWB + hi * 16);
        vec8 kf = *(const vec8*)((const char*)lkb + off0);
        vec8 vf = *(const vec8*)((const char*)lvb + off0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read x2
#pragma unroll
        for (int dd = 0; dd < DF; ++dd) {
          vec8 kn = kf, vn = vf;
          if (dd + 1 < DF) {
            const int off = swz(lo32, lo32 * ROWB + (dd + 1) * 32 + hi * 16);
            kn = *(const vec8*)((const char*)lkb + off);
            vn = *(const vec8*)((const char*)lvb + off);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          }
          sA = Tr::mfma(kf, qf[dd], sA);
          dpA =
              Tr::mfma(vf, dof[dd], dpA);
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA x2
          kf = kn;
          vf = vn;
        }
      }

      float dsv[16];
      const bool interior =
          (qrow < qe) && row_live && (ns >= ks) && (ns + BWD_BN <= ke) &&
          !((atype == 1 || atype == 3) && (ns + BWD_BN - 1 > m0 + (ke - qe))) &&
          !((atype == 2 || atype == 3) && (ns < m0 + 31 + (ks - qs)));
      if (__all(interior) && !HAS_SOFTCAP) {
        const float lsc = lse_q * log2e;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pij = fast_exp2(sA[r] * sl2 - lsc);
          dsv[r] = pij * (dpA[r] - dpsum_q) * p.scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = ns + crow(r, hi);
          bool ok = row_live && kk < ke && kk >= ks;
          if (atype == 1 || atype == 3) ok = ok && (kk - qrow <= ke - qe);
          if (atype == 2 || atype == 3) ok = ok && (kk - qrow >= ks - qs);
          float sv = sA[r];
          float dscale = p.scale;
          float t;
          if (HAS_SOFTCAP) {
            const float th = tanhf(sv * cap_pre);
            t = th * sl2;
            dscale = p.scale * (1.f - th * th);
          } else {
            t = sv * sl2;
          }
          const float pij = ok ? fast_exp2(t - lse_q * log2e) : 0.f;
          dsv[r] = pij * (dpA[r] - dpsum_q) * dscale;
        }
      }

      // ---- dq += dS K (B-frags from the transposed K tile) ----
      vec8 dsa0 = Tr::afrag(dsv, 0);
      vec8 dsa1 = Tr::afrag(dsv, 1);
      // B-frags (B[kk=k][j=d]) via tr16 straight off the K row image
      // (same recipe as the dkv kernel)
      {
        const int qhalf2 = (lane >> 4) & 1;
        const int jrow = (lane & 15) >> 2;
        const int row0 = 8 * hi + jrow;
        const int row1 = 8 * hi + 4 + jrow;
        const int k_base = (int)(unsigned long long)(
            (__attribute__((address_space(3))) const char*)lkb);
        const int lane8 = (lane & 3) * 8;
        const int sw0 = (row0 & SW32M) << 5;
        const int sw1 = (row1 & SW32M) << 5;
        const int rb0 = row0 * ROWB + lane8;
        const int rb1 = row1 * ROWB + lane8;
        const int sw2 = ((row0 + 16) & SW32M) << 5;
        const int sw3 = ((row1 + 16) & SW32M) << 5;
        const int rb2 = (row0 + 16) * ROWB + lane8;
        const int rb3 = (row1 + 16) * ROWB + lane8;
        // software-pipelined: step j+1's fragment reads issue under step j's
        // MFMA so the ~50-cycle LDS latency hides under the matrix op (the
        // serialized read->wait->mfma form parks the wave per fragment).
        // The sched_group_barriers hold the order: without them the
        // scheduler sinks each tr16 pair back in front of its own MFMA.
        vec8 bcur = Tr::tr16(k_base + rb0 + ((16 * qhalf2 * 2) ^ sw0),
                                k_base + rb1 + ((16 * qhalf2 * 2) ^ sw1));
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read x2
#pragma unroll
        for (int j = 0; j < 2 * DT; ++j) {
          vec8 bnext = bcur;
          if (j + 1 < 2 * DT) {
            const int dcoln = (((j + 1) >> 1) * 32 + 16 * qhalf2) * 2;
            if ((j + 1) & 1)
              bnext = Tr::tr16(k_base + rb2 + (dcoln ^ sw2),
                                k_base + rb3 + (dcoln ^ sw3));
            else
              bnext = Tr::tr16(k_base + rb0 + (dcoln ^ sw0),
                                k_base + rb1 + (dcoln ^ sw1));
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          }
          acc_dq[j >> 1] = Tr::mfma((j & 1) ? dsa1 : dsa0, bcur, acc_dq[j >> 1]);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA x1
          bcur = bnext;
        }
      }
    }
    }  // sub
    cur = (NBUF == 3) ? (cur == 2 ? 0 : cur + 1) : (cur ^ 1);
  }
  // End of a k segment: up to two clamped-row prefetches are still in flight
  // (NBUF=3) and nothing else waits for them — drain by hand, then barrier so
  // every wave's LDS reads are retired before the next segment, the next
  // strided work item or nobody (kernel end) restages the ring.
  drain_vm();
  __syncthreads();
  }  // seg

  // ---- store dq once (atomicAdd: q_ranges of different slices may overlap;
  // DIRECT: the caller promises they do not, see the dkv epilogue) ----
  if constexpr (DIRECT) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = m0 + crow(r, hi);
      if (qr >= qe) continue;
      ET* dst = (ET*)p.dq + (size_t)qr * q_pitch + (size_t)h * D + lo32;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        dst[dt * 32] = Tr::from_f32(acc_dq[dt][r]);
    }
  } else {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = m0 + crow(r, hi);
    if (qr >= qe) continue;
    float* dst = (float*)p.dq + (size_t)qr * q_pitch + (size_t)h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const float val = acc_dq[dt][r];
      if (val != 0.f) unsafeAtomicAdd(dst + dt * 32 + lo32, val);
    }
  }
  }
  }  // strided work loop
}


// ---------------- launchers ----------------
// Every entry is a template over the element type behind one extern "C"
// function that picks the instantiation from args->elem_type.
#define BY_ELEM_TYPE(a, fn, ...)                                       \
  ((a) && (a)->elem_type == MAGI_FFA_ELEM_FP16 ? fn<f16_t>(a, ##__VA_ARGS__) \
                                               : fn<bf16_t>(a, ##__VA_ARGS__))

template <class ET>
static int bwd_preprocess(const magi_ffa_bwd_args* a) {
  if (!a || !a->dout || !a->out || !a->dpsum) return -1;
  if (!elem_type_known(a->elem_type)) return -9;
  BwdParams<ET> p{};
  p.dout = (const ET*)a->dout;
  p.out = a->out;
  p.dpsum = a->dpsum;
  const long long n_rows = a->total_q * a->hq;
  if (n_rows == 0) return 0;
  dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)a->stream;
  if (a->out_is_fp32)
    hipLaunchKernelGGL((bwd_preprocess_kernel<ET, true>), grid, block, 0, s,
                       p, a->d, n_rows);
  else
    hipLaunchKernelGGL((bwd_preprocess_kernel<ET, false>), grid, block, 0, s,
                       p, a->d, n_rows);
  return (int)hipGetLastError();
}

extern "C" int magi_ffa_bwd_preprocess(const magi_ffa_bwd_args* a) {
  return BY_ELEM_TYPE(a, bwd_preprocess);
}

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

template <class ET, int D, bool DIRECT>
static void launch_dq(int waves, bool sc, dim3 grid, hipStream_t s,
                      const BwdParams<ET>& p) {
#define GO(SC, W)                                                        \
  hipLaunchKernelGGL((ffa_bwd_dq_kernel<ET, D, SC, W, DIRECT>), grid,    \
                     dim3(64 * W), 0, s, p)
  if constexpr (D != 192) {  // D=192 spills at 8 waves: 4-wave builds only
    if (waves == 8) {
      if (sc) GO(true, 8); else GO(false, 8);
      return;
    }
  }
  if (sc) GO(true, 4); else GO(false, 4);
#undef GO
}

template <class ET>
static int bwd_dq(const magi_ffa_bwd_args* a, bool direct_store) {
  BwdParams<ET> p;
  int rc = fill_bwd_params(a, &p, DkvOpts{false, false, 0});
  if (rc) return rc > 0 ? 0 : rc;
  const BwdKnobs knobs = dq_knobs(a);
  p.head_major = knobs.head_major;
  const int W = (a->d != 192 && a->max_seqlen_k >= knobs.bigseq) ? 8 : 4;
  if (a->n_ranges > 65535) return -5;
  const int qspan = BWD_BM * W;
  const int qblocks = (int)((a->total_q + qspan - 1) / qspan);
  dim3 grid = p.head_major ? dim3(a->hq, qblocks, (unsigned)a->n_ranges)
                           : dim3(qblocks, a->hq, (unsigned)a->n_ranges);
  p.work_nx = grid.x; p.work_ny = grid.y; p.work_nz = grid.z;
  grid = cap_grid(grid, a->cu_margin & 0xFFFF, W == 4 ? 2 : 1);
  hipStream_t s = (hipStream_t)a->stream;
  const bool sc = a->softcap > 0.f;
  auto go = [&](auto direct) {
    constexpr bool DIRECT = decltype(direct)::value;
    if (a->d == 64) launch_dq<ET, 64, DIRECT>(W, sc, grid, s, p);
    else if (a->d == 192) launch_dq<ET, 192, DIRECT>(W, sc, grid, s, p);
    else launch_dq<ET, 128, DIRECT>(W, sc, grid, s, p);
  };
  if (direct_store) go(std::true_type{}); else go(std::false_type{});
  return (int)hipGetLastError();
}

extern "C" int magi_ffa_bwd_dq(const magi_ffa_bwd_args* a) {
  return BY_ELEM_TYPE(a, bwd_dq, false);
}

static BwdKnobs dkv_knobs() {
  // dkv passes win head-major at EVERY measured size (their dk/dv atomics
  // cluster per head in one XCD's L2): 1.54x at 16k, 1.10x at 64k, 1.07x
  // at 128k (profiles/r2_headmajor_ab.md) — unconditional unless A/B'd.
  // All dkv modes run 8 waves per WG (one 512-thread WG/CU, one shared
  // staged Q/dO image) down to 1k ranges: these kernels' blocks span the
  // K dim, so the wider workgroup does NOT over-iterate causal q windows,
  // and halving the staging streams is a 50-60% win even on 2k varlen docs
  // (r2 A/B: dv 0.71->0.48 ms, dk 0.90->0.56, fused 1.37->0.92; PMC r2: dV
  // at W4 fetched 174 GB/launch vs dK-W8's 71).
  return {env_int("MAGI_BWD_HEAD_MAJOR", 1), env_int("MAGI_BWD_BIGSEQ", 1024)};
}

template <class ET, int D, int MODE, bool DIRECT, bool CAT>
static void launch_dkv(int waves, bool sc, dim3 grid, hipStream_t s,
                       const BwdParams<ET>& p) {
#define GO(SC, W)                                                          \
  hipLaunchKernelGGL((ffa_bwd_dkv_kernel<ET, D, SC, MODE, W, DIRECT, CAT>), \
                     grid, dim3(64 * W), 0, s, p)
  if constexpr (D != 192) {  // D=192 spills at 8 waves: 4-wave builds only
    if (waves == 8) {
      if (sc) GO(true, 8); else GO(false, 8);
      return;
    }
  }
  if (sc) GO(true, 4); else GO(false, 4);
#undef GO
}

template <class ET, int MODE>
static int launch_bwd_dkv(const magi_ffa_bwd_args* a, const DkvOpts& o) {
  BwdParams<ET> p;
  int rc = fill_bwd_params(a, &p, o);
  if (rc) return rc > 0 ? 0 : rc;
  const BwdKnobs knobs = dkv_knobs();
  p.head_major = knobs.head_major;
  const int W = (a->d != 192 && a->max_seqlen_k >= knobs.bigseq) ? 8 : 4;
  const int span = BWD_BN * W;
  const int nblocks = (a->max_seqlen_k + span - 1) / span;
  if (a->n_ranges > 65535) return -5;
  dim3 grid = p.head_major
                  ? dim3(p.n_heads_launch, nblocks, (unsigned)a->n_ranges)
                  : dim3(nblocks, p.n_heads_launch, (unsigned)a->n_ranges);
  p.work_nx = grid.x; p.work_ny = grid.y; p.work_nz = grid.z;
  // the fused kernel's work loop is single-trip (see kernel): never capped
  if constexpr (MODE != 0)
    grid = cap_grid(grid, a->cu_margin & 0xFFFF, W == 4 ? 2 : 1);
  hipStream_t s = (hipStream_t)a->stream;
  const bool sc = a->softcap > 0.f;
  // fused + D=192 exceeds LDS; the host routes that head dim to the split
  if (MODE == 0 && a->d == 192) return -6;
  auto go = [&](auto direct, auto cat) {
    constexpr bool DIRECT = decltype(direct)::value;
    constexpr bool CAT = decltype(cat)::value;
    if (a->d == 64) launch_dkv<ET, 64, MODE, DIRECT, CAT>(W, sc, grid, s, p);
    else if (a->d == 192) {
      if constexpr (MODE != 0)
        launch_dkv<ET, 192, MODE, DIRECT, CAT>(W, sc, grid, s, p);
    } else launch_dkv<ET, 128, MODE, DIRECT, CAT>(W, sc, grid, s, p);
  };
  auto go_cat = [&](auto direct) {
    if (p.cat > 1) go(direct, std::true_type{});
    else go(direct, std::false_type{});
  };
  if (o.direct) go_cat(std::true_type{}); else go_cat(std::false_type{});
  return (int)hipGetLastError();
}

template <class ET>
static int bwd_dkv(const magi_ffa_bwd_args* a, const DkvOpts& o) {
  return launch_bwd_dkv<ET, 0>(a, o);
}
template <class ET>
static int bwd_dv(const magi_ffa_bwd_args* a, const DkvOpts& o) {
  return launch_bwd_dkv<ET, 1>(a, o);
}
template <class ET>
static int bwd_dk(const magi_ffa_bwd_args* a, const DkvOpts& o) {
  return launch_bwd_dkv<ET, 2>(a, o);
}

extern "C" int magi_ffa_bwd_dkv(const magi_ffa_bwd_args* a) {
  return BY_ELEM_TYPE(a, bwd_dkv, DkvOpts{false, false, 0});
}

extern "C" int magi_ffa_bwd_dv(const magi_ffa_bwd_args* a) {
  return BY_ELEM_TYPE(a, bwd_dv, DkvOpts{false, false, 0});
}

extern "C" int magi_ffa_bwd_dk(const magi_ffa_bwd_args* a) {
  return BY_ELEM_TYPE(a, bwd_dk, DkvOpts{false, false, 0});
}

extern "C" int magi_ffa_bwd(const magi_ffa_bwd_args* a) {
  // sequential convenience form: dq pass then dkv pass on one stream
  int rc = magi_ffa_bwd_dq(a);
  if (rc) return rc;
  return magi_ffa_bwd_dkv(a);
}

// The same passes with the epilogue chosen per pass by the two members behind
// the embedded struct (magi_ffa.h); a null d is the null-pointer code.
extern "C" int magi_ffa_bwd_dq_direct(const magi_ffa_bwd_direct_args* d) {
  if (!d) return -1;
  return BY_ELEM_TYPE(&d->args, bwd_dq, d->dq_is_16bit != 0);
}

static DkvOpts direct_opts(const magi_ffa_bwd_direct_args* d) {
  return DkvOpts{d->dkv_is_16bit != 0, false, 0};
}

extern "C" int magi_ffa_bwd_dkv_direct(const magi_ffa_bwd_direct_args* d) {
  if (!d) return -1;
  return BY_ELEM_TYPE(&d->args, bwd_dkv, direct_opts(d));
}

extern "C" int magi_ffa_bwd_dv_direct(const magi_ffa_bwd_direct_args* d) {
  if (!d) return -1;
  return BY_ELEM_TYPE(&d->args, bwd_dv, direct_opts(d));
}

extern "C" int magi_ffa_bwd_dk_direct(const magi_ffa_bwd_direct_args* d) {
  if (!d) return -1;
  return BY_ELEM_TYPE(&d->args, bwd_dk, direct_opts(d));
}

extern "C" int magi_ffa_bwd_direct_args_size(void) {
  return (int)sizeof(magi_ffa_bwd_direct_args);
}

// The dkv passes once more behind magi_ffa_bwd_cat_args (magi_ffa.h): with
// cat_gqa == 0 the _direct entries, reserved unread.
static DkvOpts cat_opts(const magi_ffa_bwd_cat_args* c) {
  if (!c->cat_gqa) return direct_opts(&c->direct);
  return DkvOpts{c->direct.dkv_is_16bit != 0, true, c->reserved};
}

extern "C" int magi_ffa_bwd_dkv_cat(const magi_ffa_bwd_cat_args* c) {
  if (!c) return -1;
  return BY_ELEM_TYPE(&c->direct.args, bwd_dkv, cat_opts(c));
}

extern "C" int magi_ffa_bwd_dv_cat(const magi_ffa_bwd_cat_args* c) {
  if (!c) return -1;
  return BY_ELEM_TYPE(&c->direct.args, bwd_dv, cat_opts(c));
}

extern "C" int magi_ffa_bwd_dk_cat(const magi_ffa_bwd_cat_args* c) {
  if (!c) return -1;
  return BY_ELEM_TYPE(&c->direct.args, bwd_dk, cat_opts(c));
}

extern "C" int magi_ffa_bwd_cat_args_size(void) {
  return (int)sizeof(magi_ffa_bwd_cat_args);
}
