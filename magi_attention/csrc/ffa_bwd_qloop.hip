// ffa_bwd_qloop.hip — dense flex-flash-attention backward in ONE q-outer pass
// (swap_bwd_qk_loop: the reference's "Q for outer-loop and K for inner-loop",
// flex_flash_attn.py:1216). gfx950.
//
// The two-pass backward of ffa_bwd.hip walks the range table twice and
// recomputes S and dP in both passes (3 + 4 matmuls per tile). Here one
// workgroup of 4 waves owns the unit the dQ kernel owns, (q range or unique q
// range, q head, block of 128 q rows), walks the unit's k segments once and
// produces all three gradients with 5 matmuls per tile. The design is the one
// of the token-gather backward (ffa_index_bwd.hip), its M dimension q rows of
// a range in place of the query heads of a token:
//
//   once per work item
//     Q and dO rows of the block -> two swizzled LDS images (LDS-DMA), and
//     each wave's own 32 rows once more as B-fragments in registers, with the
//     rows' lse and dpsum. dQ accumulator in registers, single owner.
//   per 32-row k tile (K/V staged by LDS-DMA into a 2-slot swizzled ring)
//     phase 1, each wave on its own 32 q rows:
//       S^T = K Q^T ; dP^T = V dO^T      (lane = q row, registers = k rows)
//       P^T, dS^T in base 2: the four mask types per element, the dead-row
//       rule (lse = +-inf), softcap
//       dQ += dS K                       (K B-fragments by tr16 reads)
//       P^T, dS^T rounded to the element type -> exchange image [q row][k row]
//     phase 2, the 2 * D / 32 output tiles (dV and dK, 32 k rows x 32 columns)
//     dealt over the waves:
//       dV_tile = P^T dO ; dK_tile = dS^T Q, contracted over ALL 128 q rows of
//       the workgroup: A-fragments by tr16 reads off the exchange image,
//       B-fragments by tr16 reads off the dO / Q images. The cross-wave
//       reduction happens inside the MFMA k loop, so one f32 atomic goes out
//       per non-zero element and k tile whatever the wave count.
//   epilogue: dQ once, f32 atomic or (DIRECT) a 16-bit store.
//
// One pipeline per work item, not per segment: the tiles of all live k
// segments form one sequence (next_seg / advance below, block-uniform), and
// the stage of tile t + 1 is issued under tile t whether or not it belongs to
// the same segment. A table of 16-row k blocks therefore pays no ring restart
// and no drain per block, only tiles that are half empty (packing them is the
// business of a sparse_load variant, not built).
//
// Barriers, two per tile. Top: vmcnt(0) + lgkmcnt(0) + s_barrier. The stage
// of this tile has landed (and on the first trip the Q/dO images), and every
// wave is past phase 2 of the previous tile, so the exchange image and the
// other ring slot are free. Middle: lgkmcnt(0) + s_barrier, LDS only: the
// exchange image is complete; the prefetch stays in flight. A wave that skips
// phase 1 (no q row, or the tile lies outside its causal window) writes zeros
// into its slice of the image first: phase 2 reads every slice.
//
// Vector memory. The stage loads are issued outside the compiler's waitcnt
// tracking (glds16_untracked); the top barrier's vmcnt(0) is what retires
// them. The dK/dV atomics are vector-memory ops too and would be waited for
// by that vmcnt(0) right after they were issued, so a tile's two output
// tiles stay in registers across the barrier and are added at the START of
// the next tile, in front of its prefetch: atomics and prefetch then both
// have a whole tile to complete before the next vmcnt(0). The k loop holds no
// tracked load: Q/dO fragments, lse and dpsum are pinned before it and the
// table reads are scalar.
//
// LDS at D = 128: Q and dO images 64 KB, ring 2 x (K + V) x 32 rows = 32 KB,
// exchange image 2 x 128 x 72 B = 18 KB: 114 KB, one workgroup per CU, one
// wave per SIMD with the whole register file.

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/magi_ffa.h"
#include "ffa_bwd_common.h"
#include "ffa_device.h"

#define QL_WAVES 4
#define QL_TN 32  // k rows per tile

// One k tile of the work item's sequence: its segment's range and type, the
// tile's first row, the block's upper bound in the segment and this wave's
// own window (wave-uniform; everything else is block-uniform)
struct QlTile {
  int ks, ke, atype, n0, k_hi, wk_lo, wk_hi;
};

// Scalar loads of one and two table entries at a block-uniform address, with
// their own lgkmcnt wait. Written as C++, these reads compile to vector loads
// (the atomics may alias the tables for all the compiler knows, which rules
// the scalar cache out), and the vmcnt(0) in front of their first use would
// wait for the atomics and the prefetch just issued at every segment switch.
// The tables are read-only for the kernel, so the scalar cache is safe.
DEV_INLINE int sload1(const int* ptr) {
  int v;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)"
               : "=s"(v) : "s"(ptr) : "memory");
  return v;
}

DEV_INLINE void sload2(const int* ptr, int& a, int& b) {
  typedef int i32x2_ __attribute__((ext_vector_type(2)));
  i32x2_ v;
  asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)"
               : "=s"(v) : "s"(ptr) : "memory");
  a = v[0];
  b = v[1];
}

template <class ET, int D, bool HAS_SOFTCAP, bool DIRECT>
__global__ __launch_bounds__(64 * QL_WAVES)
void ffa_bwd_qloop_kernel(BwdParams<ET> p) {
  using Tr = ElemTraits<ET>;
  using vec8 = typename Tr::x8;
  static_assert(D == 64 || D == 128, "built for head dims 64 and 128");
  constexpr int WAVES = QL_WAVES;
  constexpr int HB = BWD_BM * WAVES;  // q rows per workgroup
  constexpr int DF = D / 16;
  constexpr int DT = D / 32;
  constexpr int ROWB = D * 2;
  constexpr int SW32M = ROWB / 32 - 1;  // 32-B-granular swizzle (tr16 reads)
  auto swz = [](int row, int byte_off) {
    return byte_off ^ ((row & SW32M) << 5);
  };

  // ---- LDS (ONE shared object, see ffa_bwd.hip) ----
  //   [Q image | dO image]  HB rows x ROWB, swizzled, staged once per item
  //   [K0 | V0 | K1 | V1]   QL_TN rows x ROWB each
  //   [P^T | dS^T]          HB rows x 72 B: 32 k columns per q row; the 8-B
  //                         pad makes the per-lane 8-B row writes
  //                         bank-conflict-free (pitch 18 dwords)
  constexpr int XP = 72;
  constexpr int QIMG = HB * ROWB;
  constexpr int KVIMG = QL_TN * ROWB;
  constexpr int OFF_Q = 0;
  constexpr int OFF_DO = QIMG;
  constexpr int OFF_KV = 2 * QIMG;
  constexpr int OFF_PT = OFF_KV + 4 * KVIMG;
  constexpr int OFF_DST = OFF_PT + HB * XP;
  constexpr int LDS_BYTES = OFF_DST + HB * XP;
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
  const int lds_base = (int)(unsigned long long)(
      (__attribute__((address_space(3))) const char*)smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // in a scalar register: the wave's windows, its phase-2 units and every
  // branch on them are then uniform to the compiler as well
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  constexpr int ROWS_PER_GLDS = 1024 / ROWB;
  const int g_r = lane / (ROWB / 16);  // row within one 1-KB glds group
  const int g_c = lane % (ROWB / 16);  // 16-B slot within the row

  // tr16 fragment off a row image (ffa_index_bwd.hip): k-step tt (16 image
  // rows = MFMA k dim), 32 image columns from byte `colb` (= M or N dim).
  // swm = 32-B swizzle mask of the image (0: unswizzled).
  const int qhalf = (lane >> 4) & 1;
  const int jrow = (lane & 15) >> 2;
  const int lane8 = (lane & 3) * 8;
  auto tr_frag = [&](int img, int pitch, int swm, int tt, int colb) -> vec8 {
    const int row0 = 16 * tt + 8 * hi + jrow;
    const int row1 = row0 + 4;
    const int cb = colb + 32 * qhalf;
    return Tr::tr16(img + row0 * pitch + lane8 + (cb ^ ((row0 & swm) << 5)),
                    img + row1 * pitch + lane8 + (cb ^ ((row1 & swm) << 5)));
  };

  // phase-2 work units: (matrix, d-tile), matrix 0 = dV, 1 = dK. A wave's
  // units are d-tiles of ONE matrix, so they share their A-fragments.
  static_assert((2 * DT) % WAVES == 0, "units per wave");
  constexpr int UPW = 2 * DT / WAVES;
  static_assert(DT % UPW == 0, "a wave's units belong to one matrix");
  const bool is_dk = wave * UPW >= DT;  // wave-uniform
  const int dt0 = wave * UPW - (is_dk ? DT : 0);

  const float log2e = 1.4426950408889634f;
  const float sl2 = HAS_SOFTCAP ? p.softcap * log2e : p.scale * log2e;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;
  const size_t k_pitch = (size_t)p.hk * D;
  const size_t q_pitch = (size_t)p.hq * D;

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
  const int ri = (int)(w2 / p.work_ny);
  const int h = p.head_major ? wx : wy;
  const int wb_lin = p.head_major ? wy : wx;
  const int qs = p.q_ranges[2 * ri], qe = p.q_ranges[2 * ri + 1];
  const int nqb = (qe - qs + HB - 1) / HB;
  if (wb_lin >= nqb) continue;  // block-uniform, as every branch around a barrier
  const int seg0 = p.seg_starts ? p.seg_starts[ri] : ri;
  const int seg1 = p.seg_starts ? p.seg_starts[ri + 1] : ri + 1;
  // causal / bi-causal: longest q blocks first (see the dQ kernel)
  const int at0 = p.attn_type_map ? p.attn_type_map[seg0] : 0;
  const int wb = (at0 == 1 || at0 == 3) ? nqb - 1 - wb_lin : wb_lin;
  const int mblk0 = qs + wb * HB;
  const int mlast = min(mblk0 + HB, qe) - 1;

  const int m0 = mblk0 + wave * BWD_BM;  // this wave's q tile
  const int qrow = m0 + lo32;
  const bool qvalid = qrow < qe;
  const int qcl = qvalid ? qrow : (qe - 1);
  const int kh = h / p.gqa;

  // ---- this wave's 32 rows of the Q and dO images (rows clamp to qe - 1:
  // their P and dS are zero, so what they hold only has to be finite) ----
#pragma unroll
  for (int gi = 0; gi < BWD_BM / ROWS_PER_GLDS; ++gi) {
    const int r0 = BWD_BM * wave + ROWS_PER_GLDS * gi;
    const int r = r0 + g_r;
    const int row = min(mblk0 + r, qe - 1);
    const int cs = g_c ^ ((r & SW32M) << 1);
    const size_t src = (size_t)row * q_pitch + (size_t)h * D + cs * 8;
    glds16_untracked(p.q + src, lds_base + OFF_Q + r0 * ROWB);
    glds16_untracked(p.dout + src, lds_base + OFF_DO + r0 * ROWB);
  }

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
  const float lsc = row_live ? lse_q * log2e : 0.f;

  f32x16 acc_dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_dq[dt] = (f32x16)(0.f);

  // ---- the work item's tile sequence ----
  QlTile nx;
  int seg = seg0 - 1;
  // first tile of the next segment in which this BLOCK has work
  auto next_seg = [&]() -> bool {
    while (++seg < seg1) {
      int ks, ke;
      sload2(p.k_ranges + 2 * seg, ks, ke);
      const int atype = p.attn_type_map ? sload1(p.attn_type_map + seg) : 0;
      if (ke <= ks) continue;
      int k_lo = ks, k_hi = ke, wk_lo = ks, wk_hi = ke;
      if (atype == 1 || atype == 3) {
        k_hi = min(k_hi, mlast + (ke - qe) + 1);
        wk_hi = min(wk_hi, min(m0 + BWD_BM, qe) - 1 + (ke - qe) + 1);
      }
      if (atype == 2 || atype == 3) {
        k_lo = max(k_lo, mblk0 + (ks - qs));
        wk_lo = max(wk_lo, m0 + (ks - qs));
      }
      if (k_lo >= k_hi) continue;
      nx = QlTile{ks, ke, atype, k_lo, k_hi, wk_lo, wk_hi};
      return true;
    }
    return false;
  };
  auto advance = [&]() -> bool {
    nx.n0 += QL_TN;
    return nx.n0 < nx.k_hi || next_seg();
  };

  // K/V stage of tile t: rows past the segment end clamp to ke - 1 (masked in
  // the math; their dK/dV rows are guarded at the atomics)
  static_assert(QL_TN / WAVES >= ROWS_PER_GLDS, "stage rows per wave");
  constexpr int GLDS_PER_WAVE = (QL_TN / WAVES) / ROWS_PER_GLDS;
  auto stage_kv = [&](int buf, const QlTile& t) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (QL_TN / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + g_r;
      const int kr = min(t.n0 + r, t.ke - 1);
      const int cs = g_c ^ ((r & SW32M) << 1);
      const size_t src = (size_t)kr * k_pitch + (size_t)kh * D + cs * 8;
      const int lk = lds_base + OFF_KV + 2 * buf * KVIMG + r0 * ROWB;
      glds16_untracked(p.k + src, lk);
      glds16_untracked(p.v + src, lk + KVIMG);
    }
  };

  // the previous tile's output tiles, added one tile late (see the head)
  f32x16 pacc[UPW];
  QlTile pend{};
  bool has_pend = false;
  auto flush = [&]() {
#pragma unroll
    for (int ui = 0; ui < UPW; ++ui) {
      float* dst = (float*)(is_dk ? p.dk : p.dv) + (size_t)kh * D +
                   (dt0 + ui) * 32 + lo32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = pend.n0 + crow(r, hi);
        const float val = pacc[ui][r];
        if (kk < pend.ke && kk >= pend.ks && val != 0.f)
          unsafeAtomicAdd(dst + (size_t)kk * k_pitch, val);
      }
    }
  };

  // q rows of the block that exist, in 16-row MFMA k steps: the rest of the
  // exchange image is zero
  const int nstep = (min(qe - mblk0, HB) + 15) >> 4;

  bool more = next_seg();
  const bool ran = more;
  int cur = 0;
  if (more) stage_kv(0, nx);
  // the only tracked vector-memory loads of a work item: pin the compiler's
  // wait for them here, outside the k loop
#pragma unroll
  for (int dd = 0; dd < DF; ++dd) {
    pin_vgpr(qf[dd]);
    pin_vgpr(dof[dd]);
  }
  pin_vgpr(lse_q);
  pin_vgpr(dpsum_q);

  while (more) {
    pipe_barrier<0>();
    const QlTile t = nx;
    if (has_pend) flush();
    more = advance();
    if (more) stage_kv(cur ^ 1, nx);

    const int ns = t.n0;
    const char* lkb = smem + OFF_KV + 2 * cur * KVIMG;
    const char* lvb = lkb + KVIMG;
    char* prow = smem + OFF_PT + (BWD_BM * wave + lo32) * XP;
    char* drow = smem + OFF_DST + (BWD_BM * wave + lo32) * XP;

    // ================= phase 1: this wave's 32 q rows =================
    if (wave_alive(m0, qe) && ns + QL_TN > t.wk_lo && ns < t.wk_hi) {
      f32x16 sA = (f32x16)(0.f), dpA = (f32x16)(0.f);
#pragma unroll
      for (int dd = 0; dd < DF; ++dd) {
        const int off = swz(lo32, lo32 * ROWB + dd * 32 + hi * 16);
        const vec8 kf = *(const vec8*)(lkb + off);
        const vec8 vf = *(const vec8*)(lvb + off);
        sA = Tr::mfma(kf, qf[dd], sA);
        dpA = Tr::mfma(vf, dof[dd], dpA);
      }

      float pv[16], dsv[16];
      const bool interior =
          row_live && (ns >= t.ks) && (ns + QL_TN <= t.ke) &&
          !((t.atype == 1 || t.atype == 3) &&
            (ns + QL_TN - 1 > m0 + (t.ke - qe))) &&
          !((t.atype == 2 || t.atype == 3) &&
            (ns < m0 + BWD_BM - 1 + (t.ks - qs)));
      if (__all(interior) && !HAS_SOFTCAP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pij = fast_exp2(sA[r] * sl2 - lsc);
          pv[r] = pij;
          dsv[r] = pij * (dpA[r] - dpsum_q) * p.scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = ns + crow(r, hi);
          bool ok = row_live && kk < t.ke && kk >= t.ks;
          if (t.atype == 1 || t.atype == 3)
            ok = ok && (kk - qrow <= t.ke - qe);
          if (t.atype == 2 || t.atype == 3)
            ok = ok && (kk - qrow >= t.ks - qs);
          const float sv = sA[r];
          float dscale = p.scale;
          float tt;
          if (HAS_SOFTCAP) {
            const float th = tanhf(sv * cap_pre);
            tt = th * sl2;
            dscale = p.scale * (1.f - th * th);
          } else {
            tt = sv * sl2;
          }
          const float pij = ok ? fast_exp2(tt - lsc) : 0.f;
          pv[r] = pij;
          dsv[r] = ok ? pij * (dpA[r] - dpsum_q) * dscale : 0.f;
        }
      }

      // ---- dQ += dS K (B-frags by tr16 off the K row image) ----
      const vec8 dsa0 = Tr::afrag(dsv, 0);
      const vec8 dsa1 = Tr::afrag(dsv, 1);
      const int k_img = lds_base + OFF_KV + 2 * cur * KVIMG;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const vec8 b0 = tr_frag(k_img, ROWB, SW32M, 0, dt * 64);
        const vec8 b1 = tr_frag(k_img, ROWB, SW32M, 1, dt * 64);
        acc_dq[dt] = Tr::mfma(dsa0, b0, acc_dq[dt]);
        acc_dq[dt] = Tr::mfma(dsa1, b1, acc_dq[dt]);
      }

      // ---- P^T / dS^T -> this lane's q row of the exchange image, 4
      // consecutive k rows per 8-B write, rounded as the A-fragments are ----
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (8 * g + 4 * hi) * 2;
        uint2 pw, dw;
        pw.x = Tr::pack_pair(pv[4 * g + 0], pv[4 * g + 1]);
        pw.y = Tr::pack_pair(pv[4 * g + 2], pv[4 * g + 3]);
        dw.x = Tr::pack_pair(dsv[4 * g + 0], dsv[4 * g + 1]);
        dw.y = Tr::pack_pair(dsv[4 * g + 2], dsv[4 * g + 3]);
        *(uint2*)(prow + cb) = pw;
        *(uint2*)(drow + cb) = dw;
      }
    } else if (BWD_BM * wave < 16 * nstep) {
      // skipped: phase 2 still reads this wave's slice
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (8 * g + 4 * hi) * 2;
        *(uint2*)(prow + cb) = make_uint2(0u, 0u);
        *(uint2*)(drow + cb) = make_uint2(0u, 0u);
      }
    }

    // exchange image visible to the whole workgroup. LDS-only barrier: the
    // prefetch and the atomics stay in flight under phase 2.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ==== phase 2: dV / dK tiles, contracted over the block's q rows ====
    {
      const int a_img = lds_base + (is_dk ? OFF_DST : OFF_PT);
      const int b_img = lds_base + (is_dk ? OFF_Q : OFF_DO);
#pragma unroll
      for (int ui = 0; ui < UPW; ++ui) pacc[ui] = (f32x16)(0.f);
#pragma unroll
      for (int tt = 0; tt < HB / 16; ++tt) {
        if (tt < nstep) {  // block-uniform
          const vec8 a = tr_frag(a_img, XP, 0, tt, 0);
#pragma unroll
          for (int ui = 0; ui < UPW; ++ui) {
            const vec8 b = tr_frag(b_img, ROWB, SW32M, tt, (dt0 + ui) * 64);
            pacc[ui] = Tr::mfma(a, b, pacc[ui]);
          }
        }
      }
      pend = t;
      has_pend = true;
    }
    cur ^= 1;
  }
  if (has_pend) flush();
  // no tile ran: the Q/dO stage is still in flight and nothing waited for it
  if (!ran) drain_vm();

  // ---- store dq once (atomicAdd: q ranges of different slices may overlap;
  // DIRECT: the caller promises they do not) ----
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
  // every wave is past its last phase 2 before the next strided work item
  // restages the Q/dO images
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }  // strided work loop
}

// ---------------- launcher ----------------
template <class ET>
static int bwd_qloop(const magi_ffa_bwd_args* a, bool direct_dq) {
  BwdParams<ET> p;
  const int rc = fill_bwd_params(a, &p, DkvOpts{false, false, 0});
  if (rc) return rc > 0 ? 0 : rc;
  if (a->n_ranges > 65535) return -5;
  p.head_major = dq_knobs(a).head_major;
  // the dQ pass's grid rule: table entries x q blocks of the longest range
  // the tokens allow
  const int qspan = BWD_BM * QL_WAVES;
  const int qblocks = (int)((a->total_q + qspan - 1) / qspan);
  dim3 grid = p.head_major ? dim3(a->hq, qblocks, (unsigned)a->n_ranges)
                           : dim3(qblocks, a->hq, (unsigned)a->n_ranges);
  p.work_nx = grid.x; p.work_ny = grid.y; p.work_nz = grid.z;
  // one resident workgroup per CU: LDS at d = 128, registers at d = 64
  // (the softcap builds there would fit two)
  grid = cap_grid(grid, a->cu_margin & 0xFFFF, 1);
  const hipStream_t s = (hipStream_t)a->stream;
  const dim3 block(64 * QL_WAVES);
  auto go = [&](auto d, auto sc, auto direct) {
    hipLaunchKernelGGL(
        (ffa_bwd_qloop_kernel<ET, decltype(d)::value, decltype(sc)::value,
                              decltype(direct)::value>),
        grid, block, 0, s, p);
  };
  auto with_d = [&](auto d) {
    if (a->softcap > 0.f) {
      if (direct_dq) go(d, std::true_type{}, std::true_type{});
      else go(d, std::true_type{}, std::false_type{});
    } else {
      if (direct_dq) go(d, std::false_type{}, std::true_type{});
      else go(d, std::false_type{}, std::false_type{});
    }
  };
  if (a->d == 64) with_d(std::integral_constant<int, 64>{});
  else with_d(std::integral_constant<int, 128>{});
  return (int)hipGetLastError();
}

// Validation in the order magi_ffa.h documents, before any HIP call
extern "C" int magi_ffa_bwd_qloop(const magi_ffa_bwd_direct_args* d) {
  if (!d) return -1;
  const magi_ffa_bwd_args* a = &d->args;
  if (!a->dout || !a->q || !a->k || !a->v || !a->lse || !a->dq || !a->dk ||
      !a->dv || !a->dpsum)
    return -1;
  if (a->d != 64 && a->d != 128) return -2;
  if (a->hk <= 0 || a->hq % a->hk != 0) return -3;
  if (!elem_type_known(a->elem_type)) return -9;
  if (a->cu_margin & 0xFFFF0000) return -12;
  if (d->dkv_is_16bit != 0) return -16;
  return BY_ELEM_TYPE(a, bwd_qloop, d->dq_is_16bit != 0);
}
