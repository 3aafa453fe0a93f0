// ffa_index_bwd.hip — MI355X-native index-attention (token-gather) BACKWARD.
//
// The reference has no backward for index_attn (its autograd returns None
// for the index inputs); this is extension work on top of the forward in
// ffa_index.hip and shares its input contract: indices_2d [total_q, max_topk]
// int32 GLOBAL K row ids per q token row (-1 = contiguous tail padding), KV
// heads folded into the K row dimension (hk == 1).
//
// Per q token row i, valid slot j, g = idx[i, j] (preprocess has filled
// dpsum = rowsum(dO * O)):
//   s  = scale * q[i,h].k[g] ; t = softcap ? softcap*tanh(s/softcap) : s
//   p  = exp(t - lse[i,h])   ; dP = dO[i,h].v[g]
//   dS = p * (dP - dpsum[i,h]) * scale (* (1 - tanh^2) under softcap)
//   dQ[i,h] += dS * k[g] ;  dK[g] += sum_h dS * q[i,h] ;  dV[g] += sum_h p * dO[i,h]
//
// Work decomposition = the forward's: one workgroup per (token row, block of
// 32*W query heads), MFMA M dimension = query heads, K/V rows gathered into
// swizzled LDS by lane-indexed global_load_lds. Per 32-row gathered tile:
//   phase 1 (each wave: its own 32 heads)
//     S^T = K Q^T ; dP^T = V dO^T          (Q/dO B-frags persistent in VGPRs)
//     P^T, dS^T elementwise                (lane = head, regs = gathered rows)
//     dQ += dS K                           (register accumulator, single
//                                           owner, stored once, no atomics)
//     P^T / dS^T -> bf16 -> LDS exchange image [head][gathered row]
//   phase 2 (the workgroup's 2*D/32 output tiles split over the waves)
//     dV_tile = P^T dO ; dK_tile = dS^T Q  with the reduction running over
//     ALL 32*W heads of the workgroup (A-frags by tr16 reads off the exchange
//     image, B-frags by tr16 reads off the Q/dO images staged once per
//     workgroup), then ONE fp32 unsafeAtomicAdd per element into dk/dv at
//     row idx[i, j]. The cross-wave reduction therefore happens inside the
//     MFMA k loop and atomic traffic does not scale with W. Padding slots and
//     out-of-range ids issue no atomic at all.
// fp32 atomics reorder, so there is no deterministic mode.

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/magi_ffa.h"
#include "ffa_device.h"

#define IDXB_BN 32  // gathered k rows per tile

struct IdxBwdParams {
  const bf16_t* dout;
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const float* lse;
  const float* dpsum;
  const int* idx2d;  // [total_q, max_topk]
  bf16_t* dq;        // [total_q, hq, D], zero-init (count==0 rows stay 0)
  float* dk;         // [total_k, 1, D] fp32, zero-init, atomic-accumulated
  float* dv;
  int max_topk;
  int hq;
  float scale;
  float softcap;
  long long total_q, total_k;
};

template <int D, bool HAS_SOFTCAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void ffa_index_bwd_kernel(
    IdxBwdParams p) {
  constexpr int DF = D / 16;
  constexpr int DT = D / 32;
  constexpr int HB = 32 * WAVES;  // query heads per workgroup

  const long long tok = blockIdx.x;
  const int h0 = blockIdx.y * HB;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  const int* irow = p.idx2d + tok * (long long)p.max_topk;
  const int count = index_valid_count(irow, p.max_topk);
  if (count == 0) return;  // dq zero-init by the host; no dk/dv contribution

  const int q0 = h0 + wave * 32;  // first query head of this wave
  const int qh = q0 + lo32;       // this lane's query head
  const bool qvalid = qh < p.hq;
  const int qclamp = qvalid ? qh : (p.hq - 1);

  const float log2e = 1.4426950408889634f;
  const float sl2 = HAS_SOFTCAP ? p.softcap * log2e : p.scale * log2e;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;

  constexpr int ROWB = D * 2;  // bf16 row bytes
  constexpr int SW32M = ROWB / 32 - 1;
  auto swz = [](int row, int byte_off) {
    return byte_off ^ ((row & SW32M) << 5);
  };

  // ---- LDS (ONE shared object, see ffa_bwd.hip) ----
  //   [Q image | dO image]   HB rows x ROWB, 32-B swizzled, staged once
  //   [K0 | V0 | K1 | V1]    32 rows x ROWB each, gathered per tile
  //   [P^T | dS^T]           HB rows x 72 B: 32 bf16 gathered-row columns per
  //                          head row; the 8-B pad makes the per-lane 8-B row
  //                          writes bank-conflict-free (pitch 18 dwords)
  constexpr int XP = 72;
  constexpr int QIMG = HB * ROWB;
  constexpr int KVIMG = IDXB_BN * ROWB;
  constexpr int OFF_Q = 0;
  constexpr int OFF_DO = QIMG;
  constexpr int OFF_KV = 2 * QIMG;
  constexpr int OFF_PT = OFF_KV + 4 * KVIMG;
  constexpr int OFF_DST = OFF_PT + HB * XP;
  constexpr int LDS_BYTES = OFF_DST + HB * XP;
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) char ismem[LDS_BYTES];
  auto lds_k = [&](int buf) -> char* {
    return ismem + OFF_KV + (2 * buf) * KVIMG;
  };
  auto lds_v = [&](int buf) -> char* {
    return ismem + OFF_KV + (2 * buf + 1) * KVIMG;
  };
  const int lds_base = (int)(unsigned long long)(
      (__attribute__((address_space(3))) const char*)ismem);

  constexpr int ROWS_PER_GLDS = 1024 / ROWB;
  const int g_r = lane / (ROWB / 16);  // row within one 1-KB glds group
  const int g_c = lane % (ROWB / 16);  // 16-B slot within the row

  // ---- stage this wave's 32 Q and dO head rows (clamped past hq) ----
  {
#pragma unroll
    for (int gi = 0; gi < 32 / ROWS_PER_GLDS; ++gi) {
      const int r0 = 32 * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + g_r;
      const int hh = min(h0 + r, p.hq - 1);
      const int cs = g_c ^ ((r & SW32M) << 1);
      const long long src = (tok * p.hq + hh) * (long long)D + cs * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(p.q + src),
          (__attribute__((address_space(3))) unsigned int*)(ismem + OFF_Q +
                                                            r0 * ROWB),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(p.dout + src),
          (__attribute__((address_space(3))) unsigned int*)(ismem + OFF_DO +
                                                            r0 * ROWB),
          16, 0, 0);
    }
  }

  // ---- persistent per-wave operands: Q / dO B-fragments, lse, dpsum ----
  bf16x8 qf[DF], dof[DF];
  {
    const long long base = (tok * p.hq + qclamp) * (long long)D;
#pragma unroll
    for (int dd = 0; dd < DF; ++dd) {
      qf[dd] = *(const bf16x8*)(p.q + base + dd * 16 + hi * 8);
      dof[dd] = *(const bf16x8*)(p.dout + base + dd * 16 + hi * 8);
    }
  }
  const float lse_q = p.lse[tok * p.hq + qclamp];
  const float dpsum_q = p.dpsum[tok * p.hq + qclamp];
  const bool row_live = qvalid && lse_q != INFINITY && lse_q != -INFINITY;
  const float lsc = row_live ? lse_q * log2e : 0.f;

  f32x16 acc_dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_dq[dt] = (f32x16)(0.f);

  // Gathered K/V stage: global row = irow[position], clamped to an in-bounds
  // row for the load (masked in the math). Staged positions never exceed
  // max_topk-1 (64 | max_topk, tiles are 32 rows).
  static_assert(IDXB_BN / WAVES >= ROWS_PER_GLDS, "stage rows per wave");
  constexpr int GLDS_PER_WAVE = (IDXB_BN / WAVES) / ROWS_PER_GLDS;
  auto stage_glds = [&](int buf, int n0x) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (IDXB_BN / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + g_r;
      long long kr = irow[n0x + r];
      if (kr < 0 || kr >= p.total_k) kr = 0;
      const int cs = g_c ^ ((r & SW32M) << 1);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              p.k + kr * (long long)D + cs * 8),
          (__attribute__((address_space(3))) unsigned int*)(lds_k(buf) +
                                                            r0 * ROWB),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              p.v + kr * (long long)D + cs * 8),
          (__attribute__((address_space(3))) unsigned int*)(lds_v(buf) +
                                                            r0 * ROWB),
          16, 0, 0);
    }
  };

  // tr16 fragment off a row image: k-step tt (16 image rows = MFMA k dim),
  // 32 image columns starting at byte `colb` (= MFMA M or N dim). Lane
  // (lo32, hi) receives image[16*tt + 8*hi + 0..7][col0 + lo32] — the A/B
  // operand layout of v_mfma_f32_32x32x16_bf16 (same recipe as the forward's
  // PV B-fragments). swm = 32-B swizzle mask of the image (0: unswizzled).
  const int qhalf = (lane >> 4) & 1;
  const int jrow = (lane & 15) >> 2;
  const int lane8 = (lane & 3) * 8;
  auto tr_frag = [&](int img, int pitch, int swm, int tt, int colb) {
    const int row0 = 16 * tt + 8 * hi + jrow;
    const int row1 = row0 + 4;
    const int cb = colb + 32 * qhalf;
    return tr16_frag(img + row0 * pitch + lane8 + (cb ^ ((row0 & swm) << 5)),
                     img + row1 * pitch + lane8 + (cb ^ ((row1 & swm) << 5)));
  };

  // phase-2 work units: (matrix, d-tile), matrix 0 = dV, 1 = dK
  static_assert((2 * DT) % WAVES == 0, "units per wave");
  constexpr int UPW = 2 * DT / WAVES;

  int cur = 0;
  stage_glds(0, 0);
  for (int ns = 0; ns < count; ns += IDXB_BN) {
    // buf[cur] (and on the first trip the Q/dO images) landed; every wave is
    // past phase 2 of the previous tile, so the exchange image and buf[cur^1]
    // are free
    __syncthreads();
    if (ns + IDXB_BN < count) stage_glds(cur ^ 1, ns + IDXB_BN);

    // global ids of this lane's 16 C-fragment rows (crow(r, hi) = 8*(r>>2)
    // + 4*hi + (r&3)): four aligned int4 loads, shared by both phases
    int gid[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int4 v4 = *(const int4*)(irow + ns + 8 * g + 4 * hi);
      gid[4 * g + 0] = v4.x;
      gid[4 * g + 1] = v4.y;
      gid[4 * g + 2] = v4.z;
      gid[4 * g + 3] = v4.w;
    }

    const char* lkb = lds_k(cur);
    const char* lvb = lds_v(cur);

    // ================= phase 1: this wave's 32 heads =================
    {
      f32x16 sA = (f32x16)(0.f), dpA = (f32x16)(0.f);
#pragma unroll
      for (int dd = 0; dd < DF; ++dd) {
        const int off = swz(lo32, lo32 * ROWB + dd * 32 + hi * 16);
        bf16x8 kf = *(const bf16x8*)(lkb + off);
        bf16x8 vf = *(const bf16x8*)(lvb + off);
        sA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[dd], sA, 0, 0, 0);
        dpA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[dd], dpA, 0, 0, 0);
      }

      float pv[16], dsv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = ns + crow(r, hi);
        const bool ok = row_live && kk < count && gid[r] >= 0 &&
                        (long long)gid[r] < p.total_k;
        const float sv = sA[r];
        float dscale = p.scale;
        float t;
        if (HAS_SOFTCAP) {
          const float th = tanhf(sv * cap_pre);
          t = th * sl2;
          dscale = p.scale * (1.f - th * th);
        } else {
          t = sv * sl2;
        }
        const float pij = ok ? fast_exp2(t - lsc) : 0.f;
        pv[r] = pij;
        dsv[r] = ok ? pij * (dpA[r] - dpsum_q) * dscale : 0.f;
      }

      // ---- dQ += dS K (B-frags by tr16 off the K row image) ----
      const bf16x8 dsa0 = cframe_to_afrag(dsv, 0);
      const bf16x8 dsa1 = cframe_to_afrag(dsv, 1);
      const int k_img = lds_base + OFF_KV + (2 * cur) * KVIMG;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 b0 = tr_frag(k_img, ROWB, SW32M, 0, dt * 64);
        const bf16x8 b1 = tr_frag(k_img, ROWB, SW32M, 1, dt * 64);
        acc_dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa0, b0,
                                                             acc_dq[dt], 0, 0, 0);
        acc_dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa1, b1,
                                                             acc_dq[dt], 0, 0, 0);
      }

      // ---- P^T / dS^T -> exchange image row (this lane's head), 4
      // consecutive gathered rows per 8-B write ----
      char* prow = ismem + OFF_PT + (32 * wave + lo32) * XP;
      char* drow = ismem + OFF_DST + (32 * wave + lo32) * XP;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = (8 * g + 4 * hi) * 2;
        uint2 pw, dw;
        pw.x = pack_bf16_pair(pv[4 * g + 0], pv[4 * g + 1]);
        pw.y = pack_bf16_pair(pv[4 * g + 2], pv[4 * g + 3]);
        dw.x = pack_bf16_pair(dsv[4 * g + 0], dsv[4 * g + 1]);
        dw.y = pack_bf16_pair(dsv[4 * g + 2], dsv[4 * g + 3]);
        *(uint2*)(prow + cb) = pw;
        *(uint2*)(drow + cb) = dw;
      }
    }

    // exchange image visible to the whole workgroup. LDS-only barrier: the
    // next tile's gather stays in flight under phase 2.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ====== phase 2: dV / dK tiles, reduced over all HB heads, scatter ======
#pragma unroll
    for (int ui = 0; ui < UPW; ++ui) {
      const int u = wave * UPW + ui;
      const bool is_dk = u >= DT;  // wave-uniform
      const int dt = is_dk ? u - DT : u;
      const int a_img = lds_base + (is_dk ? OFF_DST : OFF_PT);
      const int b_img = lds_base + (is_dk ? OFF_Q : OFF_DO);
      f32x16 acc = (f32x16)(0.f);
#pragma unroll
      for (int tt = 0; tt < HB / 16; ++tt) {
        const bf16x8 a = tr_frag(a_img, XP, 0, tt, 0);
        const bf16x8 b = tr_frag(b_img, ROWB, SW32M, tt, dt * 64);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
      }
      float* dst = (is_dk ? p.dk : p.dv) + dt * 32 + lo32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = ns + crow(r, hi);
        const long long g = gid[r];
        if (kk < count && g >= 0 && g < p.total_k)
          unsafeAtomicAdd(dst + g * (long long)D, acc[r]);
      }
    }
    cur ^= 1;
  }

  // ======================= dQ epilogue (direct store) =======================
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = q0 + crow(r, hi);
    if (qr >= p.hq) continue;
    const long long base = (tok * p.hq + qr) * (long long)D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      p.dq[base + dt * 32 + lo32] = (bf16_t)acc_dq[dt][r];
  }
}

// ------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------
template <int D, int W>
static int launch_index_bwd(const IdxBwdParams& p, dim3 grid,
                            hipStream_t stream) {
  dim3 block(64 * W);
  if (p.softcap > 0.f)
    hipLaunchKernelGGL((ffa_index_bwd_kernel<D, true, W>), grid, block, 0,
                       stream, p);
  else
    hipLaunchKernelGGL((ffa_index_bwd_kernel<D, false, W>), grid, block, 0,
                       stream, p);
  return (int)hipGetLastError();
}

extern "C" int magi_ffa_bwd_index(const magi_ffa_index_bwd_args* a) {
  if (!a || !a->dout || !a->q || !a->k || !a->v || !a->lse || !a->dpsum ||
      !a->indices_2d || !a->dq || !a->dk || !a->dv)
    return -1;
  if (a->d != 64 && a->d != 128) return -2;
  if (a->hk != 1) return -3;  // kv heads are folded into K rows (see header)
  if (a->max_topk <= 0 || (a->max_topk & 63) != 0) return -4;
  if (a->total_q <= 0 || a->total_k <= 0 || a->hq <= 0) return 0;

  IdxBwdParams p;
  p.dout = (const bf16_t*)a->dout;
  p.q = (const bf16_t*)a->q;
  p.k = (const bf16_t*)a->k;
  p.v = (const bf16_t*)a->v;
  p.lse = a->lse;
  p.dpsum = a->dpsum;
  p.idx2d = a->indices_2d;
  p.dq = (bf16_t*)a->dq;
  p.dk = a->dk;
  p.dv = a->dv;
  p.max_topk = a->max_topk;
  p.hq = a->hq;
  p.scale = a->softmax_scale;
  p.softcap = a->softcap;
  p.total_q = a->total_q;
  p.total_k = a->total_k;

  // head-block = 32*W query heads, the rule of index_fwd_entry (ffa_device.h)
  const int w = (a->hq > 64) ? 4 : (a->hq > 32 ? 2 : 1);
  const int span = 32 * w;
  const unsigned hblocks = (unsigned)((a->hq + span - 1) / span);
  dim3 grid((unsigned)a->total_q, hblocks, 1);
  hipStream_t stream = (hipStream_t)a->stream;
  if (a->d == 64) {
    if (w == 4) return launch_index_bwd<64, 4>(p, grid, stream);
    if (w == 2) return launch_index_bwd<64, 2>(p, grid, stream);
    return launch_index_bwd<64, 1>(p, grid, stream);
  }
  if (w == 4) return launch_index_bwd<128, 4>(p, grid, stream);
  if (w == 2) return launch_index_bwd<128, 2>(p, grid, stream);
  return launch_index_bwd<128, 1>(p, grid, stream);
}
