// ffa_index_fp8.hip — fp8 (OCP e4m3) index-attention (token-gather) FORWARD
// kernel for gfx950.
//
// Decomposition of ffa_index.hip, numerics of ffa_fwd_fp8.hip:
//   - one workgroup per (q token row, 32*W query heads), W in {1, 2, 4}; the
//     MFMA M dimension is the token's query heads; valid count by the
//     wave-uniform binary search over the contiguous -1 tail; count == 0
//     returns at once (host presets out = 0, lse = -inf); direct epilogue.
//   - Q, K, V are raw e4m3 bytes, no descale factors. S = K Q^T and P V run
//     on v_mfma_f32_32x32x16_fp8_fp8 (fp32 accumulate); online softmax in the
//     exp2 domain with FP8_MAX_OFFSET = 8 subtracted before exp2 (P in [0, 256],
//     inside the e4m3 range) and added back into the lse; P is packed to e4m3
//     in-register. No defer-max: a deferred maximum would let P exceed 256.
//
// K staging: rows are D BYTES, gathered straight into LDS with lane-indexed
// global_load_lds (16 B per lane, lane-linear destination, so a swizzle can
// only permute 16-B chunks through the SOURCE address). An 8-byte
// ds_read_b64 A-fragment read is serviced per 32-lane half, and all 32 lanes
// of a half read the same 8-B half of a chunk - with a 16-B-granular image
// they can never cover more than half of the 64 banks (2-way conflict at
// best). The reads are therefore 16 B wide: the k (= d) index of the QK MFMA
// chain is permuted so that lane-half `hi` owns chunk 2j+hi of a row, and
// one ds_read_b128 feeds TWO MFMAs (low 8 B -> MFMA 2j, high 8 B -> MFMA
// 2j+1). Q is loaded with the same permutation, so the dot product is
// unchanged. Chunk swizzle: dest chunk = src chunk ^ ((row / (256/D)) &
// (D/16-1)) - conflict-free for the four 16-lane groups of ds_read_b128
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, + 32).
//
// V staging: V is the B operand of PV with k = gathered rows, so a lane needs
// 8 consecutive ROWS of one d column. The rows are gathered to registers
// (same lane -> (row, chunk) map as the K DMA, one shared index load) and
// written as a byte-transposed tile vt[d][row], the ffa_fwd_fp8.hip scheme.
// The loads for stage t+1 are issued before stage t's MFMAs and written
// after them. The row XOR ((d >> 5) & 3) << 3 spreads the byte writes over
// banks and is uniform across one B-fragment read (32 consecutive d), so the
// reads stay conflict-free with the 40/72-byte row pitch.
//
// Epilogue extras (off = null pointers, out/lse bit-identical): the attention
// sink is folded in fp32 after the lse has left the 2^8-offset domain, and
// max_logits takes a per-head atomic max of m_run * ln2 (no defer-max here,
// so m_run is the true row max) — see ffa_index.hip. A count == 0 row with a
// sink stores lse = lse_sink before it returns.

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/magi_ffa.h"
#include "ffa_device.h"

#define IDX8_BN 32  // k rows per inner MFMA tile

using u8 = unsigned char;
using u8x16 = __attribute__((ext_vector_type(16))) u8;
using i64x2 = __attribute__((ext_vector_type(2))) long;

// Register budget: the D=128 instances need ~180 registers (64 accumulator +
// the exp2/pack working set + the V rows in flight), so they ask for 2
// waves/SIMD (256 registers); a 4 waves/SIMD bound (128) spills. D=64 fits
// 128 registers at 2 and 4 waves per workgroup.
template <int D, bool HAS_SOFTCAP, bool OUT_BF16, int WAVES>
__global__ __launch_bounds__(64 * WAVES, (D > 64 || WAVES < 2) ? 2 : 4) void
ffa_index_fwd_fp8_kernel(IdxFwdParams<u8> p) {
  constexpr int DF = D / 16;  // 16-deep MFMAs per QK chain
  constexpr int DT = D / 32;

  const long long tok = blockIdx.x;
  const int h0 = blockIdx.y * (32 * WAVES);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  const int* irow = p.idx2d + tok * (long long)p.max_topk;
  const int count = index_valid_count(irow, p.max_topk);
  if (__builtin_expect(count == 0, 0)) {
    // out zero-init + lse -inf preset by the host; with a sink the row's
    // softmax mass is the sink's alone: lse = lse_sink, out stays 0
    if (p.sink) {
      const int eh = h0 + wave * 32 + lo32;
      if (eh < p.hq && hi == 0) {
        const float ls =
            index_sink_lse(p.sink, p.s_sink, p.sink_ssh, tok, p.hq, eh);
        if (ls != -INFINITY) p.lse[tok * p.hq + eh] = ls;
      }
    }
    return;
  }

  const int q0 = h0 + wave * 32;  // first query head of this wave
  const int qh = q0 + lo32;       // this lane's query head
  const bool qvalid = qh < p.hq;
  const bool qvalid_any = q0 < p.hq;
  const int qclamp = qvalid ? qh : (p.hq - 1);

  const float sl2 = HAS_SOFTCAP ? p.softcap * 1.4426950408889634f
                                : p.scale * 1.4426950408889634f;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;

  constexpr int ROWB = D;             // e4m3 row bytes (64 or 128)
  constexpr int CPR = ROWB / 16;      // 16-B chunks per row (4 or 8)
  constexpr int RPW = 256 / ROWB;     // rows per 256-B bank window (4 or 2)
  auto kswz = [](int row) { return (row / RPW) & (CPR - 1); };

  // staged-image depth: the rule of ffa_index.hip (32 rows for 1-2 waves,
  // 64 rows for 4 waves)
  constexpr int KITER = (WAVES >= 4) ? 64 : 32;
  constexpr int VPITCH = KITER + 8;  // vt row pitch: 40 / 72 B, 8-B aligned
  __shared__ __attribute__((aligned(16))) char ismem[2 * KITER * ROWB +
                                                     2 * D * VPITCH];
  auto lds_k = [&](int buf) -> char* { return ismem + buf * KITER * ROWB; };
  auto lds_vt = [&](int buf) -> char* {
    return ismem + 2 * KITER * ROWB + buf * D * VPITCH;
  };

  // Q fragments: chunk 2j+hi of the lane's head row (see the k permutation
  // in the file header); .x feeds MFMA 2j, .y MFMA 2j+1
  i64x2 qf[DF / 2];
  {
    const u8* qp = p.q + (tok * p.hq + qclamp) * (long long)D;
#pragma unroll
    for (int j = 0; j < DF / 2; ++j)
      qf[j] = *(const i64x2*)(qp + (2 * j + hi) * 16);
  }

  float m_run = -INFINITY;
  float l_run = 0.f;
  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = (f32x16)(0.f);

  constexpr int ROWS_PER_GLDS = 1024 / ROWB;  // 8 or 16
  static_assert(KITER / WAVES >= ROWS_PER_GLDS, "stage rows per wave");
  constexpr int GLDS_PER_WAVE = (KITER / WAVES) / ROWS_PER_GLDS;
  u8x16 vreg[GLDS_PER_WAVE];

  // Gathered stage: global row = irow[position], clamped for safety. The
  // staged positions never exceed max_topk-1 (64 | max_topk and the loop
  // rounds count up to KITER <= 64). K goes LDS-direct, V to registers.
  auto stage_issue = [&](int buf, int n0x) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (KITER / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + lane / CPR;
      const int c = lane % CPR;
      long long kr = irow[n0x + r];
      if (kr < 0 || kr >= p.total_k) kr = 0;  // pad/garbage: any in-bounds row
      const int cs = c ^ kswz(r);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              p.k + kr * (long long)D + cs * 16),
          (__attribute__((address_space(3))) unsigned int*)(lds_k(buf) +
                                                            r0 * ROWB),
          16, 0, 0);
      vreg[gi] = *(const u8x16*)(p.v + kr * (long long)D + c * 16);
    }
  };
  auto stage_write_v = [&](int buf) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (KITER / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + lane / CPR;
      const int c = lane % CPR;
      const int rs = r ^ (((c >> 1) & 3) << 3);  // bank spread, see header
      char* vt = lds_vt(buf) + (c * 16) * VPITCH + rs;
#pragma unroll
      for (int e = 0; e < 16; ++e) vt[e * VPITCH] = (char)vreg[gi][e];
    }
  };

  auto sub_body = [&](int ns, const char* lkb, const char* lvb) {
    if (!(ns < count && qvalid_any)) return;

    // ---- S^T = K Q^T (swapped; A = K rows from LDS, one b128 per 2 MFMAs) ----
    f32x16 s = (f32x16)(0.f);
#pragma unroll
    for (int j = 0; j < DF / 2; ++j) {
      const i64x2 kf = *(const i64x2*)(
          lkb + lo32 * ROWB + (((2 * j + hi) ^ kswz(lo32)) << 4));
      s = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(kf.x, qf[j].x, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(kf.y, qf[j].y, s, 0, 0, 0);
    }

    // ---- mask (position >= count) + scale into exp2 domain ----
    const bool interior = (q0 + 31 < p.hq) && (ns + IDX8_BN <= count);
    float t[16];
    float mx = -INFINITY;
    if (interior) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float sv = s[r];
        if (HAS_SOFTCAP) sv = tanhf(sv * cap_pre);
        t[r] = sv * sl2;
        mx = fmaxf(mx, t[r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = ns + crow(r, hi);
        const bool ok = qvalid && (kk < count);
        float sv = s[r];
        if (HAS_SOFTCAP) sv = tanhf(sv * cap_pre);
        t[r] = ok ? sv * sl2 : -INFINITY;
        mx = fmaxf(mx, t[r]);
      }
    }
    float pr[16];
    softmax_step_fp8(t, mx, hi, m_run, l_run, acc_o, pr);

    // ---- P -> fp8 A-fragments, PV from the byte-transposed V tile ----
    long pa[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) pa[tt] = cframe_to_afrag_fp8(pr, tt);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int kbs = (dt & 3) << 3;  // = ((d >> 5) & 3) << 3, write side
        const long bv = *(const long*)(lvb + (dt * 32 + lo32) * VPITCH +
                                       ((16 * tt + 8 * hi) ^ kbs));
        acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(pa[tt], bv,
                                                               acc_o[dt], 0, 0, 0);
      }
    }
  };

  int cur = 0;
  stage_issue(0, 0);
  stage_write_v(0);
  for (int n0 = 0; n0 < count; n0 += KITER) {
    __syncthreads();  // buf[cur]: K glds drained, V bytes written
    const bool has_next = n0 + KITER < count;  // block-uniform
    if (has_next) stage_issue(cur ^ 1, n0 + KITER);
#pragma unroll
    for (int sub = 0; sub < KITER / IDX8_BN; ++sub) {
      const int ns = n0 + sub * IDX8_BN;
      if (ns >= count) break;  // count is block-uniform
      sub_body(ns, lds_k(cur) + sub * IDX8_BN * ROWB,
               lds_vt(cur) + sub * IDX8_BN);
    }
    // buf[cur^1] was last read before this iteration's barrier
    if (has_next) stage_write_v(cur ^ 1);
    cur ^= 1;
  }

  // ======================= epilogue (direct store) =======================
  // the fp8 sum is scaled by 2^FP8_MAX_OFFSET relative to exp2(t - m)
  float lse_new =
      (l_run > 0.f)
          ? (m_run - FP8_MAX_OFFSET + __log2f(l_run)) * 0.6931471805599453f
          : -INFINITY;
  float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;

  // per-head max of the scaled (softcapped) logits of valid slots: there is
  // no defer-max here, so m_run is the lane's true head-row max in the exp2
  // domain -> x ln2. Invalid heads are -inf and drop out; the sink below does
  // not enter.
  if (p.max_logits && qvalid && hi == 0)
    head_atomic_max(p.max_logits + qh, m_run * 0.6931471805599453f);
  // sink fold, fp32, ahead of the single rounding of out. lse_new has left
  // the 2^FP8_MAX_OFFSET domain above; inv_l still carries it (as l_run does) and
  // only takes the extra factor exp(lse - lse'). Block-uniform branch; a null
  // sink leaves both untouched.
  if (p.sink && qvalid)
    index_sink_fold(
        index_sink_lse(p.sink, p.s_sink, p.sink_ssh, tok, p.hq, qh),
        lse_new, inv_l);

  if (lse_new != -INFINITY && qvalid && hi == 0)
    p.lse[tok * p.hq + qh] = lse_new;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int src = crow(r, hi);
    const float ilq = __uint_as_float(
        __builtin_amdgcn_ds_bpermute(src << 2, __float_as_uint(inv_l)));
    const int qr = q0 + src;
    if (qr >= p.hq || ilq <= 0.f) continue;
    const long long base = (tok * p.hq + qr) * (long long)D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const float val = acc_o[dt][r] * ilq;
      if (OUT_BF16)
        p.out_bf16[base + dt * 32 + lo32] = (bf16_t)val;
      else
        p.out_f32[base + dt * 32 + lo32] = val;
    }
  }
}

// host entry: checks, params and dispatch are index_fwd_entry (ffa_device.h)
extern "C" int magi_ffa_fwd_index_fp8(const magi_ffa_index_args* a) {
  return index_fwd_entry<u8>(
      a, [](auto D, auto W, auto SC, auto OB, dim3 grid, dim3 block,
            hipStream_t stream, const IdxFwdParams<u8>& p) {
        hipLaunchKernelGGL((ffa_index_fwd_fp8_kernel<D(), SC(), OB(), W()>),
                           grid, block, 0, stream, p);
      });
}
