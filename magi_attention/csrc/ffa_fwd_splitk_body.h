// ffa_fwd_splitk_body.h — the split-k forward (swap_ab; magi_ffa_fwd_splitk).
// Included by ffa_fwd.hip behind FwdParams, FFA_BN and LOCK_GRAN.
//
// ffa_fwd_body gives every wave 32 q rows of its own, so a q range of 16 to
// 64 rows leaves most of a workgroup with nothing but staging to do. Here the
// waves that have no q rows take a share of the k loop instead:
//   - a 4-wave workgroup owns QT (1 or 2) q tiles of 32 rows; wave w is
//     (qt, kw) = (w / KS, w % KS), KS = 4 / QT. The KS waves of a tile load the
//     same Q fragments.
//   - one barrier publishes a stage of 32 * KS k rows (128 for QT = 1, 64 for
//     QT = 2) in a 2-slot ring; all four waves stage, a quarter each. Wave kw
//     runs the stage's sub-tile [32 * kw, 32 * kw + 32) and no other: swapped
//     QK^T, the softmax step with defer-max, the P repack and PV are
//     ffa_fwd_body's, on a state (m_run, l_run, acc_o) of the wave's own, which
//     it carries across the k segments of a merged table.
//   - the per-tile bounds [n_lo, n_hi) come from the tile's first and last
//     token, the block bounds from the union of the tiles; a sub-tile outside
//     its tile's bounds is skipped by the `live` test, the barrier count stays
//     uniform over the workgroup.
//   - after the last segment's drain and barrier the ring is free: the waves
//     with kw > 0 write their state into it, each lane whole 16-byte runs in
//     its own lane layout (lane l of every wave of a tile owns the same q
//     column and the same C/D slots, so the reader needs no transpose), one
//     barrier, and the kw == 0 wave folds them in ascending kw:
//       m* = max m_i, a_i = exp2(m_i - m*) (0 for m_i = -inf),
//       l = sum a_i l_i, acc = sum a_i acc_i.
//     A deferred maximum is fine: each (m_i, l_i, acc_i) is consistent with
//     its own m_i. With max_logits the defer threshold is 0 and m* is the
//     true row maximum. The order is fixed, so a result repeats run to run.
//   - the epilogue is ffa_fwd_body's, run by the kw == 0 waves from the merged
//     registers; the others pass its barriers and store nothing.
// K/V swizzle, LDS-DMA staging outside the compiler's waitcnt tracking, the
// tr16 V reads one step ahead of their MFMAs, the last-first hand-out of
// causal blocks, the cu_margin work loop and the range locks are unchanged.
#pragma once

template <class ET, int D, bool HAS_SOFTCAP, bool ATOMIC, bool OUT_16, int QT>
DEV_INLINE void ffa_fwd_splitk_body(FwdParams<ET> p) {
  using Tr = ElemTraits<ET>;
  using vec8 = typename Tr::x8;
  static_assert(QT == 1 || QT == 2, "q tiles per workgroup");
  static_assert(D == 64 || D == 128, "head dim");
  constexpr int WAVES = 4;
  constexpr int KS = WAVES / QT;  // waves that split a tile's k stage
  constexpr int DF = D / 16;
  constexpr int DT = D / 32;
  constexpr int ROWB = D * 2;
  constexpr int ROWE = ROWB / 2;
  constexpr int VSLOTS = D / 8;
  constexpr int SW32M = ROWB / 32 - 1;
  constexpr int KITER = KS * FFA_BN;  // k rows per barrier
  constexpr int NBUF = 2;
  constexpr int RING_BYTES = NBUF * 2 * KITER * ROWB;
  // a partial: acc_o as DT * 4 float4 per lane, then (m_run, l_run, 0, 0)
  constexpr int PART_F4 = (DT * 4 + 1) * 64;
  static_assert(QT * (KS - 1) * PART_F4 * 16 <= RING_BYTES, "partials fit");
  constexpr int ROWS_PER_GLDS = 1024 / ROWB;
  constexpr int GLDS_PER_WAVE = (KITER / WAVES) / ROWS_PER_GLDS;
  static_assert(GLDS_PER_WAVE >= 1, "stage rows per wave");

  const long long work_total = (long long)p.work_nx * p.work_ny * p.work_nz;
  const long long grid_span = (long long)gridDim.x * gridDim.y * gridDim.z;
  for (long long w = blockIdx.x +
           (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * blockIdx.z);
       w < work_total; w += grid_span) {
  const int wx = (int)(w % p.work_nx);
  const long long w2 = w / p.work_nx;
  const int wy = (int)(w2 % p.work_ny);
  const int wz = (int)(w2 / p.work_ny);
  const int ri = p.head_major ? wz : wy;
  const int h = p.head_major ? wx : wz;
  const int mb_lin = p.head_major ? wy : wx;
  const int qs = p.q_ranges[2 * ri], qe = p.q_ranges[2 * ri + 1];
  const int R = qe - qs;
  const int nqb = (R + 32 * QT - 1) / (32 * QT);
  if (mb_lin >= nqb) continue;                // uniform across block
  const int seg0 = p.qk_starts ? p.qk_starts[ri] : ri;
  const int seg1 = p.qk_starts ? p.qk_starts[ri + 1] : ri + 1;
  const int at0 = (p.attn_type_map && seg0 < seg1) ? p.attn_type_map[seg0] : 0;
  const int mb = (at0 == 1 || at0 == 3) ? nqb - 1 - mb_lin : mb_lin;
  const int rb = mb * (32 * QT);              // block's first row
  int ks, ke, atype;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int qt = wave / KS;                   // the wave's q tile
  const int kw = wave % KS;                   // its sub-tile of every stage
  const int lo32 = lane & 31;
  const int hi = lane >> 5;

  const int rw = rb + qt * 32;                // tile's first row
  const bool qvalid = rw + lo32 < R;
  const bool qvalid_any = rw < R;
  const int qrow = qs + rw + lo32;
  const int qload = qs + (qvalid ? rw + lo32 : R - 1);
  // first and last token of the tile (tw0, tw1) and of the block (tb0, tb1)
  const int tw0 = qs + rw, tw1 = qs + min(rw + 31, R - 1);
  const int tb0 = qs + rb, tb1 = qs + min(rb + 32 * QT - 1, R - 1);

  const float sl2 = HAS_SOFTCAP ? p.softcap * 1.4426950408889634f
                                : p.scale * 1.4426950408889634f;
  const float cap_pre = HAS_SOFTCAP ? p.scale / p.softcap : 0.f;

  int n_lo = 0, n_hi = 0, b_lo = 0, b_hi = 0;
  auto seg_bounds = [&]() {
    n_lo = ks; n_hi = ke;
    if (qvalid_any) {
      if (atype == 1 || atype == 3) n_hi = min(n_hi, tw1 + (ke - qe) + 1);
      if (atype == 2 || atype == 3) n_lo = max(n_lo, tw0 + (ks - qs));
    } else {
      n_hi = n_lo;  // empty
    }
    b_lo = ks; b_hi = ke;
    if (atype == 1 || atype == 3) b_hi = min(b_hi, tb1 + (ke - qe) + 1);
    if (atype == 2 || atype == 3) b_lo = max(b_lo, tb0 + (ks - qs));
  };
  auto swz = [](int row, int byte_off) {
    return byte_off ^ ((row & SW32M) << 5);
  };
  __shared__ __attribute__((aligned(16))) char fsmem[RING_BYTES];
  auto lds_k = [&](int buf) -> ET* {
    return (ET*)(fsmem + (2 * buf) * KITER * ROWB);
  };
  auto lds_v = [&](int buf) -> ET* {
    return (ET*)(fsmem + (2 * buf + 1) * KITER * ROWB);
  };

  vec8 qf[DF];
  {
    const ET* qp = p.q + ((size_t)qload * p.hq + h) * D;
#pragma unroll
    for (int dd = 0; dd < DF; ++dd)
      qf[dd] = *(const vec8*)(qp + dd * 16 + hi * 8);
  }

  const int kh = h / p.gqa;
  const size_t k_pitch = (size_t)p.hk * D;
  const ET* kbase = p.k + (size_t)kh * D;
  const ET* vbase = p.v + (size_t)kh * D;

  float m_run = -INFINITY;
  float l_run = 0.f;
  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = (f32x16)(0.f);

  const int fsmem_byte = (int)(unsigned long long)(
      (__attribute__((address_space(3))) const char*)fsmem);
  // rows clamp to the segment's last one, so every source row lies in [ks, ke)
  auto stage_glds = [&](int buf, int n0x) {
#pragma unroll
    for (int gi = 0; gi < GLDS_PER_WAVE; ++gi) {
      const int r0 = (KITER / WAVES) * wave + ROWS_PER_GLDS * gi;
      const int r = r0 + lane / (ROWB / 16);
      const int c = lane % (ROWB / 16);
      const int kr = min(n0x + r, ke - 1);
      const int cs = c ^ ((r & SW32M) << 1);
      static_assert(ROWB / 16 == VSLOTS, "no padding slots at d 64 / 128");
      const int csw = cs * 8;
      const int lk = fsmem_byte + (2 * buf * KITER + r0) * ROWB;
      glds16_untracked(kbase + (size_t)kr * k_pitch + csw, lk);
      glds16_untracked(vbase + (size_t)kr * k_pitch + csw, lk + KITER * ROWB);
    }
  };

  // one 32-row sub-tile: ffa_fwd_body's, on this wave's partial state
  auto sub_body = [&](int ns, const ET* lkb, const ET* lvb) {
    const bool live = (ns + FFA_BN > n_lo) && (ns < n_hi) && qvalid_any;
    if (!live) return;

    f32x16 s = (f32x16)(0.f);
#pragma unroll
    for (int dd = 0; dd < DF; ++dd) {
      vec8 kf = *(const vec8*)(
          (const char*)lkb + swz(lo32, lo32 * ROWB + dd * 32 + hi * 16));
      s = Tr::mfma(kf, qf[dd], s);
    }

    const bool interior =
        (rw + 31 < R) && (ns >= n_lo) && (ns + FFA_BN <= n_hi) &&
        !((atype == 1 || atype == 3) && (ns + FFA_BN - 1 > tw0 + (ke - qe))) &&
        !((atype == 2 || atype == 3) && (ns < tw1 + (ks - qs)));
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
        bool ok = qvalid && (kk >= n_lo) && (kk < n_hi);
        if (atype == 1 || atype == 3) ok = ok && (kk - qrow <= ke - qe);
        if (atype == 2 || atype == 3) ok = ok && (kk - qrow >= ks - qs);
        float sv = s[r];
        if (HAS_SOFTCAP) sv = tanhf(sv * cap_pre);
        t[r] = ok ? sv * sl2 : -INFINITY;
        mx = fmaxf(mx, t[r]);
      }
    }
    mx = fmaxf(mx, warp_xor32(mx));

    // defer-max as in ffa_fwd_body; max_logits wants the true maximum
    const float m_new = fmaxf(m_run, mx);
    const float defer_thr = p.max_logits ? 0.f : 8.f;
    const bool need_rescale =
        (m_new > m_run + defer_thr) ||
        (m_run == -INFINITY && m_new != -INFINITY);
    float m_use;
    float alpha;
    if (!__any(need_rescale)) {
      m_use = (m_run == -INFINITY) ? 0.f : m_run;
      alpha = 1.f;
    } else {
      m_use = (m_new == -INFINITY) ? 0.f : m_new;
      alpha = (m_run == -INFINITY) ? 0.f : fast_exp2(m_run - m_use);
      m_run = m_new;
    }

    float pr[16];
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pr[r] = fast_exp2(t[r] - m_use);
      psum += pr[r];
    }
    l_run = l_run * alpha + (psum + warp_xor32(psum));

    // wave-uniform condition: ds_bpermute reads other lanes' registers
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float aq = __uint_as_float(__builtin_amdgcn_ds_bpermute(
            crow(r, hi) << 2, __float_as_uint(alpha)));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc_o[dt][r] *= aq;
      }
    }

    vec8 pa[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) pa[tt] = Tr::afrag(pr, tt);

    {
      const int qhalf = (lane >> 4) & 1;
      const int jrow = (lane & 15) >> 2;
      const int v_base = (int)(unsigned long long)(
          (__attribute__((address_space(3))) const char*)lvb);
      const int lane8 = (lane & 3) * 8;
      auto vfrag = [&](int j) {
        const int tt = j / DT, dt = j % DT;
        const int row0 = 16 * tt + 8 * hi + jrow;
        const int row1 = row0 + 4;
        const int sw0 = (row0 & SW32M) << 5;
        const int sw1 = (row1 & SW32M) << 5;
        const int rb0 = v_base + row0 * ROWB + lane8;
        const int rb1 = v_base + row1 * ROWB + lane8;
        const int dcol = (dt * 32 + 16 * qhalf) * 2;
        return Tr::tr16(rb0 + (dcol ^ sw0), rb1 + (dcol ^ sw1));
      };
      vec8 bcur = vfrag(0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read x2
#pragma unroll
      for (int j = 0; j < 2 * DT; ++j) {
        vec8 bnext = bcur;
        if (j + 1 < 2 * DT) {
          bnext = vfrag(j + 1);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        acc_o[j % DT] = Tr::mfma(pa[j / DT], bcur, acc_o[j % DT]);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA x1
        bcur = bnext;
      }
    }
  };

  bool any_seg = false;
  for (int seg = seg0; seg < seg1; ++seg) {
    ks = p.k_ranges[2 * seg];
    ke = p.k_ranges[2 * seg + 1];
    atype = p.attn_type_map ? p.attn_type_map[seg] : 0;
    if (ke <= ks) continue;  // uniform across block
    seg_bounds();
    if (b_lo >= b_hi) continue;
    any_seg = true;
    int cur = 0;
    stage_glds(0, b_lo);
    // the compiler's wait for the Q loads, kept out of the k loop
#pragma unroll
    for (int dd = 0; dd < DF; ++dd) pin_vgpr(qf[dd]);
    for (int n0 = b_lo; n0 < b_hi; n0 += KITER) {
      // the wave's only vector-memory ops in flight are stage(cur)'s: drain
      // them, publish, then prefetch the next stage under this one's compute
      pipe_barrier<0>();
      if (n0 + KITER < b_hi) stage_glds(cur ^ 1, n0 + KITER);
      const int ns = n0 + kw * FFA_BN;
      if (ns < b_hi)
        sub_body(ns, lds_k(cur) + kw * FFA_BN * ROWE,
                 lds_v(cur) + kw * FFA_BN * ROWE);
      cur ^= 1;
    }
    // nothing is in flight (the last iteration staged nothing); the barrier
    // retires every wave's LDS reads before the ring is restaged or reused
    drain_vm();
    __syncthreads();
  }
  if (any_seg) {

  // ======================= merge of the KS partials =======================
  const bool owner = kw == 0;
  {
    float4* const part = (float4*)fsmem + qt * (KS - 1) * PART_F4;
    if (!owner) {
      float4* const ps = part + (kw - 1) * PART_F4;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          ps[(dt * 4 + j) * 64 + lane] =
              make_float4(acc_o[dt][4 * j], acc_o[dt][4 * j + 1],
                          acc_o[dt][4 * j + 2], acc_o[dt][4 * j + 3]);
      ps[DT * 4 * 64 + lane] = make_float4(m_run, l_run, 0.f, 0.f);
    }
    __syncthreads();
    if (owner) {
      float mi[KS], li[KS];
      mi[0] = m_run;
      li[0] = l_run;
      float ms = m_run;
#pragma unroll
      for (int i = 1; i < KS; ++i) {
        const float4 ml = part[(i - 1) * PART_F4 + DT * 4 * 64 + lane];
        mi[i] = ml.x;
        li[i] = ml.y;
        ms = fmaxf(ms, ml.x);
      }
      l_run = 0.f;
#pragma unroll
      for (int i = 0; i < KS; ++i) {  // ascending kw: a fixed order
        const float a = (mi[i] == -INFINITY) ? 0.f : fast_exp2(mi[i] - ms);
        l_run += a * li[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float aq[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            aq[e] = __uint_as_float(__builtin_amdgcn_ds_bpermute(
                crow(4 * j + e, hi) << 2, __float_as_uint(a)));
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            if (i == 0) {
#pragma unroll
              for (int e = 0; e < 4; ++e) acc_o[dt][4 * j + e] *= aq[e];
            } else {
              const float4 x =
                  part[(i - 1) * PART_F4 + (dt * 4 + j) * 64 + lane];
              acc_o[dt][4 * j + 0] += aq[0] * x.x;
              acc_o[dt][4 * j + 1] += aq[1] * x.y;
              acc_o[dt][4 * j + 2] += aq[2] * x.z;
              acc_o[dt][4 * j + 3] += aq[3] * x.w;
            }
          }
        }
      }
      m_run = ms;
    } else {
      m_run = -INFINITY;  // nothing of this wave reaches the epilogue
      l_run = 0.f;
    }
    // the owners' reads are done before a strided work item restages the ring
    __syncthreads();
  }

  // ======================= epilogue (kw == 0 waves) =======================
  const bool qst = qvalid && owner;
  if (p.max_logits) {
    float ml = m_run * 0.6931471805599453f;
#pragma unroll
    for (int off = 32; off; off >>= 1)
      ml = fmaxf(ml, __shfl_xor(ml, off, 64));
    if (lane == 0 && ml != -INFINITY) unsafeAtomicMax(p.max_logits + h, ml);
  }
  const float lse_new =
      (l_run > 0.f) ? (m_run + __log2f(l_run)) * 0.6931471805599453f : -INFINITY;
  const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
  const size_t orow = (size_t)qrow * p.hq + h;
  auto out_base = [&](int src) -> size_t {
    return ((size_t)(qs + rw + src) * p.hq + h) * D;
  };

  if (!ATOMIC) {
    // direct store: rows with l == 0 keep their initial value (inv_l = 0
    // also keeps the kw > 0 waves out)
    if (l_run > 0.f && qst && hi == 0) p.lse[orow] = lse_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int src = crow(r, hi);
      const float ilq = __uint_as_float(
          __builtin_amdgcn_ds_bpermute(src << 2, __float_as_uint(inv_l)));
      if (!(rw + src < R && ilq > 0.f)) continue;
      const size_t base = out_base(src);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float val = acc_o[dt][r] * ilq;
        if (OUT_16)
          p.out_16[base + dt * 32 + lo32] = Tr::from_f32(val);
        else
          p.out_f32[base + dt * 32 + lo32] = val;
      }
    }
  } else {

  // lock-guarded read-merge-write: a 32 * QT-row block spans at most two
  // LOCK_GRAN slots, taken in ascending order as by every other launch
  const int s0 = tb0 / LOCK_GRAN, s1 = tb1 / LOCK_GRAN;
  if (threadIdx.x == 0) {
    for (int sl = s0; sl <= s1; ++sl) {
      int* lk = p.locks + (size_t)sl * p.hq + h;
      int expected = 0;
      while (!__hip_atomic_compare_exchange_strong(
          lk, &expected, 1, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT))
        expected = 0;
    }
  }
  __syncthreads();

  float lse_prev = -INFINITY;
  if (qst) lse_prev = p.lse[orow];
  float lse_m;
  {
    const float a = fmaxf(lse_prev, lse_new);
    const float b = fminf(lse_prev, lse_new);
    lse_m = (a == -INFINITY) ? -INFINITY : a + log1pf(expf(b - a));
  }
  const float w_prev = (lse_prev == -INFINITY) ? 0.f : expf(lse_prev - lse_m);
  const float w_new = (lse_new == -INFINITY) ? 0.f : expf(lse_new - lse_m) * inv_l;

  if (qst && lse_m != -INFINITY && hi == 0) p.lse[orow] = lse_m;

  // a kw > 0 wave has lse_prev = lse_new = -inf: both weights 0, no access
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int src = crow(r, hi);
    const float wp = __uint_as_float(
        __builtin_amdgcn_ds_bpermute(src << 2, __float_as_uint(w_prev)));
    const float wn = __uint_as_float(
        __builtin_amdgcn_ds_bpermute(src << 2, __float_as_uint(w_new)));
    if (rw + src >= R || (wp == 0.f && wn == 0.f)) continue;
    const size_t base = out_base(src);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      float* ptr = p.out_f32 + base + dt * 32 + lo32;
      // first writer (wp == 0) must not read: `out` may be uninitialised
      const float prev = (wp > 0.f) ? wp * (*ptr) : 0.f;
      *ptr = prev + wn * acc_o[dt][r];
    }
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int sl = s1; sl >= s0; --sl)
      __hip_atomic_store(p.locks + (size_t)sl * p.hq + h, 0,
                         __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  }  // ATOMIC epilogue
  }  // any_seg
  }  // strided work loop
}

// An entry of its own, built without the packed-f32 VALU ops like every
// kernel added since SPARSE.
template <class ET, int D, bool HAS_SOFTCAP, bool ATOMIC, bool OUT_16, int QT>
__global__ __launch_bounds__(256, 2)
__attribute__((target("no-packed-fp32-ops"))) void ffa_fwd_splitk_kernel(
    FwdParams<ET> p) {
  ffa_fwd_splitk_body<ET, D, HAS_SOFTCAP, ATOMIC, OUT_16, QT>(p);
}
