// ffa_bwd_dq_body.h — the body of the dQ kernels of ffa_bwd.hip, which
// includes this file inside the braces of ffa_bwd_dq_kernel (SPARSE = false)
// and of ffa_bwd_dq_sparse_body (SPARSE = true); the block comments above
// those two describe the design. The text is shared by inclusion, not
// through a force-inlined function: the default kernels must stay the code
// they were instruction for instruction, and an inlined body does not
// compile to that (profiles/bwd_sparse_load.md). In scope at the point of
// inclusion: the template parameters ET, D, HAS_SOFTCAP, WAVES and DIRECT,
// the kernel argument `BwdParams<ET> p`, `constexpr bool SPARSE` and
// `const int* k_cum` (read only under SPARSE). No include guard: it is meant
// to be included more than once.
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
  const int at0 = (!SPARSE && p.attn_type_map) ? p.attn_type_map[seg0] : 0;
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
  // SPARSE: the row map sits behind the ring; two 4-wave workgroups must
  // still share a CU's 160 KB
  constexpr int RING_BYTES = NBUF * 2 * KITER * ROWB;
  constexpr int MAP_BYTES = SPARSE ? SPARSE_MAP_ROWS * 4 : 0;
  static_assert(!SPARSE || (D != 192 && RING_BYTES + MAP_BYTES <=
                                             (WAVES == 8 ? 163840 : 81920)),
                "LDS budget with the row map");
  __shared__ __attribute__((aligned(16))) char smem[RING_BYTES + MAP_BYTES];
  int* const smap = (int*)(smem + RING_BYTES);  // SPARSE: the row map
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
      // SPARSE: n0x, r and ke count virtual rows of the chunk (ke = Lc)
      const int kr = SPARSE ? smap[min(n0x + r, ke - 1)]
                            : min(n0x + r, ke - 1);
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
  // SPARSE: `seg` counts chunks of the virtual k axis, not segments
  const int cum0 = SPARSE ? k_cum[seg0] : 0;
  const int vlen = SPARSE ? k_cum[seg1] - cum0 : 0;  // L, block-uniform
  const int loop0 = SPARSE ? 0 : seg0;
  const int loop1 =
      SPARSE ? (vlen + SPARSE_MAP_ROWS - 1) / SPARSE_MAP_ROWS : seg1;
  for (int seg = loop0; seg < loop1; ++seg) {
  if constexpr (SPARSE) {
    const int c0 = seg * SPARSE_MAP_ROWS;  // chunk's first virtual row
    ks = 0;
    ke = min(vlen - c0, SPARSE_MAP_ROWS);  // Lc >= 1
    atype = 0;
    // The ring is drained and every wave is past the barrier that ended the
    // previous chunk or work item: nobody reads the map any more.
    for (int j = tid; j < ke; j += 64 * WAVES) {
      const int x = cum0 + c0 + j;
      // first segment boundary above x: k_cum[s] <= x < k_cum[s + 1] names a
      // non-empty segment, and k_cum[seg1] = cum0 + L > x ends the search
      int blo = seg0 + 1, bhi = seg1;
      while (blo < bhi) {
        const int mid = (blo + bhi) >> 1;
        if (k_cum[mid] > x) bhi = mid;
        else blo = mid + 1;
      }
      const int s = blo - 1;
      const int row = p.k_ranges[2 * s] + (x - k_cum[s]);
      // a k_cum that disagrees with k_ranges must not leave K and V
      smap[j] = min(max(row, 0), (int)p.total_k - 1);
    }
    __syncthreads();
  } else {
  ks = p.k_ranges[2 * seg];
  ke = p.k_ranges[2 * seg + 1];
  atype = p.attn_type_map ? p.attn_type_map[seg] : 0;
  if (ke <= ks) continue;  // uniform across block
  }
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
