// brick_sweeps.inc — the body of gls::k_brick_sweeps (csrc/brick.h): the
// steps x <- x + omega D^{-1} (b - A x) of one smoothing sequence, one
// workgroup per brick for all of them.  Per sweep j the result equals one
// k_brick launch with the fused relaxation and deferred reduction (sweep j
// rebuilds the shared nodes from sweep j - 1's partial slots in the same
// order and arithmetic as k_brick's QREC gather); the exclusive nodes'
// iterate stays in registers, so only the last sweep writes vectors.
// Expects in scope: dim, k, T, MODE, GEO, ZL, DET, G, a, sw.
#include "brick_setup.inc"
  static_assert(sizeof(T) == 4 && nc == 4 && NP == 1 && MODE != MODE_RESIDUAL && ZL == 1,
                "resident sweeps: FP32 3D smoothing levels");

  constexpr int   NI = (BrickLattice<dim, k, ZL>::L + BLOCK - 1) / BLOCK;
  const uint32_t *bn = k_nodes + brick * (int64_t)L;
  const uint32_t *bt = k_target + brick * (int64_t)L;
  uint32_t        pk[NI], tg[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int i = t + it * BLOCK;
      const uint32_t ic = (uint32_t)(i < L ? i : L - 1) * 4u;
      const uint32_t pl = load_so(bn, ic), tl = load_so(bt, ic);
      pk[it]            = i < L ? pl : 0u;
      tg[it]            = i < L ? tl : 0u;
    }
  static_assert(NI == 1, "one lattice node per thread");
  // lattice of at most SWEEP_MAX_L = 128 nodes (gls::brick_sweeps checks):
  // thread t + 128 helps thread t rebuild its shared node (slots 4..7 of an
  // 8..11-fold one)
  const uint32_t tl_hi = load_so(bt, (uint32_t)(t >= 128 && t - 128 < L ? t - 128 : 0) * 4u);
  const uint32_t tg_hi = t >= 128 && t - 128 < L ? tl_hi : 0u;
  const bool     general = G == GEO_GEN || (G == GEO_ANY && rec.curved != 0);
  const int      ncell   = (int)rec.ncell;
  const int      Lxy     = a.Lx * a.Ly;
  // the coefficient tables' image to LDS (the first sweep's barrier orders it
  // before the first read)
  if (t < NCOEF)
    s_tab[t] = coef_v;

  // the iterate at the lattice nodes (sweep j's src), b and D^{-1} there
  T u[NI][nc], xb[NI][nc], xd[NI][nc];
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int      i    = t + it * BLOCK;
      const uint32_t node = pk[it] & NODE_MASK;
#pragma unroll
      for (int c = 0; c < nc; ++c)
        u[it][c] = T(0), xb[it][c] = T(0), xd[it][c] = T(1);
      if (i < L && node != UNUSED_NODE)
        {
          load_node<T, nc>(a.src, node, u[it]);
          load_node<T, nc>(a.rb, node, xb[it]);
          if (a.rd)
            load_node<T, nc>(a.rd, node, xd[it]);
        }
    }
  for (int j = 0; j < sw.nsweep; ++j)
    {
      const bool last = j + 1 == sw.nsweep;
#if GLS_SWEEP_TIMING
      if (t == 0 && sw.timing)
        sw.timing[((size_t)brick * sw.nsweep + j) * 6 + 0] = wall_clock64();
#endif
      // the lane's indices and node ids from opaque copies: everything
      // derived from them (LDS offsets, global addresses) is recomputed per
      // sweep instead of hoisted out of the loop and held in registers
      // (the hoisted form measured ~50 VGPRs more and spilled)
      int t_l = t;
      asm volatile("" : "+v"(t_l));
      const int t = t_l;
#include "brick_lane.inc"
      uint32_t pkv[NI], tgv[NI];
#pragma unroll
      for (int it = 0; it < NI; ++it)
        {
          pkv[it] = pk[it], tgv[it] = tg[it];
          asm volatile("" : "+v"(pkv[it]), "+v"(tgv[it]));
        }
      V    part_g0 = {}, part_p = {}, part_s = {};
      int  part_m    = 0;
      bool timed_out = false; // a slot wait of this thread hit the spin bound
      if (j > 0)
        {
          // ---- shared nodes: sweep j - 1's reduction from its tagged partial
          // granules.  A granule is 8 bytes {value, sweep tag} written by one
          // write-through store (R2 of cdna_hip_programming.md §6 Guideline
          // 16: the data is the flag, no fence, no counter); a wave re-reads
          // its slots until every tag is sweep j - 1's.  The node's m slots
          // are summed in k_shared_reduce_cls's order and arithmetic (k_brick's
          // QREC gather): groups of four (x0 + x1) + (x2 + x3) in turn, then a
          // pair, then one.  Thread t < 128 reads group 0 and the rest, thread
          // t + 128 group 1 (m >= 8), handed over through LDS.
          using U4            = __attribute__((ext_vector_type(4))) unsigned int;
          const uint64_t *gp  = (j & 1) ? sw.gran[0] : sw.gran[1];
          const auto      grs = __builtin_amdgcn_make_buffer_rsrc((void *)gp, (short)0,
                                                                  (int)sw.gran_bytes, 0x00020000);
          const uint32_t  tag = sw.epoch + (uint32_t)j; // sweep j - 1's
          const bool      hi  = t >= 128;
          const uint32_t  tgx = hi ? tg_hi : tgv[0];
          const bool      shared =
            (hi ? t - 128 < L : t < L) && tgx != UNUSED_NODE && (tgx & SHARED_BIT);
          uint32_t m = 0, b0 = 0;
          if (shared)
            {
              const uint32_t slt = tgx & ~SHARED_BIT;
              const int      kc  = slot_class(a.rc, slt);
              m                  = a.rc.mult[kc];
              b0                 = a.rc.slot0[kc] + (slt - a.rc.slot0[kc]) / m * m;
            }
          // this thread's slots: k -> slot index (upper half: 4 + k, k < 4)
          const int rb = m >= 8 ? 8 : m >= 4 ? 4 : 0; // first slot after the groups
          const int nk = hi ? (m >= 8 ? 4 : 0) : (m >= 8 ? 4 + (int)m - 8 : (int)m);
          V         xv[7];
          for (int spin = 0;; ++spin)
            {
              bool ok = true;
#pragma unroll
              for (int q7 = 0; q7 < 7; ++q7)
                if (q7 < nk)
                  {
                    const int slot_k = hi ? 4 + q7 : (q7 < 4 ? q7 : q7 - 4 + rb);
                    const int off    = (int)((b0 + (uint32_t)slot_k) * 32u);
                    const U4  g0 = __builtin_amdgcn_raw_buffer_load_b128(grs, off, 0, 16);
                    const U4  g1 = __builtin_amdgcn_raw_buffer_load_b128(grs, off + 16, 0, 16);
                    ok = ok && g0[1] == tag && g0[3] == tag && g1[1] == tag && g1[3] == tag;
                    xv[q7][0] = __uint_as_float(g0[0]), xv[q7][1] = __uint_as_float(g0[2]);
                    xv[q7][2] = __uint_as_float(g1[0]), xv[q7][3] = __uint_as_float(g1[2]);
                  }
              if (__all(ok))
                break;
              if (spin >= sw.spin_max)
                {
                  if (lane == 0)
                    {
                      atomicAdd(sw.err, 1u);
                      // the host's stall flag (system scope: host memory)
                      if (sw.flag)
                        __hip_atomic_store(sw.flag, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                  timed_out = true;
                  break;
                }
              __builtin_amdgcn_s_sleep(1);
            }
          if (hi)
            {
              // group 1 for the lower thread (s_work is free between sweeps)
              if (m >= 8)
                s_work[t - 128] = (xv[0] + xv[1]) + (xv[2] + xv[3]);
            }
          else if (shared)
            {
              const int rem = (int)m - rb; // 0..3 after the groups
              part_m        = (int)m;
              if (m >= 4)
                part_g0 = (xv[0] + xv[1]) + (xv[2] + xv[3]);
              // the remainder at k = 0.. (m < 4) or k = 4.. (m >= 4)
              const V r0 = m >= 4 ? xv[4] : xv[0], r1 = m >= 4 ? xv[5] : xv[1];
              const V r2 = m >= 4 ? xv[6] : xv[2];
              if (rem >= 2)
                part_p = r0 + r1;
              part_s = rem == 3 ? r2 : r0;
            }
        }

#if GLS_SWEEP_TIMING
      if (t == 0 && sw.timing)
        sw.timing[((size_t)brick * sw.nsweep + j) * 6 + 1] = wall_clock64();
#endif
      // ---- the previous sweep's write-out has read the accumulator
      // lattice; group 1 sums are in s_work.  A wait that hit its spin bound
      // anywhere in the workgroup poisons the brick's iterate with NaN: a
      // stalled hand-off fails loudly downstream instead of smoothing with
      // stale partial sums (gls_op_sweep_stats counts it)
      const int any_timeout = __syncthreads_or(timed_out ? 1 : 0);
      if (j > 0)
        {
#pragma unroll
          for (int it = 0; it < NI; ++it)
            {
              const int      i    = t + it * BLOCK;
              const uint32_t node = pkv[it] & NODE_MASK;
              if (!(i < L && node != UNUSED_NODE && (tgv[it] & SHARED_BIT)))
                continue;
              const int m   = part_m;
              const int rb  = m >= 8 ? 8 : m >= 4 ? 4 : 0;
              const int rem = m - rb;
              V         sum = {};
              if (m >= 4)
                sum += part_g0;
              if (m >= 8)
                sum += s_work[t];
              if (rem >= 2)
                sum += part_p;
              if (rem == 3 || rem == 1)
                sum += part_s;
              V              xs, bb, dd;
              const uint32_t cm = pkv[it] >> 28;
#pragma unroll
              for (int w = 0; w < W; ++w)
                {
                  xs[w] = u[it][w], bb[w] = xb[it][w], dd[w] = xd[it][w];
                  if ((cm >> w) & 1)
                    sum[w] = xs[w];
                }
              const V v = xs + a.romega * dd * (bb - sum);
#pragma unroll
              for (int c = 0; c < nc; ++c)
                u[it][c] = v[c];
              // the last sweep's src in memory: the reduction after the
              // launch (or the next launch's gather) reads it
              if (any_timeout)
#pragma unroll
                for (int c = 0; c < nc; ++c)
                  u[it][c] = __builtin_nanf("");
              if (last)
                store_node<T, nc>((j & 1 ? sw.vec[1] : sw.vec[0]), node, u[it]);
            }
        }

      // round 0's tables and geometry (read-only; L2-resident after the first
      // sweep): in flight during the staging and the evaluate sweeps (issued
      // before the granule wait, or kept across the sweeps, they spill)
      LaneData<dim, T, MODE> cur;
      if constexpr (!(FOUR && G == GEO_GEN)) // (curved 4-wave bodies: after the evaluate sweeps)
        load_lane<dim, k, T, MODE, G>(a, ks, rec, general, wcell0, slot, in_wave, p, cur);
      // ---- stage the src lattice (homogeneous constraints read as 0)
#pragma unroll
      for (int it = 0; it < NI; ++it)
        {
          const int i = t + it * BLOCK;
          if (i >= L)
            break;
          const int      iz = idiv_f(i, a.rLxy), iy = idiv_f(i - iz * Lxy, a.rLx);
          const int      ip = (i - iz * Lxy - iy * a.Lx) + a.PLx * (iy + a.PLy * iz);
          const uint32_t cm = pkv[it] >> 28;
          T              us[nc];
#pragma unroll
          for (int c = 0; c < nc; ++c)
            {
              us[c]              = ((cm >> c) & 1) ? T(0) : u[it][c];
              s_acc[c * LP + ip] = 0.0;
            }
          V v[NP];
          to_packs<V, T, nc, NP, W>(us, v);
          s_src[ip] = v[0];
        }
      __syncthreads();

#if GLS_SWEEP_TIMING
      if (t == 0 && sw.timing)
        sw.timing[((size_t)brick * sw.nsweep + j) * 6 + 2] = wall_clock64();
#endif
#include "brick_rounds.inc"
      __syncthreads();
#if GLS_SWEEP_TIMING
      if (t == 0 && sw.timing)
        sw.timing[((size_t)brick * sw.nsweep + j) * 6 + 3] = wall_clock64();
#endif

      // ---- write out: boundary nodes -> this sweep's partial slots (through
      // to memory), exclusive nodes -> the next iterate (registers; the last
      // sweep also stores it)
      T *const        out  = (j & 1 ? sw.slots[1] : sw.slots[0]);
      uint64_t *const gout = (j & 1 ? sw.gran[1] : sw.gran[0]);
      const uint32_t  tagw = sw.epoch + (uint32_t)j + 1u;
#pragma unroll
      for (int it = 0; it < NI; ++it)
        {
          const int i = t + it * BLOCK;
          if (i >= L)
            break;
          const int      iz  = idiv_f(i, a.rLxy), iy = idiv_f(i - iz * Lxy, a.rLx);
          const int      ip  = (i - iz * Lxy - iy * a.Lx) + a.PLx * (iy + a.PLy * iz);
          const uint32_t tgt = tgv[it];
          if (tgt == UNUSED_NODE)
            continue;
          T r[nc];
#pragma unroll
          for (int c = 0; c < nc; ++c)
            r[c] = (T)s_acc[c * LP + ip];
          if (tgt & SHARED_BIT)
            {
              // the last sweep's partials: plain slots, reduced after the
              // launch; the others: tagged granules for the neighbours
              if (last)
                store_node<T, nc>(out, tgt & ~SHARED_BIT, r);
              else
                store_granules(gout, sw.gran_bytes, tgt & ~SHARED_BIT, tagw, r);
              continue;
            }
          const uint32_t cm = pkv[it] >> 28;
#pragma unroll
          for (int c = 0; c < nc; ++c)
            {
              if ((cm >> c) & 1)
                r[c] = u[it][c];
              const T base = a.rkeep ? u[it][c] : T(0);
              r[c]         = base + a.romega * xd[it][c] * (xb[it][c] - r[c]);
              u[it][c]     = r[c];
            }
          if (last)
            {
              store_node<T, nc>((j & 1 ? sw.vec[0] : sw.vec[1]), tgt, r);
              if (a.out64)
                {
                  double r64[nc];
#pragma unroll
                  for (int c = 0; c < nc; ++c)
                    r64[c] = (double)r[c];
                  store_node<double, nc>(a.out64, tgt, r64);
                }
            }
        }
#if GLS_SWEEP_TIMING
      if (t == 0 && sw.timing)
        sw.timing[((size_t)brick * sw.nsweep + j) * 6 + 4] = wall_clock64();
#endif
    }
