// brick_body.inc — the body of gls::k_brick (csrc/brick.h), included once
// per brick geometry G inside the kernel: G = GEO_CART / GEO_GEN for the
// bricks of that geometry, GEO_ANY for a body that reads the type per brick.
// (A 4-wave mixed-geometry launch includes it twice behind a wave-uniform
// branch on the brick's type.  Sharing the body through a lambda or a device
// function measured 12-216 B/lane of spills: by-reference captures and the
// reference to the kernel argument defeat the register promotion.)
// Expects in scope: dim, k, T, MODE, GEO, ZL, DET (template parameters), G, a.
#include "brick_setup.inc"

  // ---- prologue.  In flight from brick_setup.inc: the brick's record (a
  // scalar load) and the coefficient image.  Then, back to back with no wait
  // between them: the lattice node ids and write-out targets, the src gather
  // (which needs the node ids: the one dependent memory round trip) and round
  // 0's geometry and tables, whose addresses come from the record alone.  The
  // staging waits for the gather; round 0's loads stay in flight behind it.
  // Every lane loads: lanes past the lattice's end read its last entry and
  // drop it, so no branch surrounds a load and the wait counters stay exact.
  const bool general = G == GEO_GEN || (G == GEO_ANY && rec.curved != 0);
  const int  ncell   = (int)rec.ncell;
  LaneData<dim, T, MODE> cur;
#if GLS_TAB_FIRST
  // the other placement (A/B build, brick.h GLS_TAB_FIRST): round 0's loads
  // ahead of the node ids; the staging then waits for them too
  if constexpr (!(FOUR && G == GEO_GEN))
    load_lane<dim, k, T, MODE, G>(a, ks, rec, general, wcell0, slot, in_wave, p, cur);
#endif
  constexpr int   NI = (BrickLattice<dim, k, ZL>::L + BLOCK - 1) / BLOCK;
  const uint32_t *bn = k_nodes + brick * (int64_t)L;
  const uint32_t *bt = k_target + brick * (int64_t)L;
  uint32_t        pk[NI], tg[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int      i  = t + it * BLOCK;
      const uint32_t ic = (uint32_t)(i < L ? i : L - 1) * 4u;
      const uint32_t pl = load_so(bn, ic), tl = load_so(bt, ic);
      pk[it]            = i < L ? pl : 0u;
      tg[it]            = i < L ? tl : 0u;
    }

  // ---- stage the brick's src values once per node (read_dof_values:
  // homogeneous constraints read as 0; the residual reads plain values).
  // The gather is issued before round 0's loads: vmcnt retires in order, so
  // the staging then waits for the gather only.
  const int Lxy = a.Lx * a.Ly;
  T         u[NI][nc];
  // deferred reduction of the previous apply (one 16-byte pack per node)
  constexpr bool QREC = sizeof(T) == 4 && !R && nc * sizeof(T) == 16;
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int      i    = t + it * BLOCK;
      const uint32_t node = pk[it] & NODE_MASK;
      if (!(QREC && a.qslots)) // (uniform)
        {
          // branch-free: lanes past the lattice's end and the unused lattice
          // nodes of a split brick load node 0; the staging drops it (a
          // select on the loaded value here would be turned into a branch
          // around the load)
          const bool used = i < L && node != UNUSED_NODE;
          load_node<T, nc>(a.src, used ? node : 0u, u[it]);
        }
      else if (QREC && i < L && node != UNUSED_NODE && (tg[it] & SHARED_BIT))
        {
          // the previous apply's shared-node reduction of this node, in
          // k_shared_reduce_cls's order and arithmetic (bitwise the same)
          const uint32_t slt = tg[it] & ~SHARED_BIT;
          const int      kc  = slot_class(a.rc, slt);
          const uint32_t m   = a.rc.mult[kc];
          const uint32_t b0  = a.rc.slot0[kc] + (slt - a.rc.slot0[kc]) / m * m;
          const V       *pp  = reinterpret_cast<const V *>(a.qslots);
          V              sum = {};
          uint32_t       j   = 0;
          for (; j + 4 <= m; j += 4)
            {
              const V x0 = pp[b0 + j], x1 = pp[b0 + j + 1], x2 = pp[b0 + j + 2],
                      x3 = pp[b0 + j + 3];
              sum += (x0 + x1) + (x2 + x3);
            }
          if (j + 2 <= m)
            {
              const V x0 = pp[b0 + j], x1 = pp[b0 + j + 1];
              sum += x0 + x1;
              j += 2;
            }
          if (j < m)
            sum += pp[b0 + j];
          const V        xs = reinterpret_cast<const V *>(a.qprev)[node];
          const V        bb = reinterpret_cast<const V *>(a.qb)[node];
          const V        dd = a.qd ? reinterpret_cast<const V *>(a.qd)[node] : V{} + T(1);
          const uint32_t cm = pk[it] >> 28;
#pragma unroll
          for (int w = 0; w < W; ++w)
            if ((cm >> w) & 1)
              sum[w] = xs[w];
          const V v = xs + a.qomega * dd * (bb - sum);
          reinterpret_cast<V *>(a.qsrc_w)[node] = v;
#pragma unroll
          for (int c = 0; c < nc; ++c)
            u[it][c] = v[c % W];
        }
      else if (i < L && node != UNUSED_NODE)
        load_node<T, nc>(a.src, node, u[it]);
      else
#pragma unroll
        for (int c = 0; c < nc; ++c)
          u[it][c] = T(0);
    }
  // FP32 (multigrid levels): the fused relaxation's operands b, d and the
  // unmodified src of the exclusive nodes are loaded here, behind the
  // gather, instead of after the cell rounds (one memory round trip less at
  // the end of every brick; FP64 has no registers to spare for them)
  // (two-layer bricks: two lattice chunks per thread; the operands' 24
  // registers would spill, so they are read at the write-out)
  constexpr bool PRE = sizeof(T) == 4 && !R && ZL == 1 && !FOUR;
  constexpr int  NPR = PRE ? NI : 1;
  T              xb[NPR][nc], xd[NPR][nc], xs[NPR][nc];
  if constexpr (PRE)
    {
#pragma unroll
      for (int it = 0; it < NI; ++it)
        {
          const int  i    = t + it * BLOCK;
          const bool excl = i < L && tg[it] != UNUSED_NODE && !(tg[it] & SHARED_BIT);
#pragma unroll
          for (int c = 0; c < nc; ++c)
            {
              xs[it][c] = u[it][c];
              xb[it][c] = T(0);
              xd[it][c] = T(1);
            }
          if (excl && a.rb)
            {
              load_node<T, nc>(a.rb, tg[it], xb[it]);
              if (a.rd)
                load_node<T, nc>(a.rd, tg[it], xd[it]);
            }
        }
    }
  // round 0's tables and geometry, behind the gather (FOUR: Cartesian bricks
  // only; curved bricks load theirs after the evaluate sweeps)
  // (FOUR curved bricks: after the evaluate sweeps; issuing their geometry
  // here instead measured the same, profiles/r05/explore/ab_lattice_pad.txt)
  if constexpr (!GLS_TAB_FIRST && !(FOUR && G == GEO_GEN))
    load_lane<dim, k, T, MODE, G>(a, ks, rec, general, wcell0, slot, in_wave, p, cur);
#if GLS_TAB_PREFETCH
  if constexpr (FOUR && MODE == MODE_NEWTON)
    if (step < ncell)
      {
        // this wave's round-1 chunk (its Newton field groups lead the chunk):
        // one dword per 128-byte line into the L2, younger than every load
        // the prologue and round 0 wait for
        using F             = Fields<dim>;
        constexpr int NGR   = (F::N + W - 1) / W;
        constexpr int BYTES = F::NEWTON * CPW * nq * (int)sizeof(T);
        const char   *c0 = reinterpret_cast<const char *>(
          a.tab_v + (int64_t)(rec.chunk0 + step / CPW + wave) * (NGR * CPW * nq));
        const uintptr_t b0 = (uintptr_t)c0 & ~(uintptr_t)127;
        const int       nl = (int)(((uintptr_t)c0 + BYTES - b0 + 127) / 128);
        const char     *pl = reinterpret_cast<const char *>(b0) + 128 * (lane < nl ? lane : nl - 1);
        // (inline asm: the builtin makes the compiler wait for every
        // outstanding load before the next LDS access -- it cannot tell the
        // landing area from the lattice -- and the prologue would wait for
        // round 0's tables; an unknown younger load only ever makes a
        // vmcnt wait cover one more load)
        const uint32_t lds_off = (uint32_t)(uintptr_t)(
          (__attribute__((address_space(3))) unsigned char *)s_pf);
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
                     :
                     : "v"(pl), "s"(lds_off)
                     : "m0");
      }
#endif
  // the coefficient tables' image to LDS (its load is older than the gather)
  if (t < NCOEF)
    s_tab[t] = coef_v;
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int i = t + it * BLOCK;
      if (i >= L)
        break;
      const int      iz = idiv_f(i, a.rLxy), iy = idiv_f(i - iz * Lxy, a.rLx);
      const int      ip = (i - iz * Lxy - iy * a.Lx) + a.PLx * (iy + a.PLy * iz);
      const uint32_t cm = pk[it] >> 28;
      // unused lattice nodes of a split brick stage zeros
      const bool     un = (pk[it] & NODE_MASK) == UNUSED_NODE;
#pragma unroll
      for (int c = 0; c < nc; ++c)
        {
          if (un || (!R && ((cm >> c) & 1)))
            u[it][c] = T(0);
          s_acc[c * LP + ip] = 0.0;
        }
      V v[NP];
      to_packs<V, T, nc, NP, W>(u[it], v);
#pragma unroll
      for (int kp = 0; kp < NP; ++kp)
        s_src[kp * LP + ip] = v[kp];
    }
  __syncthreads();

#include "brick_rounds.inc"
  __syncthreads();

  // ---- write out: exclusive nodes -> dst, boundary nodes -> partials
  // FP64 rows under STORE_WT_ROWS: the lane keeps its row and the lane pairs
  // store whole 32-byte rows together (store_rows_paired: every lane of the
  // wavefront takes part, with a row or without)
  constexpr bool PAIRS     = sizeof(T) == 8 && nc == 4;
  const bool     rows_slot = PAIRS && store_policy(a.stp, STP_SLOT) == STORE_WT_ROWS; // (uniform)
  const bool     rows_dst  = PAIRS && store_policy(a.stp, STP_DST) == STORE_WT_ROWS;
#pragma unroll
  for (int it = 0; it < NI; ++it)
    {
      const int      i   = t + it * BLOCK;
      const uint32_t tgt = tg[it];
      T              r[nc];
      T             *row = nullptr;
      if constexpr (PAIRS)
#pragma unroll
        for (int c = 0; c < nc; ++c)
          r[c] = T(0);
      if (i < L && tgt != UNUSED_NODE)
        {
          const int iz = idiv_f(i, a.rLxy), iy = idiv_f(i - iz * Lxy, a.rLx);
          const int ip = (i - iz * Lxy - iy * a.Lx) + a.PLx * (iy + a.PLy * iz);
          double    acc[nc];
#pragma unroll
          for (int c = 0; c < nc; ++c)
            acc[c] = s_acc[c * LP + ip];
          if (tgt & SHARED_BIT)
            {
#pragma unroll
              for (int c = 0; c < nc; ++c)
                r[c] = (T)(R ? -acc[c] : acc[c]);
              if (rows_slot)
                row = a.partial + (size_t)(tgt & ~SHARED_BIT) * nc;
              else
                store_node<T, nc>(a.partial, tgt & ~SHARED_BIT, r,
                                  store_policy(a.stp, STP_SLOT));
            }
          else
            {
              const uint32_t cm = pk[it] >> 28;
#pragma unroll
              for (int c = 0; c < nc; ++c)
                {
                  r[c] = (T)(R ? -acc[c] : acc[c]);
                  if ((cm >> c) & 1)
                    r[c] = R ? T(0) : (PRE ? xs[PRE ? it : 0][c] : a.src[(size_t)tgt * nc + c]);
                }
              if constexpr (PRE)
                {
                  if (a.rb)
#pragma unroll
                    for (int c = 0; c < nc; ++c)
                      {
                        const T base = a.rkeep ? xs[it][c] : T(0);
                        r[c]         = base + a.romega * xd[it][c] * (xb[it][c] - r[c]);
                      }
                }
              else if constexpr (!R)
                if (a.rb)
#pragma unroll
                  for (int c = 0; c < nc; ++c)
                    {
                      const size_t j    = (size_t)tgt * nc + c;
                      const T      base = a.rkeep ? a.src[j] : T(0);
                      r[c] = base + a.romega * (a.rd ? a.rd[j] : T(1)) * (a.rb[j] - r[c]);
                    }
              if (rows_dst)
                row = a.dst + (size_t)tgt * nc;
              else
                store_node<T, nc>(a.dst, tgt, r, store_policy(a.stp, STP_DST));
              if constexpr (sizeof(T) == 4 && !R)
                if (a.out64)
                  {
                    double r64[nc];
#pragma unroll
                    for (int c = 0; c < nc; ++c)
                      r64[c] = (double)r[c];
                    store_node<double, nc>(a.out64, tgt, r64, store_policy(a.stp, STP_DST));
                  }
            }
        }
      if constexpr (PAIRS)
        if (rows_slot || rows_dst)
          store_rows_paired(row, r, (t & 1) != 0);
    }
