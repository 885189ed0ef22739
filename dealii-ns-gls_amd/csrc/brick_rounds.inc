// brick_rounds.inc — the cell rounds of the brick kernels (evaluate, q-point
// physics, integrate, lattice accumulation), included by brick_body.inc and
// brick_sweeps.inc after the src lattice is staged and round 0's LaneData
// (cur) is loaded or resident.  Leaves the brick's A src in s_acc.
  // the lane's tensor quadrature weight (Cartesian bricks: JxW = det J w_q)
  // (the three 1D weights are scalars of the kernel arguments, picked by
  // selects: the same values and products as a lookup by pa)
  // (opaque copies: a select between loads of kernel arguments would be
  // folded back into one per-lane load from a selected address)
  static_assert(n <= 4, "1D quadrature weights picked by selects");
  T w_0 = a.sh.w[0], w_1 = a.sh.w[n > 1 ? 1 : 0], w_2 = a.sh.w[n > 2 ? 2 : 0],
    w_3 = a.sh.w[n > 3 ? 3 : 0];
  asm volatile("" : "+s"(w_0), "+s"(w_1), "+s"(w_2), "+s"(w_3));
  const auto w1d = [&](int i) { return i == 1 ? w_1 : i == 2 ? w_2 : i == 3 ? w_3 : w_0; };
  T          wq_lane = w1d(pa[0]) * w1d(pa[1]);
  if (dim == 3)
    wq_lane *= w1d(pa[2]);
  // the cell rounds, compiled once per brick geometry G (GEO_CART: diagonal
  // J^{-1} and det J per cell; GEO_GEN: J^{-1} and JxW per q point)
  {
    // (GEO_ANY: one body for both, the geometry read per brick)
    const bool     gen   = general;
    // FOUR kernels: Cartesian bricks issue a round's loads at its start
    // (LATE), curved ones after its evaluate sweeps (AT_USE); the others
    // prefetch the next round's behind the Dq^T sweeps
    constexpr bool LATE  = FOUR && G == GEO_CART;
    constexpr bool ATUSE = FOUR && G == GEO_GEN;
    // the stages whose LDS reads are issued as batches (brick.h stage_batch)
    constexpr int  SBM   = stage_batch<dim, k, T, MODE, GEO, ZL>();
    // the gradient's batches: one pack's lines instead of a whole axis's
    [[maybe_unused]] constexpr bool GRAD_PACK = grad_by_pack<T, GEO>();
    for (int base = 0; base < ncell; base += step)
      {
        if (LATE && base > 0)
          load_lane<dim, k, T, MODE, G>(a, ks, rec, gen, base + wcell0, slot, in_wave, p, cur);
        const int  lcell = base + wave * CPW + slot;
        const bool act   = in_wave && lcell < ncell;
        // the lane's lattice node this round (inactive lanes: the first cell's)
        const int li = (act ? s_org[lcell] : 0) + lpa;
        // ---- evaluate: x sweep straight from the src lattice, then y (, z).
        // Each sweep reads its coefficient row once for every pack and issues
        // every pack's reads before the first store (a store could alias the
        // tables or the next pack's reads: interleaved, each pack would wait
        // one LDS round trip of its own)
        if constexpr (XD)
          {
            // every lane reads its own lattice node; the line's other two
            // come from the neighbouring lanes (xline)
            T kx[5];
            taps5<n>(s_tap, TAB_S, pa[0], kx);
            V r[NP];
#pragma unroll
            for (int kp = 0; kp < NP; ++kp)
              r[kp] = xline<T, V, W>(s_src[kp * LP + li], kx);
            if (in_wave)
#pragma unroll
              for (int kp = 0; kp < NP; ++kp)
                A[kp * BL::KS + q] = r[kp];
          }
        else if (in_wave)
          {
            T c[n];
            coefs<n>(sS, pa[0], c);
            V r[NP];
            contract_packs<(SBM & SB_SWEEP) != 0, n>(s_src, LP, c, li - pa[0], 1, r);
#pragma unroll
            for (int kp = 0; kp < NP; ++kp)
              A[kp * BL::KS + q] = r[kp];
          }
        wave_sync();
        V *in = A, *out = B;
#pragma unroll
        for (int ax = 1; ax < dim; ++ax)
          {
            if (in_wave)
              {
                T c[n];
                coefs<n>(sS, pa[ax], c);
                V r[NP];
                contract_packs<(SBM & SB_SWEEP) != 0, n>(in, BL::KS, c, q - pa[ax] * st[ax],
                                                         st[ax], r);
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  out[kp * BL::KS + q] = r[kp];
              }
            wave_sync();
            V *tmp = in;
            in     = out;
            out    = tmp;
          }
        // values and reference-space gradients (collocation derivative);
        // left-over lanes stay out of the reads (they would only add bank
        // conflicts in their ds_read_b128 lane groups)
        T val[nc], gref[nc][dim];
#pragma unroll
        for (int c = 0; c < nc; ++c)
          {
            val[c] = T(0);
#pragma unroll
            for (int ax = 0; ax < dim; ++ax)
              gref[c][ax] = T(0);
          }
        if constexpr (XD)
          {
            // x derivative across the lanes (every lane: idle ones read the
            // first slot's values), y and z from the buffer
            T kd[5];
            taps5<n>(s_tap, TAB_D, pa[0], kd);
#pragma unroll
            for (int kp = 0; kp < NP; ++kp)
              {
                const V v = in[kp * BL::KS + q];
                V       g[dim];
                g[0] = xline<T, V, W>(v, kd);
#pragma unroll
                for (int ax = 1; ax < dim; ++ax)
                  g[ax] = in_wave ? contract_v<n>(in + kp * BL::KS, sD, pa[ax], q - pa[ax] * st[ax],
                                                  st[ax]) :
                                    V{};
#pragma unroll
                for (int w = 0; w < W; ++w)
                  if (kp * W + w < nc)
                    {
                      val[kp * W + w] = v[w];
#pragma unroll
                      for (int ax = 0; ax < dim; ++ax)
                        gref[kp * W + w][ax] = g[ax][w];
                    }
              }
          }
        else if constexpr ((SBM & SB_GRAD) != 0)
          {
            // batched: the values, then per axis the Dq row and the lines of
            // every pack (or of one pack at a time, GRAD_PACK) in one batch
            if (in_wave)
              {
                V v[NP], g[NP][dim];
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  v[kp] = in[kp * BL::KS + q];
#pragma unroll
                for (int ax = 0; ax < dim; ++ax)
                  {
                    T c[n];
                    coefs<n>(sD, pa[ax], c);
                    if constexpr (GRAD_PACK)
                      {
#pragma unroll
                        for (int kp = 0; kp < NP; ++kp)
                          {
                            V d[1][n];
                            read_lines<n, 1>(in + kp * BL::KS, 0, q - pa[ax] * st[ax], st[ax], d);
                            __builtin_amdgcn_sched_barrier(0);
                            g[kp][ax] = contract_r<n>(c, d[0]);
                            __builtin_amdgcn_sched_barrier(0);
                          }
                      }
                    else
                      {
                        V d[NP][n];
                        read_lines<n, NP>(in, BL::KS, q - pa[ax] * st[ax], st[ax], d);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kp = 0; kp < NP; ++kp)
                          g[kp][ax] = contract_r<n>(c, d[kp]);
                        __builtin_amdgcn_sched_barrier(0);
                      }
                  }
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
#pragma unroll
                  for (int w = 0; w < W; ++w)
                    if (kp * W + w < nc)
                      {
                        val[kp * W + w] = v[kp][w];
#pragma unroll
                        for (int ax = 0; ax < dim; ++ax)
                          gref[kp * W + w][ax] = g[kp][ax][w];
                      }
              }
          }
        else if (in_wave)
#pragma unroll
          for (int kp = 0; kp < NP; ++kp)
            {
              const V v = in[kp * BL::KS + q];
              V       g[dim];
#pragma unroll
              for (int ax = 0; ax < dim; ++ax)
                g[ax] = contract_v<n>(in + kp * BL::KS, sD, pa[ax], q - pa[ax] * st[ax], st[ax]);
#pragma unroll
              for (int w = 0; w < W; ++w)
                if (kp * W + w < nc)
                  {
                    val[kp * W + w] = v[w];
#pragma unroll
                    for (int ax = 0; ax < dim; ++ax)
                      gref[kp * W + w][ax] = g[ax][w];
                  }
            }
        wave_sync();
        if constexpr (ATUSE)
          {
            // curved brick: this round's tables and geometry, issued now
            __builtin_amdgcn_sched_barrier(0);
            load_lane<dim, k, T, MODE, GEO_GEN>(a, ks, rec, true, base + wcell0, slot, in_wave, p,
                                                cur);
          }

        // ---- q-point physics (do_vmult_cell)
        // real-space gradients J^{-T} grad_ref (Cartesian: diagonal J^{-1})
        // (one branch around the whole transform: a GEO_ANY body decides per
        // brick, and a select per entry would cost a VALU op each)
        T gu[dim][dim], gp[dim];
        if (gen)
          {
#pragma unroll
            for (int c = 0; c < nc; ++c)
#pragma unroll
              for (int e = 0; e < dim; ++e)
                {
                  T s = 0;
#pragma unroll
                  for (int i = 0; i < dim; ++i)
                    s += cur.inv[i][e] * gref[c][i];
                  if (c < dim)
                    gu[c][e] = s;
                  else
                    gp[e] = s;
                }
          }
        else
          {
#pragma unroll
            for (int c = 0; c < nc; ++c)
#pragma unroll
              for (int e = 0; e < dim; ++e)
                {
                  const T s = cur.inv[e][e] * gref[c][e];
                  if (c < dim)
                    gu[c][e] = s;
                  else
                    gp[e] = s;
                }
          }
        if constexpr (ATUSE)
          {
            // J^{-1} parked in the lane's own sweep-buffer slots (A and B at
            // q, both packs: 8 values; J^{-1}_22 stays in registers) until the
            // test-function transform
            if (in_wave)
              {
                if constexpr (W == 2)
                  {
                    V m[4];
                    m[0][0] = cur.inv[0][0], m[0][1] = cur.inv[0][1];
                    m[1][0] = cur.inv[0][2], m[1][1] = cur.inv[1][0];
                    m[2][0] = cur.inv[1][1], m[2][1] = cur.inv[1][2];
                    m[3][0] = cur.inv[2][0], m[3][1] = cur.inv[2][1];
                    A[q] = m[0], A[BL::KS + q] = m[1], B[q] = m[2], B[BL::KS + q] = m[3];
                  }
                else
                  {
                    // FP32: two 4-value packs (one pack per point and half)
                    V m0, m1;
                    m0[0] = cur.inv[0][0], m0[1] = cur.inv[0][1];
                    m0[2] = cur.inv[0][2], m0[3] = cur.inv[1][0];
                    m1[0] = cur.inv[1][1], m1[1] = cur.inv[1][2];
                    m1[2] = cur.inv[2][0], m1[3] = cur.inv[2][1];
                    A[q] = m0, B[q] = m1;
                  }
              }
            __builtin_amdgcn_sched_barrier(0);
          }
        T vr[nc], gr[nc][dim];
        T d1 = cur.d1, d2 = cur.d2;
        if (delta_otf<k, MODE>() && !a.cw)
          {
            T u2 = 0;
#pragma unroll
            for (int d = 0; d < dim; ++d)
              u2 += cur.U[d] * cur.U[d];
            delta_qwise_fast(u2, cur.h, a.nu4, a.stau2, d1, d2);
          }
        if constexpr (MODE == MODE_NEWTON)
          qpoint_newton_t1<dim, T>(val, val[dim], gu, gp, cur.U, cur.GU, cur.T1, d1, d2, a.nu,
                                   a.w0, a.td, vr, gr);
        else
          qpoint_physics<dim, T, MODE>(val, val[dim], gu, gp, cur.U, cur.GU, cur.T1, cur.UT,
                                       cur.oldg, d1, d2, a.nu, a.w0, a.theta, a.td,
                                       a.have_prev, a.have_old_grad, vr, gr);
        // submit_value / submit_gradient (JxW, J^{-T}); inactive lanes: JxW 0
        const T JxW = gen ? (cur.active ? cur.JxW : T(0)) : (cur.active ? cur.JxW * wq_lane : T(0));
        T       wq[nc], ghat[dim][nc];
        if (gen)
          {
            if constexpr (ATUSE)
              {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (W == 2)
                  {
                    const V m0 = A[q], m1 = A[BL::KS + q], m2 = B[q], m3 = B[BL::KS + q];
                    cur.inv[0][0] = m0[0], cur.inv[0][1] = m0[1];
                    cur.inv[0][2] = m1[0], cur.inv[1][0] = m1[1];
                    cur.inv[1][1] = m2[0], cur.inv[1][2] = m2[1];
                    cur.inv[2][0] = m3[0], cur.inv[2][1] = m3[1];
                  }
                else
                  {
                    const V m0 = A[q], m1 = B[q];
                    cur.inv[0][0] = m0[0], cur.inv[0][1] = m0[1];
                    cur.inv[0][2] = m0[2], cur.inv[1][0] = m0[3];
                    cur.inv[1][1] = m1[0], cur.inv[1][2] = m1[1];
                    cur.inv[2][0] = m1[2], cur.inv[2][1] = m1[3];
                  }
              }
#pragma unroll
            for (int c = 0; c < nc; ++c)
              {
                wq[c] = vr[c] * JxW;
#pragma unroll
                for (int i = 0; i < dim; ++i)
                  {
                    T s = 0;
#pragma unroll
                    for (int e = 0; e < dim; ++e)
                      s += cur.inv[i][e] * gr[c][e];
                    ghat[i][c] = s * JxW;
                  }
              }
          }
        else
          {
            T sc[dim];
#pragma unroll
            for (int i = 0; i < dim; ++i)
              sc[i] = cur.inv[i][i] * JxW;
#pragma unroll
            for (int c = 0; c < nc; ++c)
              {
                wq[c] = vr[c] * JxW;
#pragma unroll
                for (int i = 0; i < dim; ++i)
                  ghat[i][c] = gr[c][i] * sc[i];
              }
          }

        // ---- integrate: Dq^T on the gradient part (two axes per exchange
        // through the A/B halves), then S^T sweeps z (, y); the x sweep is
        // fused with the accumulation into the brick lattice
        V wv[NP];
        to_packs<V, T, nc, NP, W>(wq, wv);
        if constexpr (XD)
          {
            // Dq^T along x across the lanes (every lane), y and z through
            // the A / B halves in one exchange; the terms in the LDS form's
            // order (x, y, z)
            T kdt[5];
            taps5<n>(s_tap, TAB_DT, pa[0], kdt);
            V g0[NP], g1[NP], g2[NP];
            to_packs<V, T, nc, NP, W>(ghat[0], g0);
            to_packs<V, T, nc, NP, W>(ghat[1], g1);
            to_packs<V, T, nc, NP, W>(ghat[2], g2);
#pragma unroll
            for (int kp = 0; kp < NP; ++kp)
              wv[kp] += xline<T, V, W>(g0[kp], kdt);
            if (in_wave)
#pragma unroll
              for (int kp = 0; kp < NP; ++kp)
                {
                  A[kp * BL::KS + q] = g1[kp];
                  B[kp * BL::KS + q] = g2[kp];
                }
            wave_sync();
            if (in_wave)
#pragma unroll
              for (int kp = 0; kp < NP; ++kp)
                {
                  wv[kp] += contract_v<n>(A + kp * BL::KS, sDT, pa[1], q - pa[1] * st[1], st[1]);
                  wv[kp] += contract_v<n>(B + kp * BL::KS, sDT, pa[2], q - pa[2] * st[2], st[2]);
                }
            wave_sync();
          }
        else
#pragma unroll
        for (int ax0 = 0; ax0 < dim; ax0 += 2)
          {
            if (in_wave)
              {
                V g0[NP];
                to_packs<V, T, nc, NP, W>(ghat[ax0], g0);
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  A[kp * BL::KS + q] = g0[kp];
                if (ax0 + 1 < dim)
                  {
                    V g1[NP];
                    to_packs<V, T, nc, NP, W>(ghat[(ax0 + 1) % dim], g1);
#pragma unroll
                    for (int kp = 0; kp < NP; ++kp)
                      B[kp * BL::KS + q] = g1[kp];
                  }
              }
            wave_sync();
            // batched (A/B builds only: no default kernel takes this path,
            // brick.h stage_batch): both axes' Dq^T rows and lines, A's then
            // B's, each pack's terms in the order of the unbatched form
            bool batched = false;
            if constexpr ((SBM & SB_DQT) != 0)
              if (ax0 + 1 < dim)
                {
                  batched = true;
                  if (in_wave)
                    {
                      const int ax1 = (ax0 + 1) % dim;
                      T         c0[n], c1[n];
                      V         d0[NP][n], d1[NP][n];
                      coefs<n>(sDT, pa[ax0], c0);
                      read_lines<n, NP>(A, BL::KS, q - pa[ax0] * st[ax0], st[ax0], d0);
                      coefs<n>(sDT, pa[ax1], c1);
                      read_lines<n, NP>(B, BL::KS, q - pa[ax1] * st[ax1], st[ax1], d1);
                      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                      for (int kp = 0; kp < NP; ++kp)
                        wv[kp] += contract_r<n>(c0, d0[kp]);
#pragma unroll
                      for (int kp = 0; kp < NP; ++kp)
                        wv[kp] += contract_r<n>(c1, d1[kp]);
                    }
                }
            if (!batched && in_wave)
#pragma unroll
              for (int kp = 0; kp < NP; ++kp)
                {
                  wv[kp] += contract_v<n>(A + kp * BL::KS, sDT, pa[ax0], q - pa[ax0] * st[ax0],
                                          st[ax0]);
                  if (ax0 + 1 < dim)
                    {
                      const int ax1 = (ax0 + 1) % dim;
                      wv[kp] += contract_v<n>(B + kp * BL::KS, sDT, pa[ax1],
                                              q - pa[ax1] * st[ax1], st[ax1]);
                    }
                }
            wave_sync();
          }
        if (in_wave)
#pragma unroll
          for (int kp = 0; kp < NP; ++kp)
            A[kp * BL::KS + q] = wv[kp];
        // the next round's geometry and tables: issued here (few registers
        // live), in flight during the S^T sweeps and the next evaluate (this
        // round's lattice position is kept: the prefetch overwrites cur)
        const int  li_now     = li;
        const bool active_now = cur.active;
        if (!LATE && !ATUSE && base + step < ncell)
          load_lane<dim, k, T, MODE, G>(a, ks, rec, gen, base + step + wcell0, slot, in_wave, p, cur);
        wave_sync();
        in  = A;
        out = B;
        // S^T along x of the lane's own point (XD: from the y sweep's
        // registers across the lanes; otherwise read from the buffer below)
        V xo[NP];
        if constexpr (XD)
          {
            // z sweep A -> B, then the y sweep into registers (every lane:
            // idle ones read the first slot's values) and x across the lanes
            if (in_wave)
              {
                T c[n];
                coefs<n>(sST, pa[2], c);
                V r[NP];
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  r[kp] = contract_c<n>(A + kp * BL::KS, c, q - pa[2] * st[2], st[2]);
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  B[kp * BL::KS + q] = r[kp];
              }
            wave_sync();
            T c[n];
            coefs<n>(sST, pa[1], c);
            T kst[5];
            taps5<n>(s_tap, TAB_ST, pa[0], kst);
#pragma unroll
            for (int kp = 0; kp < NP; ++kp)
              xo[kp] = xline<T, V, W>(contract_c<n>(B + kp * BL::KS, c, q - pa[1] * st[1], st[1]), kst);
          }
        else
#pragma unroll
        for (int ax = dim - 1; ax >= 1; --ax)
          {
            if (in_wave)
              {
                T c[n];
                coefs<n>(sST, pa[ax], c);
                V r[NP];
                contract_packs<(SBM & SB_SWEEP) != 0, n>(in, BL::KS, c, q - pa[ax] * st[ax],
                                                         st[ax], r);
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
                  out[kp * BL::KS + q] = r[kp];
              }
            wave_sync();
            V *tmp = in;
            in     = out;
            out    = tmp;
          }
        T cx[n];
        if constexpr (!XD)
          coefs<n>(sST, pa[0], cx);
        if constexpr (DET)
          {
            // deterministic accumulation (GLS_DETERMINISTIC): the round's
            // cells add into the lattice one after another in cell order,
            // plain read-modify-writes between workgroup barriers, instead of
            // LDS atomics in arrival order
            for (int turn = 0; turn < WPB * CPW; ++turn)
              {
                __syncthreads();
                if (active_now && wave * CPW + slot == turn)
#pragma unroll
                  for (int kp = 0; kp < NP; ++kp)
                    {
                      const V r = XD ? xo[kp] : contract_c<n>(in + kp * BL::KS, cx, q - pa[0], 1);
#pragma unroll
                      for (int w = 0; w < W; ++w)
                        if (kp * W + w < nc)
                          s_acc[(kp * W + w) * LP + li_now] += (double)r[w];
                    }
              }
            __syncthreads();
          }
        else if constexpr (!XD && (SBM & SB_XST) != 0)
          {
            // batched: the row (above) and both packs' lines before the first
            // ds_add (an LDS atomic orders every later LDS read behind it)
            if (active_now)
              {
                V r[NP];
                contract_packs<true, n>(in, BL::KS, cx, q - pa[0], 1, r);
#pragma unroll
                for (int kp = 0; kp < NP; ++kp)
#pragma unroll
                  for (int w = 0; w < W; ++w)
                    if (kp * W + w < nc)
                      lds_add(s_acc + (kp * W + w) * LP + li_now, (double)r[kp][w]);
              }
          }
        else if (active_now)
#pragma unroll
          for (int kp = 0; kp < NP; ++kp)
            {
              const V r = XD ? xo[kp] : contract_c<n>(in + kp * BL::KS, cx, q - pa[0], 1);
#pragma unroll
              for (int w = 0; w < W; ++w)
                if (kp * W + w < nc)
                  lds_add(s_acc + (kp * W + w) * LP + li_now, (double)r[w]);
            }
        wave_sync();
      }
  }
