// brick_lane.inc — a lane's place in the brick kernels: wavefront, cell
// slot, point, sweep buffers (from t; included by brick_setup.inc, and by
// brick_sweeps.inc inside its sweep loop from an opaque copy of t).
  const int  wave    = t >> 6, lane = t & 63;
  // the wavefront's first cell slot of a round in a scalar register (the
  // streamed loads' bases are scalar, brick.h load_lane)
  const int  wcell0  = __builtin_amdgcn_readfirstlane(wave) * CPW;
  // XD (3D Q2, brick.h xline): lane 16 r + 3 s + x holds point x of x-line
  // 5 r + s (cell (5 r + s) / 9, line (y, z) = its remainder); the 16th lane
  // of every row and lines 18, 19 idle.  Otherwise one lane per (cell, point)
  // in cell-major order, the 64 % nq left-over lanes idle.
  const int  lrow    = lane & 15, lsl = lrow / 3, lline = 5 * (lane >> 4) + lsl;
  const bool in_wave = XD ? lrow < 15 && lline < CPW * n * n : lane / nq < CPW;
  const int  slot    = XD ? (in_wave ? lline / (n * n) : CPW) : lane / nq;
  // idle lanes take a valid point (XD: 0) of the first slot's buffer
  const int  p       = XD ? (in_wave ? lrow - 3 * lsl + n * (lline - slot * n * n) : 0) : lane - slot * nq;
  // left-over lanes only read the first slot's buffer; every LDS store of
  // the sweeps is guarded by in_wave
  V         *A       = s_work + (wave * CPW + (in_wave ? slot : 0)) * WB;
  using BL           = BufLayout<dim, n, NP, XD>;
  V         *B       = A + NP * BL::KS;
  const int  pa[3]   = {p % n, (p / n) % n, dim == 3 ? p / (n * n) : 0};
  const int  st[3]   = {1, BL::PY, BL::PZ};               // buffer strides
  const int  q       = pa[0] + BL::PY * pa[1] + BL::PZ * pa[2]; // own slot
  const int  lpa     = pa[0] + a.PLx * (pa[1] + a.PLy * pa[2]);  // lattice offset in a cell
  const int  step    = CPW * WPB;
