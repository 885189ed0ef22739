// brick_setup.inc — the part of the brick kernels' bodies before the gather:
// LDS carving, coefficient tables, the lane's cell slot and point (included by
// brick_body.inc and brick_sweeps.inc).
// Expects in scope: dim, k, T, MODE, GEO, ZL, DET (template parameters), G, a, and
// what brick_entry.inc defines.
  using LDS          = BrickLDS<dim, k, T>;
  using V            = typename Pack<T>::V;
  constexpr int n    = k + 1;
  constexpr int nq   = LDS::nq;
  constexpr int nc   = LDS::nc;
  constexpr int W    = LDS::W;
  constexpr int NP   = LDS::NP;
  constexpr int CPW  = LDS::CPW;
  constexpr int WPB  = LDS::WPB;
  constexpr int WB   = LDS::WB;
  constexpr bool R   = MODE == MODE_RESIDUAL;
  constexpr bool FOUR = BrickOcc<dim, k, T, MODE, GEO, ZL>::four;
  static_assert(nq <= 64, "one cell must fit a wavefront");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int L      = k_L;  // lattice nodes (global order of brick_nodes)
  const int LP     = a.LP; // padded LDS lattice (bank-conflict-free x sweep)
  V        *s_src  = reinterpret_cast<V *>(smem);   // [NP][LP] brick src values
  V        *s_work = s_src + NP * LP;               // [WPB*CPW][WB]
  // the accumulator lattice is FP64 for both precisions: ds_add_f32 costs
  // ~10 us per FP32 vmult on gfx950 (racy plain-add ablation: 38.1 -> 28.2
  // us), ds_add_f64 next to nothing (40.1 -> 39.7 us)
  double   *s_acc  = reinterpret_cast<double *>(s_work + WPB * CPW * WB); // [nc][LP]
  constexpr int RP = CoefRow<T, n>::RP;
  constexpr bool XD = LDS::X; // x contractions across lanes (brick.h xline)
  T        *s_tap  = reinterpret_cast<T *>(reinterpret_cast<unsigned char *>(s_acc) +
                                     LDS::tab_offset(LP)); // [4][n][TAPS] (XD)
  T        *s_tab  = s_tap + LDS::NTAP;                    // [4][n][RP]
  const T  *sS     = s_tab + TAB_S * n * RP;
  const T  *sST    = s_tab + TAB_ST * n * RP;
  const T  *sD     = s_tab + TAB_D * n * RP;
  const T  *sDT    = s_tab + TAB_DT * n * RP;
  // lattice position of each brick cell's first node (cell-major order
  // x, y, z): one LDS read per round instead of per-lane divisions by the
  // runtime brick shape, which the compiler would hoist into registers
  int      *s_org  = reinterpret_cast<int *>(s_tab + 4 * n * RP); // [ORG]
  // landing area of the L2 prefetch (GLS_TAB_PREFETCH; never read)
  [[maybe_unused]] unsigned char *s_pf = reinterpret_cast<unsigned char *>(s_org + LDS::ORG);

  const int t = threadIdx.x;
  // the coefficient tables' image (one load per lane; every lane loads, the
  // lanes past the image a clamped entry they drop): issued here, not waited
  // for before the node ids and targets are requested.  The image goes to
  // LDS at the staging, below the gather, the oldest load in flight there.
  // (brick, rec and the k_ copies of kernel arguments: brick_entry.inc)
  constexpr int NCOEF  = 4 * n * RP;
  static_assert(NCOEF <= BLOCK, "one coefficient per thread");
  const T       coef_v = load_so(k_coef, (uint32_t)(t < NCOEF ? t : 0) * (uint32_t)sizeof(T));
  if constexpr (XD)
    if (t < 4 * n * TAPS)
      {
        // tap d = j - x of table row x: k_d = M[x][x + d], zero off the line
        const int  tb = t / (n * TAPS), x = (t / TAPS) % n, j = x + t % TAPS - 2;
        const bool v  = t % TAPS < 5 && j >= 0 && j < n;
        const int  jj = v ? j : 0;
        s_tap[t]      = !v ? T(0) :
                        tb == TAB_S  ? a.sh.S[x][jj] :
                        tb == TAB_ST ? a.sh.S[jj][x] :
                        tb == TAB_D  ? a.sh.Dq[x][jj] : a.sh.Dq[jj][x];
      }
  if (t < a.bx * a.by * a.bz && t < LDS::ORG)
    {
      const int cz = idiv_f(t, a.rbxy), rz = t - cz * a.bx * a.by;
      const int cy = idiv_f(rz, a.rbx), cx = rz - cy * a.bx;
      s_org[t]     = cx * k + a.PLx * (cy * k + a.PLy * cz * k);
    }
#include "brick_lane.inc"
