// ilu_internal.h — the ILU(k) object shared by csrc/ilu.hip (the solves, the
// C ABI) and csrc/ilu_factor.hip (the numeric factorisation on the device).
#pragma once

#include "../../include/gls_op.h"
#include "common.h"
#include "ilu_plan.h"

namespace gls
{
struct DevTri
{
  int32_t *rp = nullptr, *ci = nullptr, *order = nullptr, *lev_ptr = nullptr;
  double  *v = nullptr;
};

// what k_ilu_store leaves for the host (host-mapped memory)
struct IluFactorStatus
{
  double  min_pivot; // min |u_ii| over the good pivots
  double  bad_value; // the pivot of bad_row
  int64_t bad_row;   // the smallest row with a zero or non-finite pivot, or -1
};

// the device copy of the plan's pattern, made at the first device
// factorisation
struct DevFactor
{
  int64_t *rp = nullptr, *diag = nullptr, *a_to_f = nullptr, *from_l = nullptr, *from_u = nullptr;
  int32_t *ci = nullptr;
  double  *val = nullptr;
  double  *part_min = nullptr; // [store blocks] partial min |pivot|
  int64_t *part_bad = nullptr; // [store blocks] partial smallest bad row
  int      store_blocks = 0;
  IluFactorStatus *h_status = nullptr, *d_status = nullptr;
  hipEvent_t       ev[4]    = {nullptr, nullptr, nullptr, nullptr};
  bool             ready    = false;
};
} // namespace gls

struct glsILU_
{
  gls::IluPlan   plan;
  gls::DevTri    L, U;
  gls::DevFactor F;
  double        *dinv      = nullptr;
  int            device    = 0;
  double         upload_ms = 0;
  bool           valid     = false; // false after a failed refactorisation
  bool           on_device = false; // the last factorisation ran on the device:
                                    // plan.val is stale until it is downloaded
  double         factor_kernels_ms = 0; // k_ilu_factor_* of the last device run
};

namespace gls
{
// csrc/ilu_factor.hip: the numeric phase on the device from d_vals [nnz_a];
// sets valid / on_device, plan.min_pivot, plan.numeric_ms; throws the host's
// message on a bad pivot
void ilu_factor_device(glsILU_ *ilu, const double *d_vals, hipStream_t st);
// plan.val <- the device values (after a device factorisation)
void ilu_factor_download(glsILU_ *ilu);
void ilu_factor_release(glsILU_ *ilu);
} // namespace gls
