// Weighted binary cross entropy of device-resident predictions in float64 (bce.hip): what vp_bce_loss and the
// vp_validate_eqt_bank entry point (passes.hip) launch.
#pragma once
#include "vp_common.h"

namespace vp {

constexpr int BCE_MAX_C = 8;

// Checks every argument of one loss launch on the host; VP_ERR_INVALID (with the message set) on the first bad one.
int bce_check(const float* p, const float* y, int B, int C, int T, const double* weights);
// head (B * C doubles), per_window (B doubles) and batch (1 double) on the device, each may be null; weights: C doubles on
// the host, read before the call returns.  Arguments already checked by bce_check.
int bce_launch(const float* p, const float* y, int B, int C, int T, const double* weights, double* head, double* per_window,
               double* batch, hipStream_t s);

}  // namespace vp
