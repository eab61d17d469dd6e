// Vector cross entropy of device-resident predictions in float64 (valloss.hip): what vp_vce_loss and the
// vp_validate_bank entry points (passes.hip) launch.
#pragma once
#include "vp_common.h"

namespace vp {

// Checks every argument of one loss launch on the host; VP_ERR_INVALID (with the message set) on the first bad one.
int vce_check(const float* p, const float* y, int B, int C, int T, double eps);
// per_window (B doubles) and batch (1 double) on the device, either may be null.  Arguments already checked by vce_check.
int vce_launch(const float* p, const float* y, int B, int C, int T, double eps, double* per_window, double* batch,
               hipStream_t s);

}  // namespace vp
