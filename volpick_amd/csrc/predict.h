// Per-window scores of the pick-benchmark tasks 1-3 from device-resident probabilities (predict.hip): what
// vp_predict_windows and the vp_predict_bank pass (passes.hip) launch.
//
// score_p_or_s = p_max / s_max is NOT formed here: the record carries the two maxima and the host divides them in
// float32 (numpy's correctly rounded quotient, x / 0 = inf and 0 / 0 = NaN included) -- volpick_amd/evaluate.py.
#pragma once
#include "vp_common.h"

namespace vp {

struct PredictArgs {
  const float* prob;  // (B, n_rows, T) fp32 on the device
  int B, n_rows, T;
  int det_row, p_row, s_row;
  int det_mode;       // VP_DET_ONE_MINUS_NOISE / VP_DET_ROW
  const int* lo;      // [B] on the device, or both null: [0, T)
  const int* hi;
  vp_predict_record* out;  // [B] on the device
};

// The border rule of every per-window reduction (predict_check, sweep_check): lo and hi together or not at all, and every
// HOST border inside [0, T] and not empty.
int border_check(int B, int T, const int32_t* lo, const int32_t* hi, const char* who);
// Checks the shape arguments and, where given, the HOST copies of the borders; VP_ERR_INVALID (with the message set) on
// the first bad one.  Nothing the kernel indexes with is left unchecked.
int predict_check(int B, int n_rows, int T, int det_row, int p_row, int s_row, int det_mode, const int32_t* lo,
                  const int32_t* hi, const char* who);
// Arguments already checked by predict_check.
int predict_launch(const PredictArgs& a, hipStream_t s);

}  // namespace vp
