// Pick-benchmark task 0: the picks of every threshold of a sweep from device-resident probabilities in one launch
// (sweep.hip): what vp_sweep_windows and the vp_sweep_bank pass (passes.hip) launch.
#pragma once
#include "vp_common.h"

namespace vp {

constexpr int SW_NTH = 256;              // threads of a workgroup: one workgroup per window
constexpr int SW_MAX_CHUNK = 25;         // samples of a border a thread owns, at most (odd: see sweep.hip)
constexpr int SW_MAX_T = SW_NTH * SW_MAX_CHUNK;  // the longest border the LDS row holds
static_assert(SW_MAX_T == VP_SWEEP_MAX_T, "the header documents the kernel's limit");
constexpr int SW_MAX_NT = 32;            // threshold pairs of one launch
constexpr int SW_MAX_K = 64;             // kept triggers per (window, phase, threshold)

struct SweepArgs {
  const float* prob;  // (B, n_rows, T) fp32 on the device
  int B, n_rows, T;
  int p_row, s_row;
  const int* lo;      // [B] on the device, or both null: [0, T)
  const int* hi;
  int NT, K;
  float thr_on[SW_MAX_NT], thr_off[SW_MAX_NT];
  int* count;         // [B][2][NT] on the device
  int* peak;          // [B][2][NT][K]
  float* value;       // [B][2][NT][K], or null
};

// Checks the shape arguments, the thresholds and, where given, the HOST copies of the borders; VP_ERR_INVALID (with the
// message set) on the first bad one.  Nothing the kernel indexes with is left unchecked.
int sweep_check(int B, int n_rows, int T, int p_row, int s_row, const int32_t* lo, const int32_t* hi, const float* thr_on,
                const float* thr_off, int NT, int K, const char* who);
// Arguments already checked by sweep_check.
int sweep_launch(const SweepArgs& a, hipStream_t s);

}  // namespace vp
