// Training-batch generation from a device-resident waveform bank (batchgen.hip): the pieces the trainer's
// vp_train_step_bank (train_phasenet.hip) shares with vp_bank_make_batch.
#pragma once
#include "vp_common.h"

namespace vp {

// Plan rows (vp_plan_row or vp_aug_row) staged for the device: pinned host slots copied to device slots on the launching
// stream.  The caller decides when a slot may be refilled (the host copy of slot k must have been read by the copy a
// previous use enqueued).
struct RowRing {
  static constexpr int N = 8;
  void* host[N] = {};
  void* dev[N] = {};
  size_t cap = 0;  // bytes per slot
  // Every slot is idle when this is called.  Grows the slots to hold `bytes`.
  int reserve(size_t bytes);
  // rows -> host[slot] -> dev[slot] (async on s); returns dev[slot]
  void* stage(int slot, const void* rows, size_t bytes, hipStream_t s);
  ~RowRing();
};

struct Bank {
  int device = 0;
  long long n_traces = 0, n_floats = 0;
  long long n_written = 0, floats_written = 0;  // traces are written in order: [0, n_written) hold data
  float* data = nullptr;          // trace i: (3, len[i]) fp32 at data + off[i]
  long long* off_dev = nullptr;   // [n_traces]
  long long* len_dev = nullptr;   // [n_traces]
  double* onset_dev = nullptr;    // [n_traces][4]: P, P, S, S in trace samples, NaN = no pick
  std::vector<long long> len;     // host copy of the written traces' lengths (row validation)
  RowRing ring;                   // vp_bank_make_batch's staging
  hipEvent_t ev[RowRing::N] = {}; // behind the kernel that read ring slot i
  bool ev_used[RowRing::N] = {};
  long long batches = 0;
  ~Bank();
};

// Checks every argument of one generation launch on the host; VP_ERR_INVALID (with the message set) on the first bad one.
int bank_check(const Bank& bk, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows);
// x, y: (B, 3, T) fp32 on the bank's device.  Arguments already checked by bank_check.
int bank_launch(const Bank& bk, const vp_plan_row* rows_dev, int B, int T, float sigma, int norm, const int* label_rows,
                float* x, float* y, hipStream_t s);
// x alone -- the rows cut, demeaned and normalised exactly as bank_launch does, no labels (vp_predict_bank).
int bank_check_windows(const Bank& bk, const vp_plan_row* rows, int B, int T, int norm);
int bank_launch_windows(const Bank& bk, const vp_plan_row* rows_dev, int B, int T, int norm, float* x, hipStream_t s);
// The same for augmented rows (vp_bank_make_batch_aug): bank_check's arguments plus every field of every vp_aug_row.
int bank_check_aug(const Bank& bk, const vp_aug_row* rows, int B, int T, float sigma, int norm, const int* label_rows);
int bank_launch_aug(const Bank& bk, const vp_aug_row* rows_dev, int B, int T, float sigma, int norm, const int* label_rows,
                    float* x, float* y, hipStream_t s);

}  // namespace vp
