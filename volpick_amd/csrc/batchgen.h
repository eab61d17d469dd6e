// Training-batch generation from a device-resident waveform bank (batchgen.hip): the pieces the trainer's
// vp_train_step_bank (train_phasenet.hip) and the passes over a bank (passes.hip) share with vp_bank_make_batch -- the
// staging rings, the bank, and one descriptor, one check and one launch for every recipe (BatchSpec, BatchRows).
#pragma once
#include <initializer_list>

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
  struct Piece {
    const void* p;
    size_t bytes;
  };
  // The pieces, back to back -> host[slot] -> dev[slot] (one copy, async on s); returns dev[slot], null (with the error
  // set) when the copy fails.
  void* stage(int slot, std::initializer_list<Piece> pieces, hipStream_t s);
  ~RowRing();
};

// A RowRing that frees its own slots: use number u takes slot u % N, which is idle again behind the event that retire()
// recorded when the slot was used last.  acquire -> stage -> the launches that read the slot -> retire; a use that fails
// before retire() leaves the slot to the next one.  (The trainer frees the slots of its RowRing behind its step events,
// which it keeps for other reasons: train_phasenet.hip.)
struct StagingRing {
  using Piece = RowRing::Piece;
  // The next slot, idle and at least `bytes` large.  Slots that are too small are grown to max(bytes, at_least) once
  // every used slot is idle.  Waits on the slots' events alone: right for any stream the uses were launched on.
  int acquire(size_t bytes, size_t at_least = 0);
  void* stage(std::initializer_list<Piece> pieces, hipStream_t s) { return ring.stage(slot(), pieces, s); }
  // Behind the last launch on s that reads the slot.
  int retire(hipStream_t s);
  ~StagingRing();

 private:
  RowRing ring;
  hipEvent_t ev[RowRing::N] = {};  // created by the first acquire()
  bool ev_used[RowRing::N] = {};
  long long uses = 0;
  int slot() const { return (int)(uses % RowRing::N); }
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
  std::vector<long long> off;     // ... and of their offsets (vp_bank_read)
  StagingRing ring;               // vp_bank_make_batch's staging
  StagingRing assemble_ring;      // vp_bank_assemble's tables and partial sums (assemble.hip)
  ~Bank();
};

// What a batch carries beside x: nothing (vp_predict_bank, vp_sweep_bank), PhaseNet's P, S and noise rows, or
// EQTransformer's detection box (SeisBench's DetectionLabeller), P and S.
enum LabelKind { LABEL_NONE, LABEL_PSN, LABEL_DET };

// One generation launch, whichever recipe: the window length, the label width, the normalisation and the labels.
struct BatchSpec {
  int T = 0;
  float sigma = 1.f;  // (LABEL_NONE: not read)
  int norm = 0;       // VP_NORM_PEAK or VP_NORM_STD
  LabelKind labels = LABEL_NONE;
  // the caller's three rows of y, unchecked until bank_check: P, S, noise (LABEL_PSN) or detection, P, S (LABEL_DET)
  const int* label_rows = nullptr;
  float det_fixed_window = -1.f;  // LABEL_DET; < 0: the detection runs from P to S + 1.4 (S - P); >= 0: that many samples from P
};

// The B rows of a batch, on the host or on the device: plan rows (block 1) or augmented rows (block 1, stacking, gap and
// second normalisation; they carry labels, and PhaseNet's hold T <= 3072).
struct BatchRows {
  const void* p;
  bool aug;
  BatchRows(const vp_plan_row* rows) : p(rows), aug(false) {}
  BatchRows(const vp_aug_row* rows) : p(rows), aug(true) {}
  size_t bytes(int B) const { return (size_t)B * (aug ? sizeof(vp_aug_row) : sizeof(vp_plan_row)); }
  BatchRows at(const void* copy) const {  // the same rows where they were copied to
    BatchRows r = *this;
    r.p = copy;
    return r;
  }
};

// Checks every argument of one generation launch on the host -- B, the spec, every field of every row against the bank;
// VP_ERR_INVALID (with the message set) on the first bad one.
int bank_check(const Bank& bk, const BatchSpec& spec, BatchRows rows, int B);
// x, y: (B, 3, T) fp32 on the bank's device (y unused with LABEL_NONE).  Arguments already checked by bank_check.
int bank_launch(const Bank& bk, const BatchSpec& spec, BatchRows rows_dev, int B, float* x, float* y, hipStream_t s);

}  // namespace vp
