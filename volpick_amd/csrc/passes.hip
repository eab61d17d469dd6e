// C ABI of libvolpick_hip.so (include/volpick_hip.h): the passes over a waveform bank -- validation loss (vp_validate_* for
// PhaseNet, vp_validate_eqt_* for EQTransformer), pick-benchmark tasks 1-3 (vp_predict_*) and the task-0 threshold sweep
// (vp_sweep_*) -- and the reducers of pre-cut windows (vp_pick_windows, vp_predict_windows, vp_sweep_windows).
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "api_handle.h"
#include "batchgen.h"
#include "bce.h"
#include "predict.h"
#include "sweep.h"
#include "valloss.h"

using vp::pre_args;
using vp::run_batch;

namespace vp {

// What a handle keeps for its passes.  The passes share the scratch of one batch: a handle is used by one thread at
// a time, and every batch is enqueued whole, in stream order, before the next one starts.  Their results are their own.
struct Passes {
  template <class T>
  struct Buf : DevBuf<T> {  // freed with the handle's passes
    ~Buf() { this->release(); }
  };
  // the latest batch of any pass: the windows, their labels (reserved by the first validation batch) and their
  // probabilities, (B, 3, T) each, and the staging of its plan rows (and borders)
  Buf<float> x, y, pred;
  StagingRing ring;
  struct Validation {  // one loss per batch, one per window and -- EQTransformer's -- three head values per window
    bool open = false;
    Buf<double> batch, window, head;
    long long n_batches = 0, n_windows = 0;
  };
  Validation val;  // vp_validate_begin ... vp_validate_end
  Validation veq;  // vp_validate_eqt_begin ... vp_validate_eqt_end
  struct {  // vp_predict_begin ... vp_predict_end: one record per window
    bool open = false;
    Buf<vp_predict_record> rec;
    long long n_windows = 0;
  } prd;
  struct {  // vp_sweep_begin ... vp_sweep_end: the thresholds and K it was opened with; per window 2 NT counts and 2 NT K
            // peaks (and values, when kept)
    bool open = false;
    int NT = 0, K = 0;
    bool keep_values = false;
    float thr_on[SW_MAX_NT] = {}, thr_off[SW_MAX_NT] = {};
    Buf<int32_t> count, peak;
    Buf<float> value;
    long long n_windows = 0;
  } swp;
};

void passes_release(Passes* p) { delete p; }

}  // namespace vp

namespace {

vp::Passes& passes_of(vp_handle* h) {
  if (!h->passes) h->passes = new vp::Passes();
  return *h->passes;
}

// Room for `need` values in a results array of a validation or prediction pass, its first `used` values kept.  Growing
// waits for the stream: the launches in flight write into the old block.
template <class T>
int grow_results(DevBuf<T>& b, size_t used, size_t need, hipStream_t s) {
  if (need <= b.cap) return VP_OK;
  VP_HIP(hipStreamSynchronize(s));
  DevBuf<T> old = b;
  b = DevBuf<T>();
  const int rc = b.reserve(std::max(need, 2 * old.cap));
  hipError_t e = hipSuccess;
  if (rc == VP_OK && used) e = hipMemcpy(b.p, old.p, used * sizeof(T), hipMemcpyDeviceToDevice);
  old.release();
  if (rc != VP_OK) return rc;
  VP_HIP(e);
  return VP_OK;
}

// The forward pass of B windows, cut and normalised, (B, 3, T) at x: in chunks of max_batch, the probabilities to pred.
int forward_chunks(vp_handle* h, const float* x, int B, float* pred) {
  vp::Net& net = h->net;
  const size_t in_w = (size_t)3 * net.in_samples, out_w = (size_t)net.n_out * net.in_samples;
  for (int b0 = 0; b0 < B; b0 += net.max_batch) {
    const OutputRedirect to_pred(net, pred + (size_t)b0 * out_w);
    const int rc = run_batch(h, pre_args(h, x + (size_t)b0 * in_w, 1, 0, 0, 0, 0), std::min(net.max_batch, B - b0));
    if (rc != VP_OK) return rc;
  }
  return VP_OK;
}

// One batch of B windows of a pass over a bank, arguments already checked.  Room for the batch (with its labels when
// `labels`), for what it stages and -- room_for_results() -- for its results: nothing is enqueued before all of it stands.
// Then `staged` goes to the device as one block `rows_dev`, generate(rows_dev, x, y) cuts and normalises the windows, the
// forward pass runs in chunks of max_batch, and reduce(rows_dev, pred, y) appends the pass's results.
template <class Room, class Generate, class Reduce>
int pass_batch(vp_handle* h, int B, bool labels, std::initializer_list<vp::StagingRing::Piece> staged, float* pred_out_dev,
               Room room_for_results, Generate generate, Reduce reduce) {
  vp::Net& net = h->net;
  vp::Passes& sc = passes_of(h);
  const size_t n_in = (size_t)B * 3 * net.in_samples, n_out = (size_t)B * net.n_out * net.in_samples;
  size_t bytes = 0;
  for (const auto& piece : staged) bytes += piece.bytes;
  int rc;
  if (n_in > sc.x.cap || (labels && n_in > sc.y.cap)) {
    VP_HIP(hipStreamSynchronize(h->stream));  // launches in flight read the old blocks
    if ((rc = sc.x.reserve(n_in)) != VP_OK || (rc = sc.pred.reserve(n_out)) != VP_OK) return rc;
    if (labels && (rc = sc.y.reserve(sc.x.cap)) != VP_OK) return rc;
  }
  if ((rc = room_for_results()) != VP_OK) return rc;
  static_assert(sizeof(vp_aug_row) >= sizeof(vp_plan_row) + 2 * sizeof(int32_t), "the slots are sized for the largest row");
  if ((rc = sc.ring.acquire(bytes, (size_t)net.max_batch * sizeof(vp_aug_row))) != VP_OK) return rc;

  const char* rows_dev = static_cast<const char*>(sc.ring.stage(staged, h->stream));
  if (!rows_dev) return VP_ERR_HIP;
  if ((rc = generate(rows_dev, sc.x.p, sc.y.p)) != VP_OK) return rc;
  if ((rc = forward_chunks(h, sc.x.p, B, sc.pred.p)) != VP_OK) return rc;
  if ((rc = reduce(rows_dev, sc.pred.p, sc.y.p)) != VP_OK) return rc;
  if ((rc = sc.ring.retire(h->stream)) != VP_OK) return rc;
  if (pred_out_dev) VP_HIP(hipMemcpyAsync(pred_out_dev, sc.pred.p, n_out * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return VP_OK;
}

// Which handles a pass over a bank is for and which call opens it.
struct PassKind {
  int model_kind;           // < 0: any
  const char* unsupported;  // the message for another model kind, with %s for the caller
  const char* begin;
};
const PassKind VALIDATION{VP_MODEL_PHASENET, "%s: only a PhaseNet handle has a validation loss", "vp_validate_begin"};
const PassKind VALIDATION_EQT{VP_MODEL_EQTRANSFORMER,
                              "%s: only an EQTransformer handle has this loss (vp_validate_bank is PhaseNet's)", "vp_validate_eqt_begin"};
const PassKind PREDICTION{-1, nullptr, "vp_predict_begin"};
const PassKind SWEEP{-1, nullptr, "vp_sweep_begin"};

// What every *_bank call of a pass opens with: the handle, the bank and `others` given, the right model, the pass `state`
// open, handle and bank on one device.  `who` is the caller, for the messages.
template <class State>
int bank_call_check(vp_handle* h, vp_bank* bank, bool others, const PassKind& kind, State vp::Passes::*state, const char* who) {
  VP_REQUIRE(h && bank && others, "%s: null argument", who);
  if (kind.model_kind >= 0 && h->net.model_kind != kind.model_kind) {
    vp::set_error(kind.unsupported, who);
    return VP_ERR_UNSUPPORTED;
  }
  VP_REQUIRE((passes_of(h).*state).open, "%s: no pass is open (%s)", who, kind.begin);
  const vp::Bank& bk = *reinterpret_cast<const vp::Bank*>(bank);
  VP_REQUIRE(bk.device == h->device, "%s: bank on device %d, handle on device %d", who, bk.device, h->device);
  return VP_OK;
}

// A validation batch behind its checks: generate -> forward -> loss(pred, y, heads, per window, per batch) of all B windows,
// the results appended to v (the three head values per window only with keep_heads).
template <class Loss>
int validation_batch(vp_handle* h, const vp::Bank& bk, vp::Passes::Validation& v, const vp::BatchSpec& spec, vp::BatchRows rows,
                     int B, bool keep_heads, float* pred_out_dev, Loss loss) {
  VP_HIP(hipSetDevice(h->device));
  const int rc = pass_batch(
      h, B, true, {{rows.p, rows.bytes(B)}}, pred_out_dev,
      [&] {
        int r = grow_results(v.batch, (size_t)v.n_batches, (size_t)v.n_batches + 1, h->stream);
        if (r == VP_OK) r = grow_results(v.window, (size_t)v.n_windows, (size_t)v.n_windows + B, h->stream);
        if (r == VP_OK && keep_heads) r = grow_results(v.head, (size_t)v.n_windows * 3, ((size_t)v.n_windows + B) * 3, h->stream);
        return r;
      },
      [&](const char* rows_dev, float* x, float* y) { return vp::bank_launch(bk, spec, rows.at(rows_dev), B, x, y, h->stream); },
      [&](const char*, const float* pred, const float* y) {
        return loss(pred, y, keep_heads ? v.head.p + v.n_windows * 3 : nullptr, v.window.p + v.n_windows, v.batch.p + v.n_batches);
      });
  if (rc != VP_OK) return rc;
  ++v.n_batches;
  v.n_windows += B;
  return VP_OK;
}

// vp_validate_bank(_aug): the vector cross-entropy of all B windows.
int validate_batch(vp_handle* h, vp_bank* bank, vp::BatchRows rows, int B, float sigma, int norm, const int* label_rows, double eps,
                   float* pred_out_dev, const char* who) {
  int rc = bank_call_check(h, bank, true, VALIDATION, &vp::Passes::val, who);
  if (rc != VP_OK) return rc;
  VP_REQUIRE(eps > 0.0, "%s: eps = %g must be > 0", who, eps);
  const vp::Bank& bk = *reinterpret_cast<const vp::Bank*>(bank);
  const int T = h->net.in_samples;
  const vp::BatchSpec spec{T, sigma, norm, vp::LABEL_PSN, label_rows};
  if ((rc = vp::bank_check(bk, spec, rows, B)) != VP_OK) return rc;
  return validation_batch(h, bk, passes_of(h).val, spec, rows, B, false, pred_out_dev,
                          [&](const float* pred, const float* y, double*, double* window, double* batch) {
                            return vp::vce_launch(pred, y, B, 3, T, eps, window, batch, h->stream);
                          });
}

// vp_validate_eqt_bank(_aug): the weighted BCE of all B windows.
int validate_eqt_batch(vp_handle* h, vp_bank* bank, vp::BatchRows rows, int B, float sigma, int norm, const int* label_rows,
                       float det_fixed_window, const double* weights, float* pred_out_dev, const char* who) {
  int rc = bank_call_check(h, bank, weights != nullptr, VALIDATION_EQT, &vp::Passes::veq, who);
  if (rc != VP_OK) return rc;
  const vp::Bank& bk = *reinterpret_cast<const vp::Bank*>(bank);
  const int T = h->net.in_samples;
  const vp::BatchSpec spec{T, sigma, norm, vp::LABEL_DET, label_rows, det_fixed_window};
  if ((rc = vp::bank_check(bk, spec, rows, B)) != VP_OK) return rc;
  double row_weights[3];  // weights are (detection, P, S); the kernel takes them by row of y
  for (int i = 0; i < 3; ++i) {
    VP_REQUIRE(std::isfinite(weights[i]), "%s: weights[%d] = %g is not finite", who, i, weights[i]);
    row_weights[label_rows[i]] = weights[i];
  }
  VP_REQUIRE(h->net.n_out == 3, "%s: the model has %d outputs, the labels 3", who, h->net.n_out);
  return validation_batch(h, bk, passes_of(h).veq, spec, rows, B, true, pred_out_dev,
                          [&](const float* pred, const float* y, double* heads, double* window, double* batch) {
                            return vp::bce_launch(pred, y, B, 3, T, row_weights, heads, window, batch, h->stream);
                          });
}

// What vp_predict_bank and vp_sweep_bank stage and generate alike: the plan rows, then the B lower and the B upper borders
// when there are any; the windows alone, no labels; and reduce(pred, lo_dev, hi_dev), the borders null when there are none.
template <class Room, class Reduce>
int window_batch(vp_handle* h, const vp::Bank& bk, const vp::BatchSpec& spec, const vp_plan_row* rows, const int32_t* lo,
                 const int32_t* hi, int B, float* pred_out_dev, Room room_for_results, Reduce reduce) {
  static_assert(sizeof(vp_plan_row) % alignof(int32_t) == 0, "the borders follow the rows in a ring slot");
  const size_t row_bytes = (size_t)B * sizeof(vp_plan_row), border_bytes = lo ? (size_t)B * sizeof(int32_t) : 0;
  return pass_batch(
      h, B, false, {{rows, row_bytes}, {lo, border_bytes}, {hi, border_bytes}}, pred_out_dev, room_for_results,
      [&](const char* rows_dev, float* x, float*) {
        return vp::bank_launch(bk, spec, reinterpret_cast<const vp_plan_row*>(rows_dev), B, x, nullptr, h->stream);
      },
      [&](const char* rows_dev, const float* pred, const float*) {
        const int* d_lo = lo ? reinterpret_cast<const int*>(rows_dev + row_bytes) : nullptr;
        return reduce(pred, d_lo, d_lo ? d_lo + B : nullptr);
      });
}

// ---- the reducers of pre-cut windows: their room in h->d_in, what goes up and what comes back ------------------------------
struct WindowScratch {
  const float* prob;   // on the device
  const int *lo, *hi;  // on the device; null where the caller gave none
  int32_t* results;    // `result_words` 4-byte words
};

// h->d_in as [prob copy if host][lo B][hi B][results]; the probabilities and whichever borders were given are uploaded.
int stage_windows(vp_handle* h, const float* prob, int prob_mem, size_t n_prob, const int32_t* lo, const int32_t* hi, int B,
                  size_t result_words, WindowScratch* w) {
  static_assert(sizeof(float) == sizeof(int32_t), "the scratch is counted in 4-byte words");
  const size_t need = (prob_mem == VP_MEM_HOST ? n_prob : 0) + (size_t)2 * B + result_words;
  const int rc = h->d_in.reserve(std::max(need, (size_t)h->net.max_batch * 3 * h->net.in_samples));
  if (rc != VP_OK) return rc;
  float* p = h->d_in.p;
  w->prob = prob;
  if (prob_mem == VP_MEM_HOST) {
    VP_HIP(hipMemcpyAsync(p, prob, n_prob * sizeof(float), hipMemcpyHostToDevice, h->stream));
    w->prob = p;
    p += n_prob;
  }
  int* d_lo = reinterpret_cast<int*>(p);
  int* d_hi = d_lo + B;
  w->results = d_hi + B;
  if (lo) VP_HIP(hipMemcpyAsync(d_lo, lo, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (hi) VP_HIP(hipMemcpyAsync(d_hi, hi, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  w->lo = lo ? d_lo : nullptr;
  w->hi = hi ? d_hi : nullptr;
  return VP_OK;
}

struct Download {
  void* host;  // null: not asked for
  const void* dev;
  size_t bytes;
};
int download_and_wait(vp_handle* h, std::initializer_list<Download> parts) {
  for (const Download& d : parts)
    if (d.host) VP_HIP(hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, h->stream));
  VP_HIP(hipStreamSynchronize(h->stream));
  return VP_OK;
}

// vp_validate_end and vp_validate_eqt_end: the results of the pass `state` down, as many as the arrays hold, and the pass
// closed.  `heads` is EQTransformer's; PhaseNet's call must be given per_window wherever it holds anything.
int validation_end(vp_handle* h, vp::Passes::Validation vp::Passes::*state, const PassKind& kind, const char* who, double* batch_losses,
                   long long cap, long long* n_batches, double* per_window, bool need_per_window, double* heads,
                   long long cap_windows, long long* n_windows) {
  VP_REQUIRE(h != nullptr, "%s: null handle", who);
  auto& v = passes_of(h).*state;
  VP_REQUIRE(v.open, "%s: no pass is open (%s)", who, kind.begin);
  VP_REQUIRE(cap >= 0 && cap_windows >= 0 && (cap == 0 || batch_losses) && (!need_per_window || cap_windows == 0 || per_window),
             "%s: null output arrays", who);
  VP_HIP(hipSetDevice(h->device));
  const long long nb = std::min(cap, v.n_batches), nw = std::min(cap_windows, v.n_windows);
  const int rc = download_and_wait(h, {{nb > 0 ? batch_losses : nullptr, v.batch.p, (size_t)nb * sizeof(double)},
                                       {nw > 0 ? per_window : nullptr, v.window.p, (size_t)nw * sizeof(double)},
                                       {nw > 0 ? heads : nullptr, v.head.p, (size_t)nw * 3 * sizeof(double)}});
  if (rc != VP_OK) return rc;
  if (n_batches) *n_batches = v.n_batches;
  if (n_windows) *n_windows = v.n_windows;
  v.open = false;
  return VP_OK;
}

void sweep_args(vp::SweepArgs& a, int B, int n_rows, int T, int p_row, int s_row, const float* thr_on, const float* thr_off,
                int NT, int K) {
  a.B = B, a.n_rows = n_rows, a.T = T, a.p_row = p_row, a.s_row = s_row, a.NT = NT, a.K = K;
  memcpy(a.thr_on, thr_on, NT * sizeof(float));
  memcpy(a.thr_off, thr_off, NT * sizeof(float));
}

}  // namespace

extern "C" {

// ---- validation loss ------------------------------------------------------------------------------------------------------
int vp_validate_begin(vp_handle* h) {
  VP_REQUIRE(h != nullptr, "vp_validate_begin: null handle");
  if (h->net.model_kind != VP_MODEL_PHASENET) {
    vp::set_error("vp_validate_begin: only a PhaseNet handle has a validation loss");
    return VP_ERR_UNSUPPORTED;
  }
  auto& v = passes_of(h).val;
  v.open = true;
  v.n_batches = v.n_windows = 0;  // (launches of an abandoned pass run ahead of this one's on the same stream)
  return VP_OK;
}

int vp_validate_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                     const int* label_rows, double eps, float* pred_out_dev) {
  return validate_batch(h, bank, rows, B, sigma, norm, label_rows, eps, pred_out_dev, "vp_validate_bank");
}

int vp_validate_bank_aug(vp_handle* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                         const int* label_rows, double eps, float* pred_out_dev) {
  return validate_batch(h, bank, rows, B, sigma, norm, label_rows, eps, pred_out_dev, "vp_validate_bank_aug");
}

int vp_validate_end(vp_handle* h, double* batch_losses, long long cap, long long* n_batches, double* per_window,
                    long long cap_windows, long long* n_windows) {
  return validation_end(h, &vp::Passes::val, VALIDATION, "vp_validate_end", batch_losses, cap, n_batches, per_window, true, nullptr,
                        cap_windows, n_windows);
}

// ---- EQTransformer's validation loss: detection, P and S heads (bce.hip) ----------------------------------------------------
// The counterpart of the reference's EQTransformerLit.shared_step (volpick/model/models.py:538-549) on block 1's batch.
int vp_validate_eqt_begin(vp_handle* h) {
  VP_REQUIRE(h != nullptr, "vp_validate_eqt_begin: null handle");
  if (h->net.model_kind != VP_MODEL_EQTRANSFORMER) {
    vp::set_error("vp_validate_eqt_begin: only an EQTransformer handle has this loss (vp_validate_begin is PhaseNet's)");
    return VP_ERR_UNSUPPORTED;
  }
  auto& v = passes_of(h).veq;
  v.open = true;
  v.n_batches = v.n_windows = 0;  // (launches of an abandoned pass run ahead of this one's on the same stream)
  return VP_OK;
}

int vp_validate_eqt_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm, const int* label_rows,
                         float det_fixed_window, const double* weights, float* pred_out_dev) {
  return validate_eqt_batch(h, bank, rows, B, sigma, norm, label_rows, det_fixed_window, weights, pred_out_dev,
                            "vp_validate_eqt_bank");
}

int vp_validate_eqt_bank_aug(vp_handle* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                             const int* label_rows, float det_fixed_window, const double* weights, float* pred_out_dev) {
  return validate_eqt_batch(h, bank, rows, B, sigma, norm, label_rows, det_fixed_window, weights, pred_out_dev,
                            "vp_validate_eqt_bank_aug");
}

int vp_validate_eqt_end(vp_handle* h, double* batch_losses, long long cap, long long* n_batches, double* per_window, double* heads,
                        long long cap_windows, long long* n_windows) {
  return validation_end(h, &vp::Passes::veq, VALIDATION_EQT, "vp_validate_eqt_end", batch_losses, cap, n_batches, per_window, false,
                        heads, cap_windows, n_windows);
}

// ---- tasks 1-3: per-window records (predict.hip) ----------------------------------------------------------------------------
// The counterpart of the loop in the reference's predict_step (volpick/model/models.py:454-480, :881-906).
int vp_predict_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int det_row, int p_row, int s_row,
                       int det_mode, const int32_t* lo, const int32_t* hi, vp_predict_record* out) {
  VP_REQUIRE(h && prob && out, "vp_predict_windows: null argument");
  VP_REQUIRE(prob_mem == VP_MEM_HOST || prob_mem == VP_MEM_DEVICE, "vp_predict_windows: prob_mem %d", prob_mem);
  VP_REQUIRE(((uintptr_t)prob & 3) == 0, "vp_predict_windows: prob must be 4-byte aligned");
  const int T = h->net.in_samples;
  int rc = vp::predict_check(B, n_rows, T, det_row, p_row, s_row, det_mode, lo, hi, "vp_predict_windows");
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(h->device));
  constexpr size_t rec_words = sizeof(vp_predict_record) / sizeof(int32_t);
  static_assert(sizeof(vp_predict_record) % sizeof(int32_t) == 0 && alignof(vp_predict_record) <= alignof(int32_t), "record layout");
  WindowScratch w;
  if ((rc = stage_windows(h, prob, prob_mem, (size_t)B * n_rows * T, lo, hi, B, (size_t)B * rec_words, &w)) != VP_OK) return rc;
  vp::PredictArgs a{};
  a.prob = w.prob, a.lo = w.lo, a.hi = w.hi;
  a.out = reinterpret_cast<vp_predict_record*>(w.results);
  a.B = B, a.n_rows = n_rows, a.T = T;
  a.det_row = det_row, a.p_row = p_row, a.s_row = s_row, a.det_mode = det_mode;
  if ((rc = vp::predict_launch(a, h->stream)) != VP_OK) return rc;
  return download_and_wait(h, {{out, a.out, (size_t)B * sizeof(vp_predict_record)}});
}

int vp_predict_begin(vp_handle* h) {
  VP_REQUIRE(h != nullptr, "vp_predict_begin: null handle");
  auto& v = passes_of(h).prd;
  v.open = true;
  v.n_windows = 0;  // (launches of an abandoned pass run ahead of this one's on the same stream)
  return VP_OK;
}

// generate -> forward -> the records of all B windows, appended.
int vp_predict_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, const int32_t* lo, const int32_t* hi, int B,
                    int norm, int det_row, int p_row, int s_row, float* pred_out_dev) {
  int rc = bank_call_check(h, bank, true, PREDICTION, &vp::Passes::prd, "vp_predict_bank");
  if (rc != VP_OK) return rc;
  auto& v = passes_of(h).prd;
  const vp::Bank& bk = *reinterpret_cast<const vp::Bank*>(bank);
  vp::Net& net = h->net;
  const int T = net.in_samples;
  const int det_mode = net.model_kind == VP_MODEL_PHASENET ? VP_DET_ONE_MINUS_NOISE : VP_DET_ROW;
  vp::BatchSpec spec;  // the windows alone, no labels
  spec.T = T, spec.norm = norm;
  rc = vp::bank_check(bk, spec, rows, B);
  if (rc == VP_OK) rc = vp::predict_check(B, net.n_out, T, det_row, p_row, s_row, det_mode, lo, hi, "vp_predict_bank");
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(h->device));

  vp::PredictArgs a{};
  a.B = B, a.n_rows = net.n_out, a.T = T;
  a.det_row = det_row, a.p_row = p_row, a.s_row = s_row, a.det_mode = det_mode;
  rc = window_batch(
      h, bk, spec, rows, lo, hi, B, pred_out_dev,
      [&] { return grow_results(v.rec, (size_t)v.n_windows, (size_t)v.n_windows + B, h->stream); },
      [&](const float* pred, const int* d_lo, const int* d_hi) {
        a.prob = pred, a.lo = d_lo, a.hi = d_hi;
        a.out = v.rec.p + v.n_windows;
        return vp::predict_launch(a, h->stream);
      });
  if (rc != VP_OK) return rc;
  v.n_windows += B;
  return VP_OK;
}

int vp_predict_end(vp_handle* h, vp_predict_record* out, long long cap, long long* n_windows) {
  VP_REQUIRE(h != nullptr, "vp_predict_end: null handle");
  auto& v = passes_of(h).prd;
  VP_REQUIRE(v.open, "vp_predict_end: no pass is open (vp_predict_begin)");
  VP_REQUIRE(cap >= 0 && (cap == 0 || out), "vp_predict_end: null output array");
  VP_HIP(hipSetDevice(h->device));
  const long long nw = std::min(cap, v.n_windows);
  const int rc = download_and_wait(h, {{nw > 0 ? out : nullptr, v.rec.p, (size_t)nw * sizeof(vp_predict_record)}});
  if (rc != VP_OK) return rc;
  if (n_windows) *n_windows = v.n_windows;
  v.open = false;
  return VP_OK;
}

// ---- task 0: the threshold sweep (sweep.hip) -----------------------------------------------------------------------------
int vp_sweep_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int p_row, int s_row, const int32_t* lo,
                     const int32_t* hi, const float* thr_on, const float* thr_off, int NT, int K, int32_t* count,
                     int32_t* peak, float* value) {
  VP_REQUIRE(h && prob && thr_on && thr_off && count && peak, "vp_sweep_windows: null argument");
  VP_REQUIRE(prob_mem == VP_MEM_HOST || prob_mem == VP_MEM_DEVICE, "vp_sweep_windows: prob_mem %d", prob_mem);
  VP_REQUIRE(((uintptr_t)prob & 3) == 0, "vp_sweep_windows: prob must be 4-byte aligned");
  const int T = h->net.in_samples;
  int rc = vp::sweep_check(B, n_rows, T, p_row, s_row, lo, hi, thr_on, thr_off, NT, K, "vp_sweep_windows");
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(h->device));
  const size_t n_cnt = (size_t)B * 2 * NT, n_pk = n_cnt * K;
  WindowScratch w;  // results: [count][peak][value if asked for]
  if ((rc = stage_windows(h, prob, prob_mem, (size_t)B * n_rows * T, lo, hi, B, n_cnt + n_pk * (value ? 2 : 1), &w)) != VP_OK) return rc;
  vp::SweepArgs a{};
  sweep_args(a, B, n_rows, T, p_row, s_row, thr_on, thr_off, NT, K);
  a.prob = w.prob, a.lo = w.lo, a.hi = w.hi;
  a.count = w.results;
  a.peak = a.count + n_cnt;
  a.value = value ? reinterpret_cast<float*>(a.peak + n_pk) : nullptr;
  if ((rc = vp::sweep_launch(a, h->stream)) != VP_OK) return rc;
  return download_and_wait(h, {{count, a.count, n_cnt * sizeof(int32_t)}, {peak, a.peak, n_pk * sizeof(int32_t)},
                               {value, a.value, n_pk * sizeof(float)}});
}

int vp_sweep_begin(vp_handle* h, const float* thr_on, const float* thr_off, int NT, int K, int keep_values) {
  VP_REQUIRE(h && thr_on && thr_off, "vp_sweep_begin: null argument");
  const vp::Net& net = h->net;
  // (B, the rows and the borders are each batch's: 1, 0 / 1 and none stand in for them here)
  const int rc = vp::sweep_check(1, net.n_out, net.in_samples, 0, 1, nullptr, nullptr, thr_on, thr_off, NT, K, "vp_sweep_begin");
  if (rc != VP_OK) return rc;
  auto& v = passes_of(h).swp;
  v.NT = NT, v.K = K, v.keep_values = keep_values != 0;
  memcpy(v.thr_on, thr_on, NT * sizeof(float));
  memcpy(v.thr_off, thr_off, NT * sizeof(float));
  v.open = true;
  v.n_windows = 0;  // (launches of an abandoned pass run ahead of this one's on the same stream)
  return VP_OK;
}

// generate -> forward -> the picks of all B windows at every threshold, appended.
int vp_sweep_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, const int32_t* lo, const int32_t* hi, int B, int norm,
                  int p_row, int s_row, float* pred_out_dev) {
  int rc = bank_call_check(h, bank, true, SWEEP, &vp::Passes::swp, "vp_sweep_bank");
  if (rc != VP_OK) return rc;
  auto& v = passes_of(h).swp;
  const vp::Bank& bk = *reinterpret_cast<const vp::Bank*>(bank);
  vp::Net& net = h->net;
  const int T = net.in_samples;
  vp::BatchSpec spec;  // the windows alone, no labels
  spec.T = T, spec.norm = norm;
  rc = vp::bank_check(bk, spec, rows, B);
  if (rc == VP_OK) rc = vp::sweep_check(B, net.n_out, T, p_row, s_row, lo, hi, v.thr_on, v.thr_off, v.NT, v.K, "vp_sweep_bank");
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(h->device));
  const size_t per_cnt = (size_t)2 * v.NT, per_pk = per_cnt * v.K, nw = (size_t)v.n_windows;
  vp::SweepArgs a{};
  sweep_args(a, B, net.n_out, T, p_row, s_row, v.thr_on, v.thr_off, v.NT, v.K);
  rc = window_batch(
      h, bk, spec, rows, lo, hi, B, pred_out_dev,
      [&] {
        int r = grow_results(v.count, nw * per_cnt, (nw + B) * per_cnt, h->stream);
        if (r == VP_OK) r = grow_results(v.peak, nw * per_pk, (nw + B) * per_pk, h->stream);
        if (r == VP_OK && v.keep_values) r = grow_results(v.value, nw * per_pk, (nw + B) * per_pk, h->stream);
        return r;
      },
      [&](const float* pred, const int* d_lo, const int* d_hi) {
        a.prob = pred, a.lo = d_lo, a.hi = d_hi;
        a.count = v.count.p + nw * per_cnt;
        a.peak = v.peak.p + nw * per_pk;
        a.value = v.keep_values ? v.value.p + nw * per_pk : nullptr;
        return vp::sweep_launch(a, h->stream);
      });
  if (rc != VP_OK) return rc;
  v.n_windows += B;
  return VP_OK;
}

int vp_sweep_end(vp_handle* h, int32_t* count, int32_t* peak, float* value, long long cap_windows, long long* n_windows) {
  VP_REQUIRE(h != nullptr, "vp_sweep_end: null handle");
  auto& v = passes_of(h).swp;
  VP_REQUIRE(v.open, "vp_sweep_end: no pass is open (vp_sweep_begin)");
  VP_REQUIRE(cap_windows >= 0 && (cap_windows == 0 || (count && peak)), "vp_sweep_end: null output arrays");
  VP_REQUIRE(!value || v.keep_values, "vp_sweep_end: the pass was opened without keep_values");
  VP_HIP(hipSetDevice(h->device));
  const size_t nw = (size_t)std::min(cap_windows, v.n_windows), per_cnt = (size_t)2 * v.NT, per_pk = per_cnt * v.K;
  const int rc = download_and_wait(h, {{nw ? count : nullptr, v.count.p, nw * per_cnt * sizeof(int32_t)},
                                       {nw ? peak : nullptr, v.peak.p, nw * per_pk * sizeof(int32_t)},
                                       {nw ? value : nullptr, v.value.p, nw * per_pk * sizeof(float)}});
  if (rc != VP_OK) return rc;
  if (n_windows) *n_windows = v.n_windows;
  v.open = false;
  return VP_OK;
}

// ---- one threshold, one row: the picks of pre-cut windows (prepost.hip) ------------------------------------------------------
// Replaces the per-sample Python loop of the reference's evaluate() (eval_taks0.py:96-142).
int vp_pick_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int row, const int32_t* lo,
                    const int32_t* hi, float thr_on, float thr_off, int K, int32_t* count, int32_t* peak,
                    float* value) {
  VP_REQUIRE(h && prob && count && peak && value, "null argument");
  VP_REQUIRE(B > 0 && K > 0 && n_rows > 0 && row >= 0 && row < n_rows, "bad shape arguments");
  VP_REQUIRE(thr_off <= thr_on, "thr_off must not exceed thr_on");
  VP_HIP(hipSetDevice(h->device));
  const int T = h->net.in_samples;
  const size_t n_pk = (size_t)B * K;
  WindowScratch w;  // results: [count B][peak B*K][value B*K]; lo and hi each on its own: the kernel clips them
  const int rc = stage_windows(h, prob, prob_mem, (size_t)B * n_rows * T, lo, hi, B, B + 2 * n_pk, &w);
  if (rc != VP_OK) return rc;
  vp::WindowPickArgs a{};
  a.prob = w.prob, a.lo = w.lo, a.hi = w.hi;
  a.B = B, a.n_rows = n_rows, a.T = T, a.row = row;
  a.thr_on = thr_on, a.thr_off = thr_off;
  a.K = K;
  a.count = w.results;
  a.peak = a.count + B;
  a.value = reinterpret_cast<float*>(a.peak + n_pk);
  VP_HIP(hipMemsetAsync(a.count, 0, B * sizeof(int), h->stream));
  vp::launch_window_pick(a, h->stream);
  return download_and_wait(h, {{count, a.count, B * sizeof(int)}, {peak, a.peak, n_pk * sizeof(int)}, {value, a.value, n_pk * sizeof(float)}});
}

}  // extern "C"
