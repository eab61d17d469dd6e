// What the trainers share (train_phasenet.hip, train_eqt_dec.hip): owned device arrays and the optimiser state with its one
// Adam launch (train_optim.hip).
#pragma once
#include "vp_common.h"

namespace vp {

// A device array that belongs to its holder: allocated (and zeroed where something reads it before a kernel has written it)
// in one statement, freed with the holder.  (DevBuf of api_handle.h is the other thing: it regrows, may carry a pinned host
// mirror, and is released by hand.)
template <class T>
struct DevArray {
  T* p = nullptr;
  DevArray() = default;
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n, bool zero = false) {
    const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    return e == hipSuccess && zero ? hipMemset(p, 0, n * sizeof(T)) : e;
  }
  operator T*() const { return p; }
};

// The flat parameter blob of a trainer with its gradient and torch.optim.Adam's state.  `who` is the entry point's name in
// the refusals.
struct OptimState {
  size_t n = 0;
  DevArray<float> w;     // weights (flat blob, canonical order)
  DevArray<float> grad, adam_m, adam_v;
  DevArray<float> mask;  // 1 = trainable, 0 = left alone by Adam (BatchNorm running statistics)
  DevArray<float> ema;   // EMA of the weights: unallocated unless the trainer has one and it is on
  long step = 0;         // updates so far
  float beta1 = 0.9f, beta2 = 0.999f, adam_eps = 1e-8f, ema_decay = 0.f;

  int alloc(size_t n_floats);  // everything but `ema`, zeroed
  // one Adam update of `w` from `grad` on `stream` (and of `ema`, where allocated); counted in `launches`
  void update(hipStream_t stream, float lr, int& launches);
  // which: 0 weights, 1 gradients of the last step, 2 Adam m, 3 Adam v, 4 EMA weights; max_which: 4 where the trainer can
  // have an EMA, else 3.  Waits for `stream`, then a blocking copy.
  int read(const char* who, int device, hipStream_t stream, int max_which, int which, float* out, size_t n_floats);
  // replaces `w` alone (moments, step and EMA stay), after waiting for `stream`
  int write(const char* who, int device, hipStream_t stream, const float* weights, size_t n_floats);
};

// (every comparison is false for a NaN; a caller stores nothing before this and its own checks have passed)
int check_hyper(const char* who, float beta1, float beta2, float adam_eps);

}  // namespace vp
