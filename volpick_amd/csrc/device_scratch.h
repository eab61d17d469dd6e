// Host scaffolding of the stand-alone trace operations (mseed.hip, resample.hip, fourier.hip, attributes.hip,
// sosfilt.hip): the device scratch an operation keeps per device between calls, and the stream and events of its
// _bench entry.
#pragma once
#include <mutex>

#include "vp_common.h"

namespace vp {

// One grow-only device allocation.  The caller holds the mutex of the DeviceScratch it belongs to.
struct ScratchBlock {
  void* p = nullptr;
  size_t cap = 0;
  // *out: at least `bytes`.  A block that has to grow is freed and allocated anew with `slack` bytes to spare: its
  // contents do not survive.  `who` is the entry point the failure text names.
  int grow(const char* who, size_t bytes, size_t slack, void** out) {
    if (bytes > cap) {
      release();
      const size_t want = bytes + slack;
      if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();  // the failure is reported here: do not leave HIP's sticky last error for an unrelated later check
        p = nullptr;
        set_error("%s: cannot allocate %zu bytes of device scratch", who, want);
        return VP_ERR_NOMEM;
      }
      cap = want;
    }
    *out = p;
    return VP_OK;
  }
  size_t release() {
    if (p) (void)hipFree(p);
    const size_t freed = cap;
    p = nullptr;
    cap = 0;
    return freed;
  }
};

// The scratch of one operation on one device.  A call holds `mu` from its first use of the blocks to its last.  Each
// operation keeps a pool of its own,
//     DeviceScratch<N>& x_scratch(int device) { static DeviceScratch<N> pool[64]; return pool[(unsigned)device % 64]; }
// so that its release call frees what it allocated and nothing else.
template <int SLOTS>
struct DeviceScratch {
  std::mutex mu;
  ScratchBlock b[SLOTS];
};

// The body of every vp_*_release_scratch.
template <int SLOTS>
int release_scratch(const char* who, DeviceScratch<SLOTS>& sc, int device_id, size_t* bytes_freed) {
  VP_REQUIRE(device_id >= 0, "%s: device index", who);
  std::lock_guard<std::mutex> lock(sc.mu);  // behind any call in flight on this device
  VP_HIP(hipSetDevice(device_id));
  size_t freed = 0;
  for (ScratchBlock& b : sc.b) freed += b.release();
  if (bytes_freed) *bytes_freed = freed;
  return VP_OK;
}

// The stream and the two events of a _bench entry, destroyed on every way out of it.
struct BenchTimer {
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  BenchTimer() = default;
  BenchTimer(const BenchTimer&) = delete;
  BenchTimer& operator=(const BenchTimer&) = delete;
  ~BenchTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
  }
  hipError_t init() {
    hipError_t e = hipStreamCreate(&s);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    return e;
  }
  // `launch` (-> hipError_t) `reps` times on s, untimed
  template <typename F>
  hipError_t run(int reps, F launch) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < reps && e == hipSuccess; ++i) e = launch();
    return e;
  }
  // *ms: mean time of one of `iters` launches
  template <typename F>
  hipError_t time(int iters, F launch, float* ms) {
    float t = 0.f;
    hipError_t e = hipEventRecord(e0, s);
    if (e == hipSuccess) e = run(iters, launch);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e == hipSuccess) *ms = t / iters;
    return e;
  }
};

}  // namespace vp
