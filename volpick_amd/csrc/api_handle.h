// What the files behind the C ABI share (api.hip: the stream path; passes.hip: the passes over a bank and the reducers of
// pre-cut windows): the handle, its grow-only buffers, and one batch through the forward pass.  Not installed.
#pragma once
#include <algorithm>

#include "net.h"
#include "prepost.h"

// Grow-only device buffer of `cap` elements, with MIRROR a mapped pinned host block `host` of the same size beside it.
// Growing drops the contents; zero_new clears a new device block (synchronously).
template <class T, bool MIRROR = false>
struct DevBuf {
  T *p = nullptr, *host = nullptr;
  size_t cap = 0;
  int reserve(size_t need, bool zero_new = false) {
    if (need <= cap) return VP_OK;
    release();
    VP_HIP(hipMalloc((void**)&p, need * sizeof(T)));
    if (zero_new) VP_HIP(hipMemset(p, 0, need * sizeof(T)));
    if (MIRROR) VP_HIP(hipHostMalloc((void**)&host, need * sizeof(T), hipHostMallocMapped));
    cap = need;
    return VP_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    if (host) (void)hipHostFree(host);
    p = host = nullptr;
    cap = 0;
  }
};
using MirroredBuf = DevBuf<char, true>;  // a trigger result block (vp::ScanLayout) and what the publish kernel copies it to

namespace vp {
struct Passes;                // passes.hip: the batch scratch and the results of the handle's passes over a bank
void passes_release(Passes*);  // (null: nothing to free)
}  // namespace vp

struct vp_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  vp::Net net;
  hipEvent_t ev[5] = {};
  float total_ms = 0.f;
  bool timing = false;  // stage events cost ~5 us of stream bubble each: off unless vp_set_timing(h, 1)
  float stage_ms[4] = {0.f, 0.f, 0.f, 0.f};
  // the window description of the latest preprocessing batch: the vp_profile_* calls replay it through plans whose first
  // launch cuts its windows itself -- after checking that what it points to is still allocated (pre_is_replayable)
  vp::PreArgs last_pre{};
  int last_pre_windows = 0;
  int last_out_lo = 0, last_out_hi = 0;  // ... and the kept output range of that batch (Net::out_lo / out_hi)
  // growable device scratch
  DevBuf<float> d_in;    // staged host input (stream or windows)
  DevBuf<float> d_pred;  // [n_windows][n_out][T] predictions of one annotate call
  DevBuf<float> d_out;   // stacked output when the caller's buffer is on the host
  // vp_classify_multi: tables (window table, block table, scan rows) and the result block
  DevBuf<char> d_tab;
  MirroredBuf m_pick;
  struct Slot {          // one in-flight vp_classify_submit
    MirroredBuf pick;    // trigger results; the host mirror is filled by ONE async copy per submit
    hipEvent_t done = nullptr;
    bool busy = false;
    int n_specs = 0, cap = 0;
    int64_t fv = -1, lv = -1, nwin = 0;
  } slot[VP_MAX_INFLIGHT];
  vp::Passes* passes = nullptr;  // made by the first vp_*_begin / _bank call
};

// Until the scope ends the last layer writes to `y` (null: where it writes anyway) and the plan is told that the caller
// keeps only the samples [out_lo, out_hi) of every window ((0, 0), the state outside any scope: all of them).
struct OutputRedirect {
  vp::Net& net;
  float* const y_saved;
  OutputRedirect(vp::Net& n, float* y, int out_lo = 0, int out_hi = 0) : net(n), y_saved(n.y) {
    if (y) net.y = y;
    net.out_lo = out_lo, net.out_hi = out_hi;
  }
  ~OutputRedirect() {
    net.y = y_saved;
    net.out_lo = net.out_hi = 0;
  }
};

namespace vp {

// The window description of one batch: `dense` windows back to back at src, or windows of a stream of N samples, `step`
// apart from window `first` on (api.hip).
PreArgs pre_args(const vp_handle* h, const float* src, int dense, long N, long step, long first, int preprocess);

// One batch through annotate_batch_pre + the forward pass (api.hip).
int run_batch(vp_handle* h, const PreArgs& pa, int nb);

}  // namespace vp
