// Pure host logic of the C ABI (api.hip): how a stream is cut into windows, how a trigger result block is laid out,
// and how its rows are handed to the caller.  No HIP: tests/api_host_check.cpp builds it with the host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "pick_args.h"

namespace vp {

// The windows of one block of N samples: n_regular windows at i * step and, if they leave the end uncovered, one more
// flush with it at N - T.  No windows when N < T.
struct WindowPlan {
  int64_t N, step, n_regular = 0;
  int T, has_tail = 0;
  int64_t first_valid = -1, last_valid = -1;  // un-blinded output range: union of [start(i) + blind_l, start(i) + T - blind_r)
  WindowPlan(int64_t N_, int T_, int overlap, int blind_l, int blind_r) : N(N_), step(T_ - overlap), T(T_) {
    if (N < T) return;
    n_regular = (N - T) / step + 1;
    has_tail = ((n_regular - 1) * step + T < N) ? 1 : 0;
    first_valid = blind_l;
    last_valid = start(n_windows() - 1) + T - blind_r - 1;
  }
  int64_t n_windows() const { return n_regular + has_tail; }
  int64_t start(int64_t i) const { return i < n_regular ? i * step : N - T; }
};

// One row of a trigger result block as the host reads it.
struct ScanRow {
  int found;  // triggers the scan saw; the arrays hold min(found, cap) of them in the order they were appended
  const int64_t *on, *off, *peak;
  const float* value;
};

// The trigger result block: a counter header (two ints per row), then per row [on | off | peak : int64 x cap]
// [value : float x cap]; header and rows padded to 256 bytes.  publish_kernel / publish_table_kernel (prepost.hip) copy
// it to the host mirror by `header` and `per_spec`; every other reader and writer goes through args() and row().
struct ScanLayout {
  size_t header, per_spec, total;
  int cap;
  ScanLayout(int n_specs, int cap_) : cap(std::max(cap_, 1)) {
    header = ((size_t)n_specs * 2 * sizeof(int) + 255) / 256 * 256;
    per_spec = (size_t)cap * (3 * sizeof(int64_t) + sizeof(float));
    per_spec = (per_spec + 255) / 256 * 256;
    total = header + per_spec * n_specs;
  }
  // what the scan of `trace` writes row r of the device block with; caller_cap may be 0 (count only)
  PickArgs args(char* dev_base, int r, const float* trace, int64_t n, float thr_on, float thr_off, int caller_cap) const {
    PickArgs a{};
    a.trace = trace;
    a.n = n > 0 ? n : 0;
    a.thr_on = thr_on;
    a.thr_off = thr_off;
    a.on = (int64_t*)(dev_base + header + per_spec * r);
    a.off = a.on + cap;
    a.peak = a.off + cap;
    a.value = (float*)(a.peak + cap);
    a.cap = caller_cap;
    a.count = (int*)dev_base + 2 * r;
    return a;
  }
  ScanRow row(const char* host_base, int r) const {
    const int64_t* on = (const int64_t*)(host_base + header + per_spec * r);
    return ScanRow{((const int*)host_base)[2 * r], on, on + cap, on + 2 * cap, (const float*)(on + 3 * cap)};
  }
};

// Hands out rows [0, n_rows) of a host block: of each row its first min(found, row_cap) entries sorted by onset, until
// the caller's `cap` entries are written; entry(i, r) is told that output i came from row r.  Returns the number of
// triggers found, which a row holding more than row_cap raises to at least `overflow_total` (0: no such rule).
template <class Entry>
int collect_rows(const ScanLayout& L, const char* host_base, int n_rows, int row_cap, int64_t* on, int64_t* off,
                 int64_t* peak, float* value, int cap, int overflow_total, Entry&& entry) {
  int total = 0, written = 0;
  std::vector<int> order;
  for (int r = 0; r < n_rows; ++r) {
    const ScanRow t = L.row(host_base, r);
    total += t.found;
    const int m = std::min(t.found, row_cap);
    order.resize(m);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return t.on[x] < t.on[y]; });
    for (int k = 0; k < m && written < cap; ++k, ++written) {
      on[written] = t.on[order[k]];
      off[written] = t.off[order[k]];
      peak[written] = t.peak[order[k]];
      value[written] = t.value[order[k]];
      entry(written, r);
    }
    if (t.found > row_cap) total = std::max(total, overflow_total);
  }
  return total;
}

}  // namespace vp
