// Argument block of one trigger-scan row (prepost.hip).  Plain data, no HIP: the host-only logic of api_host.h and its
// stand-alone test build against this header alone.
#pragma once
#include <cstdint>

namespace vp {

struct PickArgs {
  const float* trace;
  long n;
  float thr_on, thr_off;
  int64_t *on, *off, *peak;
  float* value;
  int cap;
  int* count;
};

}  // namespace vp
