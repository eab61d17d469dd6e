// How an entry point of libvolpick_hip refuses an argument: the thread's error text and VP_REQUIRE.  No HIP, so host-only
// checks (tests/sos_host_check.cpp) can include it; VP_HIP lives in vp_common.h.
#pragma once
#include "../../include/volpick_hip.h"

namespace vp {

void set_error(const char* fmt, ...);

}  // namespace vp

#define VP_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      vp::set_error(__VA_ARGS__); \
      return VP_ERR_INVALID;      \
    }                             \
  } while (0)
