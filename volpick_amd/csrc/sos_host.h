// What the trace operations check and prepare on the host before they touch the device: the sample kind, the section
// coefficients as the kernels take them, the pole radius and the warm-up it asks for.  No HIP: tests/sos_host_check.cpp
// builds it with the host compiler.
#pragma once
#include <cmath>
#include <cstddef>

#include "vp_error.h"

namespace vp {

constexpr int DMAXS = 4;  // second-order sections the kernels are instantiated for

struct SosArg {
  double c[DMAXS][5];  // b0 b1 b2 a1 a2 (a0 == 1)
};

inline size_t elem_bytes(int kind) { return kind == VP_SAMPLES_FLOAT64 ? 8 : 4; }

inline int check_sample_kind(const char* who, int in_kind) {
  VP_REQUIRE(in_kind == VP_SAMPLES_INT32 || in_kind == VP_SAMPLES_FLOAT32 || in_kind == VP_SAMPLES_FLOAT64,
             "%s: in_kind %d is none of VP_SAMPLES_INT32 / FLOAT32 / FLOAT64", who, in_kind);
  return VP_OK;
}

// Largest pole radius of `ns` sections in scipy's six-column layout.
inline double sos_pole_radius(const double* sos, int ns) {
  double r = 0.0;
  for (int s = 0; s < ns; ++s) {
    const double a1 = sos[6 * s + 4], a2 = sos[6 * s + 5];
    const double disc = a1 * a1 - 4.0 * a2;
    double rs;
    if (disc < 0.0) {
      rs = std::sqrt(a2);  // complex pair: |z|^2 = a2
    } else {
      const double q = std::sqrt(disc);
      rs = std::fmax(std::fabs(-a1 + q), std::fabs(-a1 - q)) * 0.5;
    }
    r = std::fmax(r, rs);
  }
  return r;
}

// Samples after which the response to a wrong starting state has decayed by 2^-40: from the largest pole radius.
inline int warmup_length(const double* sos, int ns, double* r_out) {
  const double r = sos_pole_radius(sos, ns);
  *r_out = r;
  if (!(r < 1.0)) return -1;
  if (r < 1e-12) return 2 * ns;
  return (int)std::ceil(40.0 * std::log(2.0) / -std::log(r)) + 2 * ns;
}

// `n_sections` rows of scipy's layout (non-null) into `arg`, zero rows behind them; *radius: the largest pole radius.
// Whether that radius is acceptable is the caller's question.
inline int load_sos(const char* who, const double* sos, int n_sections, SosArg* arg, double* radius) {
  VP_REQUIRE(n_sections >= 1 && n_sections <= DMAXS, "%s: n_sections = %d, the kernel is built for 1..%d", who, n_sections,
             DMAXS);
  for (int s = 0; s < n_sections; ++s) {
    for (int i = 0; i < 6; ++i) VP_REQUIRE(std::isfinite(sos[6 * s + i]), "%s: section %d has a non-finite coefficient", who, s);
    VP_REQUIRE(sos[6 * s + 3] == 1.0, "%s: section %d has a0 = %g, need 1 (scipy's sos layout)", who, s, sos[6 * s + 3]);
    arg->c[s][0] = sos[6 * s + 0];
    arg->c[s][1] = sos[6 * s + 1];
    arg->c[s][2] = sos[6 * s + 2];
    arg->c[s][3] = sos[6 * s + 4];
    arg->c[s][4] = sos[6 * s + 5];
  }
  for (int s = n_sections; s < DMAXS; ++s)
    for (int i = 0; i < 5; ++i) arg->c[s][i] = 0.0;
  *radius = sos_pole_radius(sos, n_sections);
  return VP_OK;
}

}  // namespace vp
