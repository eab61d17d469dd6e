// What vp_sta_lta checks and prepares on the host before it touches the device: every argument, and the coefficients and
// the power table of the recursive type.  No HIP: tests/stalta_host_check.cpp builds it with the host compiler.
#pragma once
#include <cfloat>
#include <cstdint>

#include "sos_host.h"  // check_sample_kind, elem_bytes

namespace vp {

constexpr int STALTA_LEVELS = 16;        // doubling powers: 0..7 span the pieces of a tile, 8..15 the tiles of a carry chunk
constexpr int STALTA_PIECE = 32;         // samples per thread (DC of sos_tile.h)
constexpr int64_t STALTA_MAX_NLTA = 65536;

// The recursive type's two states, index 0 the short and 1 the long average: s <- a s + c x^2.
struct StaLtaRec {
  double c[2];                  // 1 / nsta, 1 / nlta
  double a[2];                  // 1 - c, rounded once: the factor the float64 rule itself multiplies by
  double pw[2][STALTA_LEVELS];  // a^(STALTA_PIECE 2^k)
};

// pw by squaring in long double (64-bit significand here): level k is off by about 2^(k + 5) 2^-64 relative before its one
// rounding to double, against the 2^(k + 5) 2^-53 that as many float64 multiplications may cost.  A power below the
// smallest double is 0: its term has left the sum.
inline void stalta_rec_table(int64_t nsta, int64_t nlta, StaLtaRec* r) {
  const int64_t w[2] = {nsta, nlta};
  for (int s = 0; s < 2; ++s) {
    r->c[s] = 1.0 / (double)w[s];
    r->a[s] = 1.0 - r->c[s];
    long double p = (long double)r->a[s];
    for (int sq = 1; sq < STALTA_PIECE; sq *= 2) p *= p;
    for (int k = 0; k < STALTA_LEVELS; ++k) {
      r->pw[s][k] = (double)p;
      p *= p;
    }
  }
}

inline bool stalta_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// Every argument of vp_sta_lta but the device index.  `who` is the entry point the refusal names.
inline int check_sta_lta(const char* who, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                         int type, int64_t nsta, int64_t nlta, const void* out_dev, int out_kind) {
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(out_kind == VP_SAMPLES_FLOAT32 || out_kind == VP_SAMPLES_FLOAT64,
             "%s: out_kind %d is neither VP_SAMPLES_FLOAT32 nor VP_SAMPLES_FLOAT64", who, out_kind);
  VP_REQUIRE(type == VP_STALTA_CLASSIC || type == VP_STALTA_RECURSIVE,
             "%s: type %d is neither VP_STALTA_CLASSIC nor VP_STALTA_RECURSIVE", who, type);
  VP_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
  VP_REQUIRE(n_series >= 1, "%s: n_series = %d, need at least 1", who, n_series);
  VP_REQUIRE(series_stride >= n, "%s: series_stride = %lld is below n = %lld", who, (long long)series_stride, (long long)n);
  VP_REQUIRE(nsta >= 1 && nsta <= nlta, "%s: need 1 <= nsta <= nlta, got nsta = %lld, nlta = %lld", who, (long long)nsta,
             (long long)nlta);
  VP_REQUIRE(n == 0 || (in_dev && out_dev), "%s: null argument", who);
  if (n > 0) {
    const size_t span = (size_t)(n_series - 1) * (size_t)series_stride + (size_t)n;
    VP_REQUIRE(!stalta_overlap(in_dev, span * elem_bytes(in_kind), out_dev, span * elem_bytes(out_kind)),
               "%s: out_dev overlaps in_dev", who);
  }
  if (nlta > STALTA_MAX_NLTA) {
    set_error("%s: nlta = %lld, the kernel takes windows up to %lld samples", who, (long long)nlta, (long long)STALTA_MAX_NLTA);
    return VP_ERR_UNSUPPORTED;
  }
  return VP_OK;
}

}  // namespace vp
