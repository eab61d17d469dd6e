// Host side of the exact carry of sosfilt.hip: the table M_k = A^(piece 2^k) of the filter's state-transition matrix.
// Plain C++, no device code: a stand-alone program can include it.
//
// A is close to defective for the filters that need the carry most (a 0.01 Hz high-pass at 100 Hz has its four poles
// within 3e-4 of 1, and A^8192 has entries of 240 although every pole is inside the unit circle).  Squaring such a
// matrix in plain float64 loses a factor ~8 per squaring: A^8192 came out 5.7e-7 off, a quarter of the filter's error
// bound.  The squarings therefore run in double-double (two float64 per number, ~106 bits) and only the table handed
// to the kernels is rounded to float64.
#pragma once
#include <cmath>
#include <cstring>

namespace vp {
namespace sosmat {

constexpr int MAXD = 8;              // state doubles: 2 per section, at most 4 sections
constexpr int STRIDE = MAXD * MAXD;  // doubles per matrix of the table: row-major d x d in the first d * d

struct DD {
  double hi, lo;
};

inline DD renorm(double s, double e) {  // |e| <= |s|
  const double hi = s + e;
  return {hi, e - (hi - s)};
}
inline DD dd_add(DD x, DD y) {
  const double s = x.hi + y.hi;
  const double b = s - x.hi;
  const double e = (x.hi - (s - b)) + (y.hi - b);  // the rounding error of s, exactly
  return renorm(s, e + (x.lo + y.lo));
}
inline DD dd_mul(DD x, DD y) {
  const double p = x.hi * y.hi;
  const double e = std::fma(x.hi, y.hi, -p);  // the rounding error of p, exactly
  return renorm(p, e + (x.hi * y.lo + x.lo * y.hi));
}

inline void dd_square(const DD* x, DD* y, int d) {
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      DD acc = {0.0, 0.0};
      for (int k = 0; k < d; ++k) acc = dd_add(acc, dd_mul(x[i * d + k], x[k * d + j]));
      y[i * d + j] = acc;
    }
}

// table[k * STRIDE + i * d + j] = (A^(2^(log2_piece + k)))[i][j] for k < levels, d = 2 ns.  A's column j is the state after
// one zero sample from the unit state j, by the recurrence of scipy's sosfilt (state order: s1, s2 of section 0, of
// section 1, ...).  sos: ns rows b0 b1 b2 a0 a1 a2 with a0 == 1.
inline void doubling_matrices(const double* sos, int ns, int log2_piece, int levels, double* table) {
  const int d = 2 * ns;
  DD a[STRIDE], b[STRIDE];
  for (int j = 0; j < d; ++j) {
    double z[MAXD] = {0};
    z[j] = 1.0;
    double v = 0.0;
    for (int s = 0; s < ns; ++s) {
      const double* c = sos + 6 * s;
      const double y = c[0] * v + z[2 * s];
      z[2 * s] = c[1] * v - c[4] * y + z[2 * s + 1];
      z[2 * s + 1] = c[2] * v - c[5] * y;
      v = y;
    }
    for (int i = 0; i < d; ++i) a[i * d + j] = {z[i], 0.0};
  }
  for (int k = 0; k < log2_piece; ++k) {
    dd_square(a, b, d);
    std::memcpy(a, b, sizeof(a));
  }
  std::memset(table, 0, sizeof(double) * (size_t)levels * STRIDE);
  for (int k = 0; k < levels; ++k) {
    for (int i = 0; i < d * d; ++i) table[k * STRIDE + i] = a[i].hi;
    dd_square(a, b, d);
    std::memcpy(a, b, sizeof(a));
  }
}

}  // namespace sosmat
}  // namespace vp
