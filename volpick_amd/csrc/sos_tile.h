// What the two recursive-filter kernels share (resample.hip: decimation by warm-up; sosfilt.hip: general filters by an
// exact carry): the cut of a pass into tiles and pieces, the padded LDS image of a tile, the section coefficients as a
// kernel argument (sos_host.h, with the host's checks) and one sample's recurrence.
#pragma once
#include "sos_host.h"  // DMAXS, SosArg
#include "vp_common.h"

namespace vp {

constexpr int DT = 256;         // threads per workgroup
constexpr int DC = 32;          // samples per thread (one piece)
constexpr int DTILE = DT * DC;  // samples per workgroup (one tile)

// Piece p of a tile image starts at double (DC + 1) p: lane l of a wave reads dword (2 DC + 2) l = 2 l (mod 64), so the
// 32 lanes of a ds_read_b64 group cover the 64 banks once.
__device__ __forceinline__ int phys(const int q) { return q + (q >> 5); }
static_assert(DC == 32, "phys() is written for pieces of 32");

// One sample through NS sections: direct form II transposed, the recurrence of scipy's sosfilt.
template <int NS>
__device__ __forceinline__ double sos_step(const SosArg& sos, double (&s1)[NS], double (&s2)[NS], double v) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double y = sos.c[s][0] * v + s1[s];
    s1[s] = sos.c[s][1] * v - sos.c[s][3] * y + s2[s];
    s2[s] = sos.c[s][2] * v - sos.c[s][4] * y;
    v = y;
  }
  return v;
}

}  // namespace vp
