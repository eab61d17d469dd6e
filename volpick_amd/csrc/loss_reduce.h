// What the float64 loss kernels (valloss.hip, bce.hip) share: a thread's strided share of a sum of per-sample terms over two
// fp32 arrays, and the workgroup sum in a fixed order.  No atomics: the same input at the same addresses gives the same bits.
#pragma once
#include <cstdint>

#include "vp_common.h"

namespace vp {

// Sum of v over the workgroup of NTH threads, the same bits in every thread: the 64 partials of a wave by __shfl_down
// (32, 16, ..., 1), the wave sums by a tree in LDS.  `red`: NTH / 64 doubles of LDS.
template <int NTH>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();  // the previous sum has been read by everyone
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
#pragma unroll
  for (int s = NTH / 64 / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// This thread's share of sum_i term(p[i], y[i]), i in [0, n), added in ascending order: the scalar head term j (the head:
// the < 4 samples in front of the first 16-byte boundary), then the float4 groups j, j + NTH, ... of the body, each x, y, z,
// w, then the scalar tail term j.  Where p and y differ in their alignment mod 16 every term is a scalar one, strided the
// same way.  Every sum rounds on its own.
template <int NTH, class Term>
__device__ __forceinline__ double strided_partial(const float* __restrict__ p, const float* __restrict__ y, long long n, Term term) {
#pragma clang fp contract(off)
  const int j = threadIdx.x;
  double acc = 0.0;
  if ((((uintptr_t)p ^ (uintptr_t)y) & 15) != 0) {
    for (long long i = j; i < n; i += NTH) acc += term(p[i], y[i]);
    return acc;
  }
  long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long long nvec = (n - head) >> 2;
  const long long tail = head + 4 * nvec;
  if (j < head) acc += term(p[j], y[j]);
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  const float4* y4 = reinterpret_cast<const float4*>(y + head);
  for (long long v = j; v < nvec; v += NTH) {
    const float4 a = p4[v], b = y4[v];
    acc += term(a.x, b.x);
    acc += term(a.y, b.y);
    acc += term(a.z, b.z);
    acc += term(a.w, b.w);
  }
  if (tail + j < n) acc += term(p[tail + j], y[tail + j]);
  return acc;
}

}  // namespace vp
