// The per-window reductions of the reference's predict_step (volpick/model/models.py:454-480 and :881-906) on
// probabilities that are already on the device: for window b and its border [lo, hi) one vp_predict_record with
//   det            max_t (1 - noise[t]) (VP_DET_ONE_MINUS_NOISE: every 1 - x is the fp32 subtraction torch performs, then the
//                  maximum) or max_t det[t] (VP_DET_ROW);
//   p_max, s_max   the maxima of the P and S rows;
//   p_arg, s_arg   where they are, relative to lo.
// Maximum and argmax follow torch on the CPU: a NaN is above every number, and among equal values (-0 == +0) or among
// NaNs the lowest index wins; the maximum is the value AT that index.  That order is total, so whichever way the partial
// results are combined the record is the same: no atomics, the same bits every run.
//
// One workgroup of PW_NTH threads per window.  Per row, thread j takes the scalar head element j (the < 4 samples in front
// of the row's first 16-byte boundary: lo is arbitrary and a (B, 3, 3001) row starts 4-byte aligned only), the float4 groups
// j, j + PW_NTH, ... of the body, and the scalar tail element j; then __shfl_down within the wave, a tree in LDS across the
// waves, and thread 0 writes the record.  The kernel is bound by the 3 (hi - lo) 4 bytes it reads per window.
#include <climits>
#include <cmath>

#include "predict.h"

namespace vp {
namespace {

constexpr int PW_NTH = 256;
constexpr int PW_WAVES = PW_NTH / 64;

struct Best {
  float v;
  int i;
};

// Does (bv, bi) come before (av, ai) in torch's order?
__device__ __forceinline__ bool beats(float bv, int bi, float av, int ai) {
  const bool bn = bv != bv, an = av != av;
  if (bn != an) return bn;
  if (!bn && bv != av) return bv > av;
  return bi < ai;
}
__device__ __forceinline__ void take(Best& a, float v, int i) {
  if (beats(v, i, a.v, a.i)) a.v = v, a.i = i;
}

// This thread's best of f(p[0 .. n)), f(x) = 1 - x (ONE_MINUS) or x.  A thread without an element returns (-inf, INT_MAX),
// which every element beats.
template <bool ONE_MINUS>
__device__ __forceinline__ Best row_partial(const float* __restrict__ p, int n) {
  const int j = threadIdx.x;
  Best a{-INFINITY, INT_MAX};
  int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  const int tail = head + 4 * nvec;
  auto f = [](float x) { return ONE_MINUS ? 1.0f - x : x; };
  if (j < head) take(a, f(p[j]), j);
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  for (int v = j; v < nvec; v += PW_NTH) {
    const float4 q = p4[v];
    const int i = head + 4 * v;
    take(a, f(q.x), i);
    take(a, f(q.y), i + 1);
    take(a, f(q.z), i + 2);
    take(a, f(q.w), i + 3);
  }
  if (tail + j < n) take(a, f(p[tail + j]), tail + j);
  return a;
}

__global__ __launch_bounds__(PW_NTH) void predict_windows_kernel(const PredictArgs a) {
  __shared__ float red_v[3][PW_WAVES];
  __shared__ int red_i[3][PW_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = a.lo ? a.lo[b] : 0;
  const int n = (a.hi ? a.hi[b] : a.T) - lo;
  const float* w = a.prob + (long long)b * a.n_rows * a.T + lo;

  Best r[3];  // det, P, S
  const float* det = w + (long long)a.det_row * a.T;
  r[0] = a.det_mode == VP_DET_ONE_MINUS_NOISE ? row_partial<true>(det, n) : row_partial<false>(det, n);
  r[1] = row_partial<false>(w + (long long)a.p_row * a.T, n);
  r[2] = row_partial<false>(w + (long long)a.s_row * a.T, n);

#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take(r[k], __shfl_down(r[k].v, o, 64), __shfl_down(r[k].i, o, 64));
    if ((tid & 63) == 0) red_v[k][tid >> 6] = r[k].v, red_i[k][tid >> 6] = r[k].i;
  }
  __syncthreads();
#pragma unroll
  for (int s = PW_WAVES / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (beats(red_v[k][tid + s], red_i[k][tid + s], red_v[k][tid], red_i[k][tid]))
          red_v[k][tid] = red_v[k][tid + s], red_i[k][tid] = red_i[k][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    vp_predict_record rec;
    rec.det = red_v[0][0];
    rec.p_max = red_v[1][0];
    rec.s_max = red_v[2][0];
    rec.p_arg = red_i[1][0];
    rec.s_arg = red_i[2][0];
    a.out[b] = rec;
  }
}

}  // namespace

int border_check(int B, int T, const int32_t* lo, const int32_t* hi, const char* who) {
  VP_REQUIRE((lo == nullptr) == (hi == nullptr), "%s: lo and hi come together or not at all", who);
  if (lo)
    for (int b = 0; b < B; ++b)
      VP_REQUIRE(lo[b] >= 0 && hi[b] <= T && hi[b] > lo[b], "%s: window %d: border [%d, %d) is empty or outside [0, %d]", who,
                 b, (int)lo[b], (int)hi[b], T);
  return VP_OK;
}

int predict_check(int B, int n_rows, int T, int det_row, int p_row, int s_row, int det_mode, const int32_t* lo,
                  const int32_t* hi, const char* who) {
  VP_REQUIRE(B >= 1, "%s: B = %d", who, B);
  VP_REQUIRE(T >= 1, "%s: T = %d", who, T);
  VP_REQUIRE(n_rows >= 3 && n_rows <= 64, "%s: n_rows = %d outside [3, 64]", who, n_rows);
  for (int r : {det_row, p_row, s_row}) VP_REQUIRE(r >= 0 && r < n_rows, "%s: row %d outside [0, %d)", who, r, n_rows);
  VP_REQUIRE(det_row != p_row && det_row != s_row && p_row != s_row, "%s: rows (%d, %d, %d) are not distinct", who, det_row,
             p_row, s_row);
  VP_REQUIRE(det_mode == VP_DET_ONE_MINUS_NOISE || det_mode == VP_DET_ROW, "%s: unknown det_mode %d", who, det_mode);
  return border_check(B, T, lo, hi, who);
}

int predict_launch(const PredictArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(predict_windows_kernel, dim3(a.B), dim3(PW_NTH), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("predict_windows_kernel launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp
