// Vector cross entropy (the reference's volpick/model/models.py:34-51) of predictions that are already on the device, in
// float64: L_b = -(1/T) sum_c sum_t y log((double)p + eps) per window, and the batch loss (1/B) sum_b L_b.
//
// A window's C*T samples are contiguous, so the two sums are one sum over n = C*T terms.  The order of every sum is fixed
// -- no atomics -- so the same input at the same addresses gives the same bits:
//   1. thread j of the window's workgroup (VCE_NTH threads) adds its terms in ascending order: the scalar head term j (the
//      head: the < 4 samples in front of the first 16-byte boundary), then the float4 groups j, j + VCE_NTH, ... of the body,
//      each x, y, z, w, then the scalar tail term j.  (Window b >= 1 of a (B, 3, 3001) array starts b * 36012 bytes in:
//      4-byte aligned only.)  Where p and y differ in their alignment mod 16 every term is a scalar one, strided the same way;
//   2. the 64 partials of a wave by __shfl_down (32, 16, ..., 1), the wave sums by a tree in LDS;
//   3. the batch: thread j adds L_j, L_{j + VCE_NTH}, ... in ascending order, then step 2 again.
// NaN and Inf go through as IEEE arithmetic takes them (0 * log(0 + ...) included), as numpy's do.
#include <cmath>
#include <cstdint>

#include "loss_reduce.h"
#include "valloss.h"

// every product and sum below rounds on its own, in whichever kernel it is compiled: the three kernels agree to the bit
#pragma clang fp contract(off)

namespace vp {
namespace {

constexpr int VCE_NTH = 256;
constexpr int VCE_WAVES = VCE_NTH / 64;

__device__ __forceinline__ double vce_term(float p, float y, double eps) { return (double)y * log((double)p + eps); }

// This thread's share of sum_i y[i] log(p[i] + eps), i in [0, n): step 1 of the header (loss_reduce.h).
__device__ __forceinline__ double window_partial(const float* __restrict__ p, const float* __restrict__ y, long long n,
                                                 double eps) {
  return strided_partial<VCE_NTH>(p, y, n, [eps](float pi, float yi) { return vce_term(pi, yi, eps); });
}

// One workgroup per window.
__global__ __launch_bounds__(VCE_NTH) void vce_window_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                             long long n, int T, double eps, double* __restrict__ per_window) {
  __shared__ double red[VCE_WAVES];
  const long long b = blockIdx.x;
  const double s = block_sum<VCE_NTH>(window_partial(p + b * n, y + b * n, n, eps), red);
  if (threadIdx.x == 0) per_window[b] = -s / (double)T;
}

// One workgroup: the mean of the B window values (step 3).
__global__ __launch_bounds__(VCE_NTH) void vce_batch_kernel(const double* __restrict__ per_window, int B,
                                                            double* __restrict__ batch) {
  __shared__ double red[VCE_WAVES];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += VCE_NTH) acc += per_window[b];
  const double s = block_sum<VCE_NTH>(acc, red);
  if (threadIdx.x == 0) *batch = s / (double)B;
}

// The batch loss alone, with nowhere to keep the window values: one workgroup walks the windows and thread b % VCE_NTH
// keeps L_b, so every sum has the order of the two kernels above (and their bits) -- at one compute unit's speed.
__global__ __launch_bounds__(VCE_NTH) void vce_batch_only_kernel(const float* __restrict__ p, const float* __restrict__ y, int B,
                                                                 long long n, int T, double eps, double* __restrict__ batch) {
  __shared__ double red[VCE_WAVES];
  double acc = 0.0;
  for (int b = 0; b < B; ++b) {
    const double s = block_sum<VCE_NTH>(window_partial(p + (long long)b * n, y + (long long)b * n, n, eps), red);
    if (b % VCE_NTH == (int)threadIdx.x) acc += -s / (double)T;
  }
  const double s = block_sum<VCE_NTH>(acc, red);
  if (threadIdx.x == 0) *batch = s / (double)B;
}

}  // namespace

int vce_check(const float* p, const float* y, int B, int C, int T, double eps) {
  VP_REQUIRE(p && y, "vce loss: null p or y");
  VP_REQUIRE(((uintptr_t)p & 3) == 0 && ((uintptr_t)y & 3) == 0, "vce loss: p and y must be 4-byte aligned");
  VP_REQUIRE(B >= 1, "vce loss: B = %d", B);
  VP_REQUIRE(C >= 1 && C <= 8, "vce loss: C = %d outside [1, 8]", C);
  VP_REQUIRE(T >= 1, "vce loss: T = %d", T);
  VP_REQUIRE(eps > 0.0, "vce loss: eps = %g must be > 0", eps);  // (a NaN fails the comparison too)
  return VP_OK;
}

int vce_launch(const float* p, const float* y, int B, int C, int T, double eps, double* per_window, double* batch,
               hipStream_t s) {
  const long long n = (long long)C * T;
  if (per_window) {
    hipLaunchKernelGGL(vce_window_kernel, dim3(B), dim3(VCE_NTH), 0, s, p, y, n, T, eps, per_window);
    if (batch) hipLaunchKernelGGL(vce_batch_kernel, dim3(1), dim3(VCE_NTH), 0, s, per_window, B, batch);
  } else if (batch) {
    hipLaunchKernelGGL(vce_batch_only_kernel, dim3(1), dim3(VCE_NTH), 0, s, p, y, B, n, T, eps, batch);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("vce loss launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp

extern "C" int vp_vce_loss(int device_id, const float* p_dev, const float* y_dev, int B, int C, int T, double eps,
                           double* per_window_dev, double* batch_dev, void* stream) {
  const int rc = vp::vce_check(p_dev, y_dev, B, C, T, eps);
  if (rc != VP_OK) return rc;
  VP_REQUIRE(((uintptr_t)per_window_dev & 7) == 0 && ((uintptr_t)batch_dev & 7) == 0, "vce loss: outputs must be 8-byte aligned");
  VP_HIP(hipSetDevice(device_id));
  return vp::vce_launch(p_dev, y_dev, B, C, T, eps, per_window_dev, batch_dev, reinterpret_cast<hipStream_t>(stream));
}
