// Weighted binary cross entropy (torch.nn.BCELoss, mean reduction, as the reference's EQTransformerLit.shared_step sums it
// over its three heads: volpick/model/models.py:538-549) of predictions that are already on the device, in float64:
//   term       = -( y max(log p, -100) + (1 - y) max(log(1 - p), -100) ),  p and y widened to double first
//   head[b][c] = (1/T) sum_t term,   L_b = sum_c w_c head[b][c],   batch = (1/B) sum_b L_b.
// Every window has T samples, so the batch value is sum_c w_c BCELoss(p[:, c], y[:, c]).
//
// Shaped as the vector cross entropy (valloss.hip; the two share loss_reduce.h), one row of T samples at a time: the order
// of every sum is fixed -- no atomics -- so the same input at the same addresses gives the same bits:
//   1. thread j of the window's workgroup (BCE_NTH threads) adds its terms of row c in ascending order: the scalar head
//      term j (the < 4 samples in front of the first 16-byte boundary), the float4 groups j, j + BCE_NTH, ... of the body,
//      each x, y, z, w, then the scalar tail term j.  Where p and y differ in their alignment mod 16 every term is a scalar
//      one, strided the same way;
//   2. the 64 partials of a wave by __shfl_down (32, 16, ..., 1), the wave sums by a tree in LDS;
//   3. L_b: w_0 head_0 + w_1 head_1 + ... in ascending c;
//   4. the batch: thread j adds L_j, L_{j + BCE_NTH}, ... in ascending order, then step 2 again.
// The clamp is torch's: max(l, -100) keeps a NaN l, so NaN, Inf and p outside [0, 1] go through as the formula takes them.
// Both logarithms of every element are taken, also where y is exactly 0 or 1.
#include <cmath>
#include <cstdint>

#include "bce.h"
#include "loss_reduce.h"

// every product and sum below rounds on its own, in whichever kernel it is compiled: the kernels agree to the bit
#pragma clang fp contract(off)

namespace vp {
namespace {

constexpr int BCE_NTH = 256;
constexpr int BCE_WAVES = BCE_NTH / 64;

struct BceWeights {
  double w[BCE_MAX_C];
};

__device__ __forceinline__ double clamped_log(double v) {
  const double l = log(v);
  return l < -100.0 ? -100.0 : l;  // std::max(l, -100.0) of torch's kernel: a NaN stays
}

__device__ __forceinline__ double bce_term(float pf, float yf) {
  const double p = (double)pf, y = (double)yf;
  return -(y * clamped_log(p) + (1.0 - y) * clamped_log(1.0 - p));
}

// Window b: its C head values (to head, when not null) and L_b, the same bits in every thread.
__device__ __forceinline__ double window_loss(const float* __restrict__ p, const float* __restrict__ y, long long b, int C, int T,
                                              const BceWeights& wt, double* __restrict__ head, double* red) {
  double L = 0.0;
  for (int c = 0; c < C; ++c) {
    const long long at = (b * C + c) * T;
    const double part = strided_partial<BCE_NTH>(p + at, y + at, T, [](float pi, float yi) { return bce_term(pi, yi); });
    const double h = block_sum<BCE_NTH>(part, red) / (double)T;
    if (head && threadIdx.x == 0) head[b * C + c] = h;
    L += wt.w[c] * h;
  }
  return L;
}

// One workgroup per window.
__global__ __launch_bounds__(BCE_NTH) void bce_window_kernel(const float* __restrict__ p, const float* __restrict__ y, int C, int T,
                                                             const BceWeights wt, double* __restrict__ head,
                                                             double* __restrict__ per_window) {
  __shared__ double red[BCE_WAVES];
  const double L = window_loss(p, y, blockIdx.x, C, T, wt, head, red);
  if (per_window && threadIdx.x == 0) per_window[blockIdx.x] = L;
}

// One workgroup: the mean of the B window values (step 4).
__global__ __launch_bounds__(BCE_NTH) void bce_batch_kernel(const double* __restrict__ per_window, int B, double* __restrict__ batch) {
  __shared__ double red[BCE_WAVES];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += BCE_NTH) acc += per_window[b];
  const double s = block_sum<BCE_NTH>(acc, red);
  if (threadIdx.x == 0) *batch = s / (double)B;
}

// The batch loss with nowhere to keep the window values: one workgroup walks the windows and thread b % BCE_NTH keeps
// L_b, so every sum has the order of the two kernels above (and their bits) -- at one compute unit's speed.
__global__ __launch_bounds__(BCE_NTH) void bce_batch_only_kernel(const float* __restrict__ p, const float* __restrict__ y, int B, int C,
                                                                 int T, const BceWeights wt, double* __restrict__ head,
                                                                 double* __restrict__ batch) {
  __shared__ double red[BCE_WAVES];
  double acc = 0.0;
  for (int b = 0; b < B; ++b) {
    const double L = window_loss(p, y, b, C, T, wt, head, red);
    if (b % BCE_NTH == (int)threadIdx.x) acc += L;
  }
  const double s = block_sum<BCE_NTH>(acc, red);
  if (threadIdx.x == 0) *batch = s / (double)B;
}

}  // namespace

int bce_check(const float* p, const float* y, int B, int C, int T, const double* weights) {
  VP_REQUIRE(p && y && weights, "bce loss: null p, y or weights");
  VP_REQUIRE(((uintptr_t)p & 3) == 0 && ((uintptr_t)y & 3) == 0, "bce loss: p and y must be 4-byte aligned");
  VP_REQUIRE(B >= 1, "bce loss: B = %d", B);
  VP_REQUIRE(C >= 1 && C <= BCE_MAX_C, "bce loss: C = %d outside [1, %d]", C, BCE_MAX_C);
  VP_REQUIRE(T >= 1, "bce loss: T = %d", T);
  for (int c = 0; c < C; ++c) VP_REQUIRE(std::isfinite(weights[c]), "bce loss: weights[%d] = %g is not finite", c, weights[c]);
  return VP_OK;
}

int bce_launch(const float* p, const float* y, int B, int C, int T, const double* weights, double* head, double* per_window,
               double* batch, hipStream_t s) {
  BceWeights wt{};
  for (int c = 0; c < C; ++c) wt.w[c] = weights[c];
  if (per_window || !batch) {
    if (per_window || head) hipLaunchKernelGGL(bce_window_kernel, dim3(B), dim3(BCE_NTH), 0, s, p, y, C, T, wt, head, per_window);
    if (batch) hipLaunchKernelGGL(bce_batch_kernel, dim3(1), dim3(BCE_NTH), 0, s, per_window, B, batch);
  } else {
    hipLaunchKernelGGL(bce_batch_only_kernel, dim3(1), dim3(BCE_NTH), 0, s, p, y, B, C, T, wt, head, batch);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("bce loss launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp

extern "C" int vp_bce_loss(int device_id, const float* p_dev, const float* y_dev, int B, int C, int T, const double* weights,
                           double* head_dev, double* per_window_dev, double* batch_dev, void* stream) {
  const int rc = vp::bce_check(p_dev, y_dev, B, C, T, weights);
  if (rc != VP_OK) return rc;
  VP_REQUIRE((((uintptr_t)head_dev | (uintptr_t)per_window_dev | (uintptr_t)batch_dev) & 7) == 0, "bce loss: outputs must be 8-byte aligned");
  VP_HIP(hipSetDevice(device_id));
  return vp::bce_launch(p_dev, y_dev, B, C, T, weights, head_dev, per_window_dev, batch_dev, reinterpret_cast<hipStream_t>(stream));
}
