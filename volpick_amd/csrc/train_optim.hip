// The optimiser of both trainers: adam_kernel (its one definition), the bias correction in front of its launch, and the host
// copies of the state (train_optim.h).
#include "train_optim.h"

#include <cmath>

namespace vp {

// torch.optim.Adam (no weight decay, no amsgrad); `mask` = 1 for trainable entries, 0 for the BN running statistics.
// ema (may be null): exponential moving average of the weights after the step, ema = d * ema + (1 - d) * w
// (the reference's optional EMA callback, volpick/model/train.py:153-176, decay 0.999, every step); the running
// statistics are buffers, not parameters: their EMA slots simply track the current values.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ mask, float* __restrict__ ema, int n, float lr,
                                                   float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   float ema_decay) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float wi = w[i];
  if (mask[i] != 0.f) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    wi -= (lr / bc1) * (mi / denom);
    w[i] = wi;
    if (ema) ema[i] = ema_decay * ema[i] + (1.f - ema_decay) * wi;
  } else if (ema) {
    ema[i] = wi;
  }
}

int OptimState::alloc(size_t n_floats) {
  n = n_floats;
  for (DevArray<float>* a : {&w, &grad, &adam_m, &adam_v, &mask}) VP_HIP(a->alloc(n, true));
  return VP_OK;
}

void OptimState::update(hipStream_t stream, float lr, int& launches) {
  step += 1;
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  ++launches;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w.p, grad.p, adam_m.p, adam_v.p, mask.p, ema.p,
                     (int)n, lr, beta1, beta2, adam_eps, bc1, sqrtf(bc2), ema_decay);
}

int OptimState::read(const char* who, int device, hipStream_t stream, int max_which, int which, float* out, size_t n_floats) {
  VP_REQUIRE(n_floats == n && which >= 0 && which <= max_which, "%s: bad size or selector", who);
  VP_REQUIRE(which != 4 || ema.p, "%s: EMA is off (vp_train_set_ema)", who);
  const DevArray<float>* const src[] = {&w, &grad, &adam_m, &adam_v, &ema};
  VP_HIP(hipSetDevice(device));
  VP_HIP(hipStreamSynchronize(stream));
  VP_HIP(hipMemcpy(out, src[which]->p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
  return VP_OK;
}

int OptimState::write(const char* who, int device, hipStream_t stream, const float* weights, size_t n_floats) {
  VP_REQUIRE(n_floats == n, "%s: expected %zu floats, got %zu", who, n, n_floats);
  VP_HIP(hipSetDevice(device));
  VP_HIP(hipStreamSynchronize(stream));
  VP_HIP(hipMemcpy(w.p, weights, n_floats * sizeof(float), hipMemcpyHostToDevice));
  return VP_OK;
}

int check_hyper(const char* who, float beta1, float beta2, float adam_eps) {
  VP_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: beta1 %g, beta2 %g outside [0, 1) (1 - beta^t divides the step)",
             who, (double)beta1, (double)beta2);
  VP_REQUIRE(adam_eps > 0.f && std::isfinite(adam_eps), "%s: adam_eps %g is not finite and positive", who, (double)adam_eps);
  return VP_OK;
}

}  // namespace vp
