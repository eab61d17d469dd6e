// The counter-based generator behind everything random the device draws: the noise of augmented batches (batchgen.hip) and
// the dropout masks of the pick-branch training step (train_eqt_pick.hip).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vp {

// Philox4x32-10 (Salmon et al., SC'11): ctr <- the bijection of ctr under key.
__device__ __forceinline__ void philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, ctr[0]), l0 = 0xD2511F53u * ctr[0];
    const uint32_t h1 = __umulhi(0xCD9E8D57u, ctr[2]), l1 = 0xCD9E8D57u * ctr[2];
    const uint32_t c1 = ctr[1], c3 = ctr[3];
    ctr[0] = h1 ^ c1 ^ k0;
    ctr[1] = l1;
    ctr[2] = h0 ^ c3 ^ k1;
    ctr[3] = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The dropout mask of the pick branches.  Element (branch k, window b of the batch, channel c, time step t) of training
// step n (the trainer's count of steps so far, update or not) under `seed`:
//
//   ctr = {b, (k * 16 + c) * 47 + t, low word of n, high word of n},  key = (low word of seed, high word of seed)
//   w   = philox4x32_10(ctr, key);  ONE output word is used, w[0]
//   r   = (float)(w[0] >> 8) * 2^-24        (exact: 24 bits, r in [0, 1))
//   keep  <=>  r >= drop_rate               (a comparison of floats; drop_rate = 0 keeps every element)
//
// A kept element is multiplied by 1 / (1 - drop_rate), formed ONCE on the host in float (1.f / (1.f - drop_rate)) and passed
// to the kernels; a dropped one becomes +0.  The forward pass keeps the 0 / 1 mask; the backward pass reads it and multiplies
// by the same scale.
__device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t step, int b, int element, float drop_rate) {
  uint32_t w[4] = {(uint32_t)b, (uint32_t)element, (uint32_t)step, (uint32_t)(step >> 32)};
  philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(w[0] >> 8) * 0x1p-24f >= drop_rate;
}

}  // namespace vp
