// EQTransformer bottleneck, one launch per layer (the six-launch plan, plan_flags[2] = 1): scalar FMA chains on the vector ALUs,
// the independent reference of the one-launch kernel (eqt_mid4.hip); see eqt_kernels.h.
// The device helpers live in eqt_mid_parts.h (shared with eqt_mid4.hip); here a window's team is the whole workgroup.
#define MID_TID threadIdx.x
#define MID_NT blockDim.x
#define MID_TEAM 0
#include "eqt_mid_parts.h"

namespace vp {

// ---------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(128) void bilstm_kernel(const BiLstmArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[T * CIN];
  __shared__ float gx[2][T * 64];
  __shared__ float hc[32][48];
  const int tid = MID_TID, b = blockIdx.x;
  const float* src = a.src + (long)b * a.ws_src;
  for (int idx = tid; idx < CIN * T; idx += 128) {
    const int c = idx / T, t = idx - c * T;
    xs[t * CIN + c] = src[(long)c * a.ls_src + HALO + t];
  }
  __syncthreads();
  const int wave = tid >> 6;
  lstm_direction<CIN>(xs, gx[wave], wave == 0 ? a.fwd : a.bwd, wave == 1, &hc[wave * 16][0], 48);
  __syncthreads();
  float* dst = a.dst + (long)b * a.ws_dst;
  for (int idx = tid; idx < EQT_H * T; idx += 128) {  // Conv1d(32,16,1) + BatchNorm, folded
    const int co = idx / T, t = idx - co * T;
    float acc = a.bc[co];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc = fmaf(a.wc[co * 32 + c], hc[c][t], acc);
    dst[(long)co * a.ls_dst + HALO + t] = acc;
  }
}

int launch_bilstm(const BiLstmArgs& a, int cin, int B, hipStream_t s) {
  if (cin == 64) {
    hipLaunchKernelGGL(bilstm_kernel<64>, dim3(B), dim3(128), 0, s, a);
  } else if (cin == 16) {
    hipLaunchKernelGGL(bilstm_kernel<16>, dim3(B), dim3(128), 0, s, a);
  } else {
    set_error("bilstm: unsupported input size %d", cin);
    return VP_ERR_UNSUPPORTED;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
constexpr int TR_NTH = 512;  // threads per window (1024 ran the kernel itself 3 us faster and the pipeline 1 % slower: a round-1 workgroup-size sweep, LOG.md)
__global__ __launch_bounds__(TR_NTH) void transformer_kernel(const TransformerArgs a) {
  constexpr int NTH = TR_NTH;
  __shared__ float xs[T][EQT_H];
  // q / k / e of the attention and, afterwards, the padded feed-forward weights share one pool
  constexpr int POOL = 2 * T * KP + T * 48;
  constexpr int W1S = 17, W2S = 129;  // row strides that spread the rows over the LDS banks
  static_assert(128 * W1S + EQT_H * W2S <= POOL, "feed-forward weights must fit the attention scratch");
  __shared__ float pool[POOL];
  float(*q)[KP] = reinterpret_cast<float(*)[KP]>(pool);
  float(*k)[KP] = reinterpret_cast<float(*)[KP]>(pool + T * KP);
  float(*e)[48] = reinterpret_cast<float(*)[48]>(pool + 2 * T * KP);
  float* w1s = pool;
  float* w2s = pool + 128 * W1S;
  __shared__ float v[T][EQT_H];
  __shared__ float y1[T][EQT_H];
  __shared__ float h1[T][128];
  const int tid = MID_TID, b = blockIdx.x;
  load_window_transposed(a.src + (long)b * a.ws_src, a.ls_src, xs);
  __syncthreads();
  attention_core(xs, q, k, e, v, a.att, a.attn_eps, 0);  // ends with a barrier: q / k / e are dead now
  for (int i = tid; i < 128 * 16; i += NTH) {  // coalesced global reads, padded LDS rows
    w1s[(i >> 4) * W1S + (i & 15)] = a.w1[i];
    w2s[(i >> 7) * W2S + (i & 127)] = a.w2[i];
  }
  if (tid < T) {  // y1 = LN1(x + attention(x))
    float z[EQT_H];
#pragma unroll
    for (int c = 0; c < EQT_H; ++c) z[c] = xs[tid][c] + v[tid][c];
    layer_norm16(z, a.g1, a.b1, a.ln_eps, y1[tid]);
  }
  __syncthreads();
  for (int idx = tid; idx < T * 128; idx += NTH) {  // FF: Linear(16,128) + ReLU
    const int t = idx >> 7, m = idx & 127;
    float acc = a.bb1[m];
#pragma unroll
    for (int c = 0; c < EQT_H; ++c) acc = fmaf(w1s[m * W1S + c], y1[t][c], acc);
    h1[t][m] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  for (int idx = tid; idx < T * EQT_H; idx += NTH) {  // Linear(128,16) + residual
    const int t = idx >> 4, c = idx & 15;
    float a0 = a.bb2[c], a1 = 0.f;
#pragma unroll 8
    for (int m = 0; m < 128; m += 2) {
      a0 = fmaf(w2s[c * W2S + m], h1[t][m], a0);
      a1 = fmaf(w2s[c * W2S + m + 1], h1[t][m + 1], a1);
    }
    v[t][c] = y1[t][c] + (a0 + a1);
  }
  __syncthreads();
  if (tid < T) layer_norm16(v[tid], a.g2, a.b2, a.ln_eps, xs[tid]);
  __syncthreads();
  float* dst = a.dst + (long)b * a.ws_dst;
  float* up = a.up ? a.up + (long)b * a.ws_up : nullptr;
  for (int idx = tid; idx < EQT_H * T; idx += NTH) {
    const int c = idx / T, t = idx - c * T;
    const float val = xs[t][c];
    dst[(long)c * a.ls_dst + HALO + t] = val;
    if (up) up[(long)c * a.ls_up + HALO + t] = val;
  }
}

int launch_transformer(const TransformerArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(transformer_kernel, dim3(B), dim3(TR_NTH), 0, s, a);
  return 0;
}

// ---------------------------------------------------------------------------------------
// P / S branch: LSTM(16,16) -> banded additive attention -> x2-upsampled decoder input.
constexpr int PICK_NTH = 256;  // threads per (window, branch): 1024 held every wave slot of the chip through the 47 sequential LSTM steps of ONE wave
__global__ __launch_bounds__(PICK_NTH) void pick_branch_kernel(const PickBranchArgs a) {
  constexpr int NTH = PICK_NTH;
  __shared__ __attribute__((aligned(16))) float xs[T][EQT_H];
  __shared__ float gx[T * 64];
  __shared__ float hl[EQT_H][48];
  __shared__ float x2[T][EQT_H];
  __shared__ __attribute__((aligned(8))) float q[T][KP], k[T][KP];
  __shared__ float e[T][48];
  __shared__ float v[T][EQT_H];
  const int tid = MID_TID, b = blockIdx.x, br = blockIdx.y;
  load_window_transposed(a.src + (long)b * a.ws_src, a.ls_src, xs);
  __syncthreads();
  if (tid < 64) lstm_direction<EQT_H>(&xs[0][0], gx, a.lstm[br], false, &hl[0][0], 48);
  __syncthreads();
  for (int idx = tid; idx < T * EQT_H; idx += NTH) {
    const int t = idx >> 4, c = idx & 15;
    x2[t][c] = hl[c][t];
  }
  __syncthreads();
  attention_core(x2, q, k, e, v, a.att[br], a.attn_eps, a.width);
  float* up = a.up + (long)((1 + br) * a.B + b) * a.ws_up;
  for (int idx = tid; idx < EQT_H * T; idx += NTH) {
    const int c = idx / T, t = idx - c * T;
    const float val = v[t][c];
    up[(long)c * a.ls_up + HALO + t] = val;
  }
}

int launch_pick_branch(const PickBranchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(pick_branch_kernel, dim3(a.B, 2), dim3(PICK_NTH), 0, s, a);
  return 0;
}

}  // namespace vp
