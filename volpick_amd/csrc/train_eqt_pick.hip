// EQTransformer: training forward and backward of the two pick branches (pick_lstms.{0,1} -> dropout -> pick_attentions.{0,1})
// in fp32, for the decoder trainer's scope VP_EQT_TRAIN_PICK_BRANCHES (train_eqt_dec.hip holds the state and orders the launches).
//
//   lstm forward     pre_t = (b_ih + b_hh) + W_ih x_t + W_hh h_{t-1}; i, f, o = sigmoid, g = tanh; c_t = f c_{t-1} + i g;
//                    h_t = o tanh(c_t)                                         pick_lstm_fwd_kernel   (one wave per recurrence)
//   attention fwd    hd = h mask / (1 - p); q = hd Wt, k = hd Wx; e_ij = Wa . tanh(q_i + k_j + bh) + ba; m_i = max_j e_ij over
//                    the FULL row (lowest index among equals kept); p_ij = exp(e_ij - m_i) in the band; a = p / (sum + 1e-5);
//                    v_i = sum_j a_ij hd_j -> decoder.in of the P / S decoder   pick_attn_fwd_kernel
//   attention bwd    from gv: ga_ij = gv_i . hd_j, ge_ij = a_ij (ga_ij - sum_j' a_ij' ga_ij'), the row maximum's share
//                    gm_i = -sum_j ge_ij added at the kept argmax; the tanh terms of at most four columns per row recomputed;
//                    gq, gk, ghd, gh = ghd mask / (1 - p), and the window's Wa sums  pick_attn_bwd_kernel
//   lstm bwd         dh_t = gh_t + W_hh^T gpre_{t+1}; dc_t = gc_t + dh_t o (1 - tanh^2 c_t); gpre_t; gc_{t-1} = dc_t f
//                                                                              pick_lstm_bwd_kernel   (one wave per recurrence)
//   d weight         per (branch, window): sum_t gpre_t x_t^T, sum_t gpre_t h_{t-1}^T, sum_t gpre_t (both biases), hd^T gk (Wx),
//                    hd^T gq (Wt), sum_i gq_i (bh), the Wa sums, +0 for ba      pick_wgrad_kernel + pick_fold_kernel
//
// The gradient of ba is zero (a constant of a row cancels in e - max e): +0.0 is written.  Gradients into x are not formed.
// One workgroup per (branch, window); nothing tiles the batch.  No atomics: every sum has one owner and a fixed order, and the
// per-window partial blocks are folded over the windows in index order, as dec_fold_kernel does.
//
// Transcendentals are the library's expf / tanhf and true divisions: the arithmetic here is ~1 MFLOP per (branch, window), the
// recurrences are bound by the latency of 47 dependent steps, and the gradients are compared with float64 at fp32 bars.
#include "train_eqt_pick.h"

#include "philox.h"

namespace vp {
namespace {

using D = PickDims;
constexpr int T = D::T, H = D::H, G = D::G, U = D::U, CIN = D::CIN;
constexpr int TS = T + 2;      // LDS stride of a [rows][47] block: odd, so that rows spread over the banks
constexpr int GS = G + 1;      // LDS stride of a [47][64] block
constexpr int HS = H + 1;      // LDS stride of a [47][16] block
constexpr int US = U + 1;      // LDS stride of a [47][32] block
constexpr int NSLOT = D::BAND + 1;  // score terms a row's backward needs: the band and the argmax
constexpr int ATT_THREADS = 256, ATT_GROUPS = ATT_THREADS / U;
static_assert(G == 64, "a wave's 64 lanes are the 64 gate rows");
static_assert(H == CIN && D::BAND == 3, "the kernels below assume nn.LSTM(16, 16) and a band of 3");

struct PickArgs {
  const float* w;  // the trainer's weight blob
  int off[D::NBR][PK_NSEG];
  const float* x;  // [B][16][47]
  float *pre, *act, *c, *h, *mask, *hd, *v, *q, *k, *e, *a, *argmax, *din;
  float *gv, *ghd, *gh, *gc, *gpre, *gq, *gk, *gwa, *partial;
  int B;
  float drop_rate, scale;
  uint64_t seed, step;
};

__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float lane_value(float v, int lane) { return __shfl(v, lane, 64); }

// rows x 47 of one window: global [rows][47] <-> LDS [rows][stride]
template <int NT>
__device__ __forceinline__ void load_rows(const float* __restrict__ src, float* dst, int rows, int stride, int tid) {
  for (int idx = tid; idx < rows * T; idx += NT) {
    const int r = idx / T, t = idx - r * T;
    dst[r * stride + t] = src[idx];
  }
}

// ---- LSTM forward: block = one wave = one (window, branch); lane = gate row (gate = lane >> 4, unit = lane & 15) -------------
__global__ __launch_bounds__(64) void pick_lstm_fwd_kernel(const PickArgs a) {
  __shared__ float xs[T * HS];    // [t][c]
  __shared__ float pres[T * GS];  // [t][row]: the input projection, then the pre-activation
  __shared__ float acts[T * GS];
  __shared__ float cs[T * HS], hs[T * HS];
  const int lane = threadIdx.x, b = blockIdx.x, br = blockIdx.y, unit = lane & (H - 1), gate = lane >> 4;
  const long win = (long)br * a.B + b;
  {
    const float* x = a.x + (long)b * CIN * T;
    for (int idx = lane; idx < CIN * T; idx += 64) {
      const int c = idx / T, t = idx - c * T;
      xs[t * HS + c] = x[idx];
    }
  }
  float wih[CIN], whh[H];
  {
    const float* wi = a.w + a.off[br][PK_W_IH] + lane * CIN;
    const float* wh = a.w + a.off[br][PK_W_HH] + lane * H;
#pragma unroll
    for (int j = 0; j < CIN; ++j) wih[j] = wi[j], whh[j] = wh[j];
  }
  const float bias = a.w[a.off[br][PK_B_IH] + lane] + a.w[a.off[br][PK_B_HH] + lane];
  __syncthreads();
  for (int t = 0; t < T; ++t) {  // the input projection of every step: off the serial path
    float p0 = bias, p1 = 0.f;
#pragma unroll
    for (int j = 0; j < CIN; j += 2) p0 = fmaf(wih[j], xs[t * HS + j], p0), p1 = fmaf(wih[j + 1], xs[t * HS + j + 1], p1);
    pres[t * GS + lane] = p0 + p1;
  }
  float h = 0.f, c = 0.f;  // of this lane's unit: the four lanes of a unit hold the same values
  for (int t = 0; t < T; ++t) {
    float p0 = pres[t * GS + lane], p1 = 0.f;  // (written by this lane)
#pragma unroll
    for (int j = 0; j < H; j += 2) p0 = fmaf(whh[j], lane_value(h, j), p0), p1 = fmaf(whh[j + 1], lane_value(h, j + 1), p1);
    const float pre = p0 + p1;
    const float act = gate == 2 ? tanhf(pre) : sigmoidf_(pre);
    const float ig = lane_value(act, unit), fg = lane_value(act, H + unit), gg = lane_value(act, 2 * H + unit),
                og = lane_value(act, 3 * H + unit);
    c = fmaf(fg, c, ig * gg);
    h = og * tanhf(c);
    pres[t * GS + lane] = pre;
    acts[t * GS + lane] = act;
    if (gate == 0) cs[t * HS + unit] = c, hs[t * HS + unit] = h;
  }
  __syncthreads();
  for (int idx = lane; idx < G * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    a.pre[win * G * T + idx] = pres[t * GS + r];
    a.act[win * G * T + idx] = acts[t * GS + r];
  }
  for (int idx = lane; idx < H * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    a.c[win * H * T + idx] = cs[t * HS + r];
    a.h[win * H * T + idx] = hs[t * HS + r];
  }
}

// ---- dropout + attention forward: block = 256 threads = one (window, branch) -------------------------------------------------
__global__ __launch_bounds__(ATT_THREADS) void pick_attn_fwd_kernel(const PickArgs a) {
  __shared__ float hd[H * TS];               // [c][t]
  __shared__ float qs[T * US], ks[T * US];   // [t][u]
  __shared__ float es[T * TS];               // [i][j]
  __shared__ float ab[T * D::BAND];          // a in the band: [i][j - i + 1]
  __shared__ float wt[H * U], wx[H * U], bh[U], wa[U];
  const int tid = threadIdx.x, b = blockIdx.x, br = blockIdx.y;
  const long win = (long)br * a.B + b;
  for (int idx = tid; idx < H * U; idx += ATT_THREADS) wt[idx] = a.w[a.off[br][PK_WT] + idx], wx[idx] = a.w[a.off[br][PK_WX] + idx];
  if (tid < U) bh[tid] = a.w[a.off[br][PK_BH] + tid], wa[tid] = a.w[a.off[br][PK_WA] + tid];
  const float ba = a.w[a.off[br][PK_BA]];
  for (int idx = tid; idx < H * T; idx += ATT_THREADS) {
    const int c = idx / T, t = idx - c * T;
    const bool keep = dropout_keep(a.seed, a.step, b, br * H * T + idx, a.drop_rate);
    const float v = keep ? a.h[win * H * T + idx] * a.scale : 0.f;
    hd[c * TS + t] = v;
    a.mask[win * H * T + idx] = keep ? 1.f : 0.f;
    a.hd[win * H * T + idx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < 2 * U * T; idx += ATT_THREADS) {  // q = hd Wt, k = hd Wx: chains of 16 products
    const int which = idx / (U * T), rem = idx - which * (U * T), u = rem / T, t = rem - u * T;
    const float* wm = which ? wx : wt;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < H; ++c) s = fmaf(hd[c * TS + t], wm[c * U + u], s);
    (which ? ks : qs)[t * US + u] = s;
    (which ? a.k : a.q)[win * U * T + rem] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < T * T; idx += ATT_THREADS) {
    const int i = idx / T, j = idx - i * T;
    float s = 0.f;
#pragma unroll 8
    for (int u = 0; u < U; ++u) s = fmaf(wa[u], tanhf((qs[i * US + u] + ks[j * US + u]) + bh[u]), s);
    s += ba;
    es[i * TS + j] = s;
    a.e[win * T * T + idx] = s;
  }
  __syncthreads();
  if (tid < T) {  // row i: the maximum over the full row and its first index, then the band
    const int i = tid;
    float m = es[i * TS];
    int arg = 0;
    for (int j = 1; j < T; ++j) {
      const float v = es[i * TS + j];
      if (v > m) m = v, arg = j;
    }
    float p[D::BAND], sum = 0.f;
#pragma unroll
    for (int s = 0; s < D::BAND; ++s) {
      const int j = i - 1 + s;
      p[s] = (j >= 0 && j < T) ? expf(es[i * TS + j] - m) : 0.f;
      sum += p[s];
    }
    const float den = sum + D::ATT_EPS;
#pragma unroll
    for (int s = 0; s < D::BAND; ++s) ab[i * D::BAND + s] = p[s] / den;
    a.argmax[win * T + i] = (float)arg;
  }
  __syncthreads();
  for (int idx = tid; idx < T * T; idx += ATT_THREADS) {
    const int i = idx / T, j = idx - i * T, s = j - i + 1;
    a.a[win * T * T + idx] = (s >= 0 && s < D::BAND) ? ab[i * D::BAND + s] : 0.f;
  }
  float* din = a.din + ((long)(1 + br) * a.B + b) * H * T;
  for (int idx = tid; idx < H * T; idx += ATT_THREADS) {
    const int c = idx / T, i = idx - c * T;
    float s = 0.f;
#pragma unroll
    for (int sl = 0; sl < D::BAND; ++sl) {
      const int j = i - 1 + sl;
      if (j >= 0 && j < T) s = fmaf(ab[i * D::BAND + sl], hd[c * TS + j], s);
    }
    a.v[win * H * T + idx] = s;
    din[idx] = s;
  }
}

// ---- attention and dropout backward: block = 256 threads = one (window, branch) ----------------------------------------------
__global__ __launch_bounds__(ATT_THREADS) void pick_attn_bwd_kernel(const PickArgs a) {
  __shared__ float hd[H * TS], gvs[H * TS];  // [c][t]
  __shared__ float qs[T * US], ks[T * US];   // [t][u]: q and k, then (behind a barrier) gq and gk
  __shared__ float ab[T * D::BAND];
  __shared__ float gs[T * NSLOT];            // the score gradient of row i's slots: the band's columns, then the argmax
  __shared__ int col[T * NSLOT];             // their columns; -1: none (outside the row, or the argmax lies in the band)
  __shared__ float ds[T * NSLOT * U];        // gradient of the tanh argument of (i, slot, u)
  __shared__ float pwa[ATT_GROUPS * U];
  __shared__ float wt[H * U], wx[H * U], bh[U], wa[U];
  const int tid = threadIdx.x, b = blockIdx.x, br = blockIdx.y;
  const long win = (long)br * a.B + b;
  for (int idx = tid; idx < H * U; idx += ATT_THREADS) wt[idx] = a.w[a.off[br][PK_WT] + idx], wx[idx] = a.w[a.off[br][PK_WX] + idx];
  if (tid < U) bh[tid] = a.w[a.off[br][PK_BH] + tid], wa[tid] = a.w[a.off[br][PK_WA] + tid];
  load_rows<ATT_THREADS>(a.hd + win * H * T, hd, H, TS, tid);
  load_rows<ATT_THREADS>(a.gv + win * H * T, gvs, H, TS, tid);
  for (int idx = tid; idx < U * T; idx += ATT_THREADS) {
    const int u = idx / T, t = idx - u * T;
    qs[t * US + u] = a.q[win * U * T + idx];
    ks[t * US + u] = a.k[win * U * T + idx];
  }
  for (int idx = tid; idx < T * D::BAND; idx += ATT_THREADS) {
    const int i = idx / D::BAND, j = i - 1 + (idx - i * D::BAND);
    ab[idx] = (j >= 0 && j < T) ? a.a[win * T * T + i * T + j] : 0.f;
  }
  __syncthreads();
  if (tid < T) {
    const int i = tid;
    float ga[D::BAND], dot = 0.f;
#pragma unroll
    for (int s = 0; s < D::BAND; ++s) {
      const int j = i - 1 + s;
      float g = 0.f;
      if (j >= 0 && j < T) {
#pragma unroll
        for (int c = 0; c < H; ++c) g = fmaf(gvs[c * TS + i], hd[c * TS + j], g);
      }
      ga[s] = g;
      dot = fmaf(ab[i * D::BAND + s], g, dot);
    }
    float ge[D::BAND], gm = 0.f;
#pragma unroll
    for (int s = 0; s < D::BAND; ++s) {
      ge[s] = ab[i * D::BAND + s] * (ga[s] - dot);
      gm -= ge[s];
    }
    const int js = (int)a.argmax[win * T + i], ss = js - i + 1;
    const bool in_band = ss >= 0 && ss < D::BAND;
#pragma unroll
    for (int s = 0; s < D::BAND; ++s) {
      const int j = i - 1 + s;
      gs[i * NSLOT + s] = (in_band && s == ss) ? ge[s] + gm : ge[s];
      col[i * NSLOT + s] = (j >= 0 && j < T) ? j : -1;
    }
    gs[i * NSLOT + D::BAND] = in_band ? 0.f : gm;
    col[i * NSLOT + D::BAND] = (in_band || js < 0 || js >= T) ? -1 : js;
  }
  __syncthreads();
  {  // thread (group, u): rows group, group + 8, ...; the tanh terms recomputed
    const int grp = tid / U, u = tid - grp * U;
    float sum_wa = 0.f;
    for (int i = grp; i < T; i += ATT_GROUPS) {
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const int j = col[i * NSLOT + s];
        float d = 0.f;
        if (j >= 0) {
          const float g = gs[i * NSLOT + s];
          const float th = tanhf((qs[i * US + u] + ks[j * US + u]) + bh[u]);
          sum_wa = fmaf(g, th, sum_wa);
          d = (g * wa[u]) * fmaf(-th, th, 1.f);
        }
        ds[(i * NSLOT + s) * U + u] = d;
      }
    }
    pwa[grp * U + u] = sum_wa;
  }
  __syncthreads();  // q and k have been read: their arrays now take gq and gk (the loop below reads ds and col alone)
  for (int idx = tid; idx < 2 * U * T; idx += ATT_THREADS) {
    const int which = idx / (U * T), rem = idx - which * (U * T), u = rem / T, t = rem - u * T;
    float s;
    if (which == 0) {  // gq_i: the row's slots in order
      const float* d = ds + t * NSLOT * U + u;
      s = ((d[0] + d[U]) + d[2 * U]) + d[3 * U];
    } else {  // gk_j: the band's rows i = j - 1, j, j + 1 (slot j - i + 1), then the rows whose argmax is j, in order
      s = 0.f;
#pragma unroll
      for (int di = -1; di <= 1; ++di) {
        const int i = t + di;
        if (i >= 0 && i < T) s += ds[(i * NSLOT + (1 - di)) * U + u];
      }
      for (int i = 0; i < T; ++i)
        if (col[i * NSLOT + D::BAND] == t) s += ds[(i * NSLOT + D::BAND) * U + u];
    }
    (which ? ks : qs)[t * US + u] = s;
    (which ? a.gk : a.gq)[win * U * T + rem] = s;
  }
  if (tid < U) {
    float s = pwa[tid];
    for (int g = 1; g < ATT_GROUPS; ++g) s += pwa[g * U + tid];
    a.gwa[win * U + tid] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < H * T; idx += ATT_THREADS) {
    const int c = idx / T, i = idx - c * T;
    float s = 0.f;
#pragma unroll
    for (int di = -1; di <= 1; ++di) {  // v_i' = sum_j a_i'j hd_j reads hd_i in the rows i' = i - 1, i, i + 1
      const int ip = i + di;
      if (ip >= 0 && ip < T) s = fmaf(ab[ip * D::BAND + (1 - di)], gvs[c * TS + ip], s);
    }
#pragma unroll 8
    for (int u = 0; u < U; ++u) s = fmaf(wt[c * U + u], qs[i * US + u], s);
#pragma unroll 8
    for (int u = 0; u < U; ++u) s = fmaf(wx[c * U + u], ks[i * US + u], s);
    a.ghd[win * H * T + idx] = s;
    a.gh[win * H * T + idx] = a.mask[win * H * T + idx] != 0.f ? s * a.scale : 0.f;
  }
}

// ---- LSTM backward through time: block = one wave = one (window, branch); lane = gate row ------------------------------------
__global__ __launch_bounds__(64) void pick_lstm_bwd_kernel(const PickArgs a) {
  __shared__ float acts[T * GS];  // [t][row]
  __shared__ float gps[T * GS];   // gpre [t][row]
  __shared__ float cs[T * HS], ghs[T * HS], gcs[T * HS];
  const int lane = threadIdx.x, b = blockIdx.x, br = blockIdx.y, unit = lane & (H - 1), gate = lane >> 4;
  const long win = (long)br * a.B + b;
  for (int idx = lane; idx < G * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    acts[t * GS + r] = a.act[win * G * T + idx];
  }
  for (int idx = lane; idx < H * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    cs[t * HS + r] = a.c[win * H * T + idx];
    ghs[t * HS + r] = a.gh[win * H * T + idx];
  }
  float wcol[H];  // W_hh[gate * 16 + u'][unit], u' = 0 .. 15: this lane's quarter of column `unit` of W_hh
  {
    const float* wh = a.w + a.off[br][PK_W_HH];
#pragma unroll
    for (int j = 0; j < H; ++j) wcol[j] = wh[(gate * H + j) * H + unit];
  }
  __syncthreads();
  float gc = 0.f;  // the cell gradient entering step t (the same in the four lanes of a unit)
  for (int t = T - 1; t >= 0; --t) {
    float part = 0.f;
    if (t + 1 < T) {
      const float* gp = gps + (t + 1) * GS + gate * H;
#pragma unroll
      for (int j = 0; j < H; ++j) part = fmaf(wcol[j], gp[j], part);
    }
    const float p0 = lane_value(part, unit), p1 = lane_value(part, H + unit), p2 = lane_value(part, 2 * H + unit),
                p3 = lane_value(part, 3 * H + unit);
    const float dh = ghs[t * HS + unit] + ((p0 + p1) + (p2 + p3));
    const float ig = acts[t * GS + unit], fg = acts[t * GS + H + unit], gg = acts[t * GS + 2 * H + unit],
                og = acts[t * GS + 3 * H + unit];
    const float cprev = t > 0 ? cs[(t - 1) * HS + unit] : 0.f;
    const float tc = tanhf(cs[t * HS + unit]);
    const float dc = fmaf(dh * og, fmaf(-tc, tc, 1.f), gc);
    float gp;
    if (gate == 0)
      gp = (dc * gg) * (ig * (1.f - ig));
    else if (gate == 1)
      gp = (dc * cprev) * (fg * (1.f - fg));
    else if (gate == 2)
      gp = (dc * ig) * fmaf(-gg, gg, 1.f);
    else
      gp = (dh * tc) * (og * (1.f - og));
    if (gate == 0) gcs[t * HS + unit] = gc;
    gps[t * GS + lane] = gp;
    gc = dc * fg;
    __syncthreads();  // (one wave: orders the LDS write above before the next step's reads)
  }
  for (int idx = lane; idx < G * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    a.gpre[win * G * T + idx] = gps[t * GS + r];
  }
  for (int idx = lane; idx < H * T; idx += 64) {
    const int r = idx / T, t = idx - r * T;
    a.gc[win * H * T + idx] = gcs[t * HS + r];
  }
}

// ---- weight gradients of one (window, branch): its block of PICK_PSZ sums, each a chain over the time steps in order ---------
__global__ __launch_bounds__(ATT_THREADS) void pick_wgrad_kernel(const PickArgs a) {
  __shared__ float gp[G * TS], xs[CIN * TS], hs[H * TS], hd[H * TS], gq[U * TS], gk[U * TS];  // [row][t]
  const int tid = threadIdx.x, b = blockIdx.x, br = blockIdx.y;
  const long win = (long)br * a.B + b;
  load_rows<ATT_THREADS>(a.gpre + win * G * T, gp, G, TS, tid);
  load_rows<ATT_THREADS>(a.x + (long)b * CIN * T, xs, CIN, TS, tid);
  load_rows<ATT_THREADS>(a.h + win * H * T, hs, H, TS, tid);
  load_rows<ATT_THREADS>(a.hd + win * H * T, hd, H, TS, tid);
  load_rows<ATT_THREADS>(a.gq + win * U * T, gq, U, TS, tid);
  load_rows<ATT_THREADS>(a.gk + win * U * T, gk, U, TS, tid);
  __syncthreads();
  constexpr int S_WHH = pick_seg_start(PK_W_HH), S_BIH = pick_seg_start(PK_B_IH), S_WX = pick_seg_start(PK_WX),
                S_WT = pick_seg_start(PK_WT), S_BH = pick_seg_start(PK_BH), S_WA = pick_seg_start(PK_WA), S_BA = pick_seg_start(PK_BA);
  float* out = a.partial + win * PICK_PSZ;
  for (int idx = tid; idx < PICK_PSZ; idx += ATT_THREADS) {
    float s = 0.f;
    if (idx < S_BIH) {  // W_ih[row][c], W_hh[row][u]
      const bool hh = idx >= S_WHH;
      const int rem = idx - (hh ? S_WHH : 0), row = rem / H, j = rem - row * H;
      const float* other = hh ? hs + j * TS - 1 : xs + j * TS;  // h_{t-1} (t >= 1) or x_t
      for (int t = hh ? 1 : 0; t < T; ++t) s = fmaf(gp[row * TS + t], other[t], s);
    } else if (idx < S_WX) {  // b_ih[row], b_hh[row]: the same sum
      const int row = (idx - S_BIH) % G;
      for (int t = 0; t < T; ++t) s += gp[row * TS + t];
    } else if (idx < S_BH) {  // Wx[c][u] = sum_j hd[c][j] gk[j][u], Wt[c][u] = sum_i hd[c][i] gq[i][u]
      const bool is_t = idx >= S_WT;
      const int rem = idx - (is_t ? S_WT : S_WX), c = rem / U, u = rem - c * U;
      const float* g = (is_t ? gq : gk) + u * TS;
      for (int t = 0; t < T; ++t) s = fmaf(hd[c * TS + t], g[t], s);
    } else if (idx < S_WA) {  // bh[u] = sum_i gq[i][u]
      const int u = idx - S_BH;
      for (int t = 0; t < T; ++t) s += gq[u * TS + t];
    } else if (idx < S_BA) {
      s = a.gwa[win * U + (idx - S_WA)];
    }  // ba: +0
    out[idx] = s;
  }
}

// where element idx of a branch's block goes in the gradient blob
template <int S = 0>
__device__ __forceinline__ int pick_dest(const PickArgs& a, int br, int idx) {
  if constexpr (S + 1 < PK_NSEG) {
    constexpr int NEXT = pick_seg_start(S + 1);
    if (idx >= NEXT) return pick_dest<S + 1>(a, br, idx);
  }
  constexpr int START = pick_seg_start(S);
  return a.off[br][S] + (idx - START);
}

// grad[tensor][i] = partial[branch][0][...] + partial[branch][1][...] + ... in the windows' order
__global__ __launch_bounds__(256) void pick_fold_kernel(const PickArgs a, float* __restrict__ grad) {
  const int idx = blockIdx.x * 256 + threadIdx.x, br = blockIdx.y;
  if (idx >= PICK_PSZ) return;
  const float* p = a.partial + (long)br * a.B * PICK_PSZ + idx;
  float s = p[0];
  for (int b = 1; b < a.B; ++b) s += p[(long)b * PICK_PSZ];
  grad[pick_dest(a, br, idx)] = s;
}

PickArgs pick_args(const PickState& ps, const float* w, const float* x, float* din, int B) {
  PickArgs a{};
  a.w = w, a.x = x, a.din = din, a.B = B;
  for (int br = 0; br < D::NBR; ++br)
    for (int s = 0; s < PK_NSEG; ++s) a.off[br][s] = ps.off[br][s];
  a.pre = ps.pre.p, a.act = ps.act.p, a.c = ps.c.p, a.h = ps.h.p, a.mask = ps.mask.p, a.hd = ps.hd.p, a.v = ps.v.p, a.q = ps.q.p;
  a.k = ps.k.p, a.e = ps.e.p, a.a = ps.a.p, a.argmax = ps.argmax.p;
  a.gv = ps.gv.p, a.ghd = ps.ghd.p, a.gh = ps.gh.p, a.gc = ps.gc.p, a.gpre = ps.gpre.p, a.gq = ps.gq.p, a.gk = ps.gk.p, a.gwa = ps.gwa.p;
  a.partial = ps.partial.p;
  a.drop_rate = ps.drop_rate, a.scale = ps.scale, a.seed = ps.seed, a.step = ps.step;
  return a;
}

}  // namespace

int PickState::alloc(int mb, const AddTensor& add) {
  max_batch = mb;
  auto rows = [&](DevArray<float>& buf, const char* name, int C, int L) -> int {
    VP_HIP(buf.alloc((size_t)D::NBR * mb * C * L, true));
    add(name, buf.p, D::NBR, C, L);
    return VP_OK;
  };
  int r;
#define PICK_ROWS(buf, name, C, L) \
  if ((r = rows(buf, name, C, L)) != VP_OK) return r
  PICK_ROWS(pre, "pick.pre", G, T);
  PICK_ROWS(act, "pick.act", G, T);
  PICK_ROWS(c, "pick.c", H, T);
  PICK_ROWS(h, "pick.h", H, T);
  PICK_ROWS(mask, "pick.mask", H, T);
  PICK_ROWS(hd, "pick.hd", H, T);
  PICK_ROWS(q, "pick.q", U, T);
  PICK_ROWS(k, "pick.k", U, T);
  PICK_ROWS(e, "pick.e", T, T);
  PICK_ROWS(a, "pick.a", T, T);
  PICK_ROWS(argmax, "pick.argmax", 1, T);
  PICK_ROWS(v, "pick.v", H, T);
  PICK_ROWS(gv, "pick.gv", H, T);
  PICK_ROWS(gq, "pick.gq", U, T);
  PICK_ROWS(gk, "pick.gk", U, T);
  PICK_ROWS(ghd, "pick.ghd", H, T);
  PICK_ROWS(gh, "pick.gh", H, T);
  PICK_ROWS(gc, "pick.gc", H, T);
  PICK_ROWS(gpre, "pick.gpre", G, T);
#undef PICK_ROWS
  VP_HIP(gwa.alloc((size_t)D::NBR * mb * U, true));
  VP_HIP(partial.alloc((size_t)D::NBR * mb * PICK_PSZ, true));
  return VP_OK;
}

void PickState::release_events() {
  for (hipEvent_t& e : ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

void pick_forward(PickState& ps, const float* w, const float* x, float* din, int B, hipStream_t s, int& launches) {
  const PickArgs a = pick_args(ps, w, x, din, B);
  const dim3 grid(B, D::NBR);
  hipLaunchKernelGGL(pick_lstm_fwd_kernel, grid, dim3(64), 0, s, a);
  hipLaunchKernelGGL(pick_attn_fwd_kernel, grid, dim3(ATT_THREADS), 0, s, a);
  launches += 2;
}

void pick_backward(PickState& ps, const float* w, int B, hipStream_t s, int& launches) {
  const PickArgs a = pick_args(ps, w, nullptr, nullptr, B);
  const dim3 grid(B, D::NBR);
  hipLaunchKernelGGL(pick_attn_bwd_kernel, grid, dim3(ATT_THREADS), 0, s, a);
  hipLaunchKernelGGL(pick_lstm_bwd_kernel, grid, dim3(64), 0, s, a);
  launches += 2;
}

void pick_wgrad(PickState& ps, const float* x, float* grad, int B, hipStream_t s, int& launches) {
  const PickArgs a = pick_args(ps, nullptr, x, nullptr, B);
  hipLaunchKernelGGL(pick_wgrad_kernel, dim3(B, D::NBR), dim3(ATT_THREADS), 0, s, a);
  hipLaunchKernelGGL(pick_fold_kernel, dim3((PICK_PSZ + 255) / 256, D::NBR), dim3(256), 0, s, a, grad);
  launches += 2;
}

}  // namespace vp
