// Training batches from a device-resident waveform bank (include/volpick_hip.h, vp_bank_*): window cut with zero fill,
// demean + peak / std normalisation and Gaussian phase labels -- with a noise row for PhaseNet, with SeisBench's detection
// box for EQTransformer -- one workgroup per window.  The host plans every random choice (volpick_amd/generate.py); this file
// only executes the plan rows.  One descriptor (BatchSpec, batchgen.h) names a launch, bank_check and bank_launch serve every
// recipe, and the kernels are bank_block1_kernel<label kind> for plan rows, bank_aug_psn_kernel (x in registers, T <= 3072)
// and bank_aug_kernel<6, LABEL_DET> (x in LDS, T <= 6144) for augmented rows, the two on the same step helpers.
#include "batchgen.h"

#include <cmath>
#include <memory>

#include "philox.h"

namespace vp {

namespace {

// What every generation kernel takes.  A kernel reads the fields of its label kind and of its kind of rows alone.
struct GenArgs {
  const float* data;
  const long long* off;
  const long long* len;
  const double* onset;  // [trace][4]
  const vp_plan_row* rows;  // block 1's kernels: one plan row per window ...
  const vp_aug_row* aug;    // ... the augmented kernels: one record per window
  float* x;
  float* y;
  int T;
  int norm;
  float sigma;
  int row_p, row_s, row_n;  // rows of y; row_n: the noise row (LABEL_PSN)
  int row_det;              // the detection row (LABEL_DET)
  double fixed_window;      // LABEL_DET; >= 0: the detection ends fixed_window samples behind P; < 0: it follows S
};

constexpr int GEN_NTH = 1024, GEN_NWV = GEN_NTH / 64, GEN_MAXE = 6;  // T <= 6144: the window lives in registers
constexpr int GEN_MAX_T = GEN_NTH * GEN_MAXE;
constexpr int AUG_MAXE = 3, AUG_MAX_T = GEN_NTH * AUG_MAXE;  // augmented PhaseNet rows: T <= 3072 (three samples per thread)

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Reduction scratch of the statistics below.  Each function's first write to red follows the barrier behind its
// predecessor's last read of it, and every thread reads the result before the next function's second barrier, so calls
// may follow each other without a barrier in between.
struct GenShared {
  double red[3][GEN_NWV];
  double stat[3];
  float redf[3][GEN_NWV];
  float statf[3];
};

// x[c][t] = src[c][start + t] where lo <= start + t < hi (t < T), else 0.  lo / hi were checked against the trace's length
// on the host (bank_check).
template <int E>
__device__ __forceinline__ void gather_window(const GenArgs& a, const vp_plan_row& r, int tid, float v[3][E]) {
  const long long L = a.len[r.trace];
  const float* src = a.data + a.off[r.trace] + r.start;  // uniform: the loads below take a 32-bit per-lane offset
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const unsigned t = tid + k * GEN_NTH;
    const long long i = r.start + t;
    const bool in = t < (unsigned)a.T && i >= r.lo && i < r.hi;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][k] = in ? src[c * L + t] : 0.f;
  }
}

// Per-channel mean and normaliser of v over the T samples, in float64: a constant channel demeans to exact zeros (as
// numpy's float64 mean of float32 samples does), and the quotient (v - mean) / den is rounded to fp32 once.
// den = max|v - mean| (peak) or the population standard deviation, plus 1e-10.
template <int E>
__device__ __forceinline__ void window_stats(const float v[3][E], int T, bool peak, int tid, GenShared& sh,
                                             double mean[3], double den[3]) {
  const int lane = tid & 63, wave = tid >> 6;
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (double)v[c][k];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double ws = wave_sum_d(s[c]);
    if (lane == 0) sh.red[c][wave] = ws;
  }
  __syncthreads();
  if (tid < 3) {
    double acc = 0.0;
    for (int i = 0; i < GEN_NWV; ++i) acc += sh.red[tid][i];
    sh.stat[tid] = acc / (double)T;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) mean[c] = sh.stat[c];
  double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (tid + k * GEN_NTH < T) {
        const double d = (double)v[c][k] - mean[c];
        m[c] = peak ? fmax(m[c], fabs(d)) : m[c] + d * d;
      }
  __syncthreads();  // every thread has read stat[] before it is overwritten below
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double wm = peak ? wave_max_d(m[c]) : wave_sum_d(m[c]);
    if (lane == 0) sh.red[c][wave] = wm;
  }
  __syncthreads();
  if (tid < 3) {
    double acc = 0.0;
    for (int i = 0; i < GEN_NWV; ++i) acc = peak ? fmax(acc, sh.red[tid][i]) : acc + sh.red[tid][i];
    sh.stat[tid] = (peak ? acc : sqrt(acc / (double)T)) + 1e-10;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) den[c] = sh.stat[c];
}

// Per-channel maximum of m over the workgroup (fp32; m >= 0 or any sign, as the caller reduces).
__device__ __forceinline__ void block_max3(float m[3], int tid, GenShared& sh) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float wm = wave_max_f(m[c]);
    if (lane == 0) sh.redf[c][wave] = wm;
  }
  __syncthreads();
  if (tid < 3) {
    float acc = sh.redf[tid][0];
    for (int i = 1; i < GEN_NWV; ++i) acc = fmaxf(acc, sh.redf[tid][i]);
    sh.statf[tid] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) m[c] = sh.statf[c];
}

// A window's onsets relative to its start in float64 (traces of 10^6+ samples keep the fraction); has[j] = finite.
__device__ __forceinline__ void window_onsets(const GenArgs& a, const vp_plan_row& r, double o[4], bool has[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double on = a.onset[(long long)r.trace * 4 + j];
    has[j] = isfinite(on);
    o[j] = on - (double)r.start;
  }
}

// P (ph[0]) and S (ph[1]) at window sample t: the maximum over the phase's onsets of exp(-(t - o)^2 / two_s2), the
// distance narrowed to fp32 only once it is small where the Gaussian is not.
__device__ __forceinline__ void phase_labels(const double o[4], const bool has[4], long long t, float two_s2, float ph[2]) {
  ph[0] = ph[1] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (has[j]) {
      const float d = (float)((double)t - o[j]);
      ph[j >> 1] = fmaxf(ph[j >> 1], expf(-(d * d) / two_s2));
    }
}

// Window w of the batch: row r cut, demeaned and normalised into a.x.
__device__ __forceinline__ void write_window(const GenArgs& a, const vp_plan_row& r, int w, int tid, GenShared& sh) {
  const int T = a.T;
  float v[3][GEN_MAXE];
  gather_window(a, r, tid, v);
  double mean[3], den[3];
  window_stats(v, T, a.norm == VP_NORM_PEAK, tid, sh, mean, den);
  float* xw = a.x + (long long)w * 3 * T;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int k = 0; k < GEN_MAXE; ++k) {
      const int t = tid + k * GEN_NTH;
      if (t < T) xw[(long long)c * T + t] = (float)(((double)v[c][k] - mean[c]) / den[c]);
    }
  }
}

// SeisBench's DetectionLabeller (ndim == 2) on a window's onsets o (P, P, S, S; window-relative): the box is 1 on the
// integer samples t with lo <= t < hi, lo = max(int(p), 0), hi = max(int(s + factor (s - p)), 0), p and s the earliest
// finite P and S onsets, factor = 1.4; empty (lo = hi = 0) without a P or without an S, and for s < p.  A fixed window w
// puts s = p + w and factor = 0.  int() truncates toward zero; lo and hi stay doubles, so no onset overflows an integer.
__device__ __forceinline__ void detection_span(const double o[4], const bool has[4], double fixed_window, double& lo, double& hi) {
  // Python rounds the product, then the sum.  With contraction off for this block the compiler emits a multiply and an add
  // (what __dmul_rn / __dadd_rn stand for; the header's versions are plain operators that -ffp-contract=fast may still fuse):
  // p = -2304, s = -1101.5 must end at 582.0, not at the fused 581.9999999999999.
#pragma clang fp contract(off)
  lo = hi = 0.0;
  double p = INFINITY, s = INFINITY;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (has[j]) p = fmin(p, o[j]);
    if (has[2 + j]) s = fmin(s, o[2 + j]);
  }
  double factor = 1.4;
  if (fixed_window >= 0.0) {
    s = p + fixed_window;  // min_i (p_i + w) = min_i p_i + w: the sum is monotonic
    factor = 0.0;
  }
  if (!(p < INFINITY) || !(s < INFINITY) || s < p) return;
  const double span = s - p;
  const double tail = factor * span;
  const double end = s + tail;
  lo = fmax(trunc(p), 0.0);
  hi = fmax(trunc(end), 0.0);  // (a NaN end -- 0 * inf of onsets 10^308 apart -- gives 0: an empty box)
}

// Block 1, one window per workgroup: x for every label kind; LABEL_NONE: nothing else (vp_predict_bank: a.y, a.onset,
// a.sigma and the label rows are not read); LABEL_PSN: the P and S Gaussians and the noise row clip(1 - P - S, 0, 1);
// LABEL_DET: the same P and S bits, no noise row, and the detection box.
template <LabelKind K>
__global__ __launch_bounds__(GEN_NTH) void bank_block1_kernel(const GenArgs a) {
  __shared__ GenShared sh;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int T = a.T;
  const vp_plan_row r = a.rows[w];
  write_window(a, r, w, tid, sh);
  if constexpr (K != LABEL_NONE) {
    double o[4], lo = 0.0, hi = 0.0;
    bool has[4];
    window_onsets(a, r, o, has);
    if constexpr (K == LABEL_DET) detection_span(o, has, a.fixed_window, lo, hi);
    const float two_s2 = 2.f * a.sigma * a.sigma;
    float* yw = a.y + (long long)w * 3 * T;
    for (int t = tid; t < T; t += GEN_NTH) {
      float ph[2];
      phase_labels(o, has, t, two_s2, ph);
      yw[(long long)a.row_p * T + t] = ph[0];
      yw[(long long)a.row_s * T + t] = ph[1];
      if constexpr (K == LABEL_PSN)
        yw[(long long)a.row_n * T + t] = fminf(fmaxf(1.f - ph[0] - ph[1], 0.f), 1.f);
      else
        yw[(long long)a.row_det * T + t] = (double)t >= lo && (double)t < hi ? 1.f : 0.f;
    }
  }
}

// The standard normal of (key, channel c, sample t): include/volpick_hip.h, vp_aug_row step 5.
__device__ __forceinline__ double gauss_noise(uint64_t key, int c, int t) {
  uint32_t w[4] = {(uint32_t)t, (uint32_t)c, 0u, 0u};
  philox4x32_10(w, (uint32_t)key, (uint32_t)(key >> 32));
  const double u0 = (double)((((uint64_t)w[1] << 32) | w[0]) >> 11) * 0x1p-53;
  const double u1 = (double)((((uint64_t)w[3] << 32) | w[2]) >> 11) * 0x1p-53;
  return sqrt(-2.0 * log(1.0 - u0)) * cos(2.0 * M_PI * u1);
}

// ---- augmented rows (include/volpick_hip.h, vp_aug_row): what the two kernels below share -------------------------------------
// Row r cut, demeaned and normalised into v (fp32, 0 behind T): a primary window or a source.
template <int E>
__device__ __forceinline__ void load_normalised(const GenArgs& a, const vp_plan_row& r, int tid, GenShared& sh, float v[3][E]) {
  const int T = a.T;
  gather_window(a, r, tid, v);
  double mean[3], den[3];
  window_stats(v, T, a.norm == VP_NORM_PEAK, tid, sh, mean, den);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k) v[c][k] = tid + k * GEN_NTH < T ? (float)(((double)v[c][k] - mean[c]) / den[c]) : 0.f;
}

// A source window into v.  With zero_rule: the source's channels are zeroed where the current x is all |x| <= 1e-8, and
// max|x| over every channel is returned; x_max(false, m) is the kernel's max|x| per channel, taken behind the source's loads.
template <int E, class XMax>
__device__ __forceinline__ float load_source(const GenArgs& a, const vp_plan_row& r, int tid, GenShared& sh, float v[3][E],
                                             bool zero_rule, XMax x_max) {
  load_normalised(a, r, tid, sh, v);
  if (!zero_rule) return 0.f;
  float xmax[3];
  x_max(false, xmax);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (!(xmax[c] > 1e-8f))
#pragma unroll
      for (int k = 0; k < E; ++k) v[c][k] = 0.f;
  return fmaxf(fmaxf(xmax[0], xmax[1]), xmax[2]);
}

// Step 5: x plus Gaussian noise scaled by f = gauss * the signed maximum of x over every channel.
__device__ __forceinline__ double gauss_scale(const vp_aug_row& rec, const float xmax[3]) {
  return (double)rec.gauss * (double)fmaxf(fmaxf(xmax[0], xmax[1]), xmax[2]);
}
__device__ __forceinline__ float gauss_add(float x, double f, uint64_t key, int c, int t) {
  return (float)((double)x + f * gauss_noise(key, c, t));
}

// Step 7 (and block 1's last step): v demeaned and normalised into window w of a.x.
template <int E>
__device__ __forceinline__ void store_normalised(const GenArgs& a, const float v[3][E], int w, int tid, GenShared& sh) {
  const int T = a.T;
  double mean[3], den[3];
  window_stats(v, T, a.norm == VP_NORM_PEAK, tid, sh, mean, den);
  float* xw = a.x + (long long)w * 3 * T;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int t = tid + k * GEN_NTH;
      if (t < T) xw[(long long)c * T + t] = (float)(((double)v[c][k] - mean[c]) / den[c]);
    }
}

// The labels of row r shifted by d samples, merged into P, S and -- LABEL_DET and with_det -- D by maximum:
// label(t) = label_r(t - d) where 0 <= t - d < T, else 0 (which changes no maximum of labels >= 0).
template <int E, LabelKind K>
__device__ __forceinline__ void merge_labels(const GenArgs& a, const vp_plan_row& r, int d, bool with_det, int tid, float P[E],
                                             float S[E], float D[E]) {
  double o[4], lo = 0.0, hi = 0.0;
  bool has[4];
  window_onsets(a, r, o, has);
  if constexpr (K == LABEL_DET) detection_span(o, has, a.fixed_window, lo, hi);
  const float two_s2 = 2.f * a.sigma * a.sigma;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int ts = tid + k * GEN_NTH - d;
    if (ts < 0 || ts >= a.T) continue;
    float ph[2];
    phase_labels(o, has, ts, two_s2, ph);
    P[k] = fmaxf(P[k], ph[0]);
    S[k] = fmaxf(S[k], ph[1]);
    if (K == LABEL_DET && with_det && (double)ts >= lo && (double)ts < hi) D[k] = 1.f;
  }
}

// v again, behind a wall the compiler does not see through: what follows from it (addresses, bounds predicates) is computed
// where it is used, not hoisted to the head of the kernel and held in registers -- or spilled -- across every step.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// The labels of window w (steps 1, 3 and 6).  No step on x reads a label, and a label follows from onsets, shifts and the
// gap alone; so both kernels form P, S and D once, behind the store of x:
//   LABEL_DET (vp_bank_make_batch_eqt_aug): the maximum over the primary and the event sources, the detection box of an
//     event merged only when the event was shifted; 0 in the gap;
//   LABEL_PSN (vp_bank_make_batch_aug): behind each event's maximum P and S are divided by max(1, P + S), in event order;
//     0 in the gap; noise = 1 - P - S, clipped to [0, 1] unless an event renormalised y.
template <int E, LabelKind K>
__device__ __forceinline__ void write_aug_labels(const GenArgs& a, const vp_aug_row& rec, const vp_plan_row& pr, int w, int tid0) {
  static_assert(K != LABEL_NONE, "augmented rows carry labels");
  const int T = a.T, g0 = rec.gap_lo, g1 = rec.gap_hi;
  float P[E], S[E], D[E];
#pragma unroll
  for (int k = 0; k < E; ++k) P[k] = S[k] = D[k] = 0.f;
  const int tid = opaque(tid0);
  merge_labels<E, K>(a, pr, 0, true, tid, P, S, D);
  bool renorm = false;
#pragma unroll 1
  for (int i = 0; i < 2; ++i) {
    const vp_aug_event& ev = rec.event[i];
    if (ev.kind == VP_AUG_NONE) continue;
    vp_plan_row sr = pr;
    if (ev.kind == VP_AUG_BANK) sr = ev.row;
    merge_labels<E, K>(a, sr, ev.shift, ev.shift != 0, opaque(tid0), P, S, D);
    if constexpr (K == LABEL_PSN) {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float dn = fmaxf(1.f, P[k] + S[k]);
        P[k] = P[k] / dn;
        S[k] = S[k] / dn;
      }
      renorm = true;
    }
  }
  float* yw = a.y + (long long)w * 3 * T;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int t = tid + k * GEN_NTH;
    if (t >= T) continue;
    const bool gap = t >= g0 && t < g1;
    const float p = gap ? 0.f : P[k], q = gap ? 0.f : S[k];
    yw[(long long)a.row_p * T + t] = p;
    yw[(long long)a.row_s * T + t] = q;
    if constexpr (K == LABEL_PSN) {
      const float n = 1.f - p - q;
      yw[(long long)a.row_n * T + t] = renorm ? n : fminf(fmaxf(n, 0.f), 1.f);
    } else {
      yw[(long long)a.row_det * T + t] = gap ? 0.f : D[k];
    }
  }
}

// One augmented PhaseNet window per workgroup (vp_bank_make_batch_aug, T <= 3072): the record's steps in order with x and
// the P / S labels in registers, three samples per thread beside one source; each event source is shifted through LDS one
// channel at a time.  (The LDS form below, instantiated at E = 3, writes the same bits and is slower, and so is this form
// with its labels formed behind the store of x: profiles/batchgen_refactor_ab_parent.txt.)
__global__ __launch_bounds__(GEN_NTH) void bank_aug_psn_kernel(const GenArgs a) {
  constexpr int E = AUG_MAXE;
  __shared__ GenShared sh;
  __shared__ float stage[AUG_MAX_T];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int T = a.T;
  const vp_aug_row& rec = a.aug[w];
  const vp_plan_row pr = rec.primary;
  float x[3][E], s[3][E];

  // max|x| per channel (sign = false) or max x (sign = true) over the window: m[c] for every thread
  auto x_max = [&](bool sign, float m[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[c] = sign ? -INFINITY : 0.f;
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (tid + k * GEN_NTH < T) m[c] = fmaxf(m[c], sign ? x[c][k] : fabsf(x[c][k]));
    }
    block_max3(m, tid, sh);
  };

  // 1. the primary window, as bank_block1_kernel writes it; 2. the truncation behind the first event
  load_normalised(a, pr, tid, sh, x);
  const int cut = rec.cut;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (tid + k * GEN_NTH >= cut) x[c][k] = 0.f;
  float P[E], S[E], D[E];  // (D: LABEL_DET's, unused)
#pragma unroll
  for (int k = 0; k < E; ++k) P[k] = S[k] = D[k] = 0.f;
  merge_labels<E, LABEL_PSN>(a, pr, 0, false, tid, P, S, D);
  bool renorm = false;  // y renormalised by an event: noise = 1 - P - S, else clip(1 - P - S, 0, 1)

  // 3. events: a duplicate is the primary window as step 1 left it, cut and normalised again to the same bits
#pragma unroll 1
  for (int i = 0; i < 2; ++i) {
    const vp_aug_event& ev = rec.event[i];
    if (ev.kind == VP_AUG_NONE) continue;
    const bool bank = ev.kind == VP_AUG_BANK;
    vp_plan_row sr = pr;  // (a copy, not a reference to one of two: pr stays in registers)
    if (bank) sr = ev.row;
    load_source(a, sr, tid, sh, s, bank, x_max);
    const int zb = ev.zero_before, d = ev.shift;
    const float scale = ev.scale;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int t = tid + k * GEN_NTH;
        if (t < T) stage[t] = t < zb ? 0.f : s[c][k];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int t = tid + k * GEN_NTH, ts = t - d;
        if (t < T && ts >= 0 && ts < T) x[c][k] += scale * stage[ts];
      }
      __syncthreads();
    }
    merge_labels<E, LABEL_PSN>(a, sr, d, false, tid, P, S, D);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float dn = fmaxf(1.f, P[k] + S[k]);
      P[k] = P[k] / dn;
      S[k] = S[k] / dn;
    }
    renorm = true;
  }

  // 4. noise windows
#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const vp_aug_noise& nz = rec.noise[j];
    if (nz.kind == VP_AUG_NONE) continue;
    const float f = load_source(a, nz.row, tid, sh, s, true, x_max) * nz.scale;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < E; ++k) x[c][k] += s[c][k] * f;
  }

  // 5. Gaussian noise scaled by the signed maximum of x
  if (rec.gauss > 0.f) {
    float m[3];
    x_max(true, m);
    const double f = gauss_scale(rec, m);
    const uint64_t key = rec.noise_key;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int t = tid + k * GEN_NTH;
        if (t < T) x[c][k] = gauss_add(x[c][k], f, key, c, t);
      }
  }

  // 6. the gap in x, 7. the second normalisation
  const int g0 = rec.gap_lo, g1 = rec.gap_hi;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int t = tid + k * GEN_NTH;
    if (t >= g0 && t < g1)
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c][k] = 0.f;
  }
  store_normalised(a, x, w, tid, sh);
  float* yw = a.y + (long long)w * 3 * T;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int t = tid + k * GEN_NTH;
    if (t >= T) continue;
    const bool gap = t >= g0 && t < g1;
    const float p = gap ? 0.f : P[k], q = gap ? 0.f : S[k], n = 1.f - p - q;
    yw[(long long)a.row_p * T + t] = p;
    yw[(long long)a.row_s * T + t] = q;
    yw[(long long)a.row_n * T + t] = renorm ? n : fminf(fmaxf(n, 0.f), 1.f);
  }
}

// One augmented window per workgroup, T <= 1024 E (vp_bank_make_batch_eqt_aug at E = 6): the same steps where x, a source
// and the float64 statistics together do not fit the 128 registers of a 1024-thread workgroup.  x lives in LDS between
// steps 1 and 7 -- xs[c][t], every sample read and written by the one thread t % 1024, hence without barriers of its own --
// and registers hold one window at a time: the primary, a source, then x for step 7.  A source is shifted through a second
// LDS row, one channel at a time.
template <int E, LabelKind K>
__global__ __launch_bounds__(GEN_NTH) void bank_aug_kernel(const GenArgs a) {
  __shared__ GenShared sh;
  __shared__ float stage[E * GEN_NTH];
  __shared__ float xs[3][E * GEN_NTH];
  const int w = blockIdx.x, tid0 = threadIdx.x;
  const int T = a.T;
  const vp_aug_row& rec = a.aug[w];
  const vp_plan_row pr = rec.primary;
  float v[3][E];

  // max|x| per channel (sign = false) or max x (sign = true) over the window: m[c] for every thread
  auto x_max = [&](bool sign, float m[3]) {
    const int tid = opaque(tid0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[c] = sign ? -INFINITY : 0.f;
      for (int t = tid; t < T; t += GEN_NTH) m[c] = fmaxf(m[c], sign ? xs[c][t] : fabsf(xs[c][t]));
    }
    block_max3(m, tid, sh);
  };

  // 1. the primary window, as bank_block1_kernel writes it; 2. the truncation behind the first event
  load_normalised(a, pr, opaque(tid0), sh, v);
  const int cut = rec.cut;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int t = tid0 + k * GEN_NTH;
      if (t < T) xs[c][t] = t < cut ? v[c][k] : 0.f;
    }

  // 3. events: a duplicate is the primary window as step 1 left it, cut and normalised again to the same bits
#pragma unroll 1
  for (int i = 0; i < 2; ++i) {
    const vp_aug_event& ev = rec.event[i];
    if (ev.kind == VP_AUG_NONE) continue;
    const bool bank = ev.kind == VP_AUG_BANK;
    vp_plan_row sr = pr;  // (a copy, not a reference to one of two: pr stays in registers)
    if (bank) sr = ev.row;
    load_source(a, sr, opaque(tid0), sh, v, bank, x_max);
    const int zb = ev.zero_before, d = ev.shift;
    const float scale = ev.scale;
    const int tid = opaque(tid0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int t = tid + k * GEN_NTH;
        if (t < T) stage[t] = t < zb ? 0.f : v[c][k];
      }
      __syncthreads();
      for (int t = tid; t < T; t += GEN_NTH) {
        const int ts = t - d;
        if (ts >= 0 && ts < T) xs[c][t] += scale * stage[ts];
      }
      __syncthreads();
    }
  }

  // 4. noise windows
#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const vp_aug_noise& nz = rec.noise[j];
    if (nz.kind == VP_AUG_NONE) continue;
    const float f = load_source(a, nz.row, opaque(tid0), sh, v, true, x_max) * nz.scale;
    const int tid = opaque(tid0);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int t = tid + k * GEN_NTH;
        if (t < T) xs[c][t] += v[c][k] * f;
      }
  }

  // 5. Gaussian noise scaled by the signed maximum of x
  if (rec.gauss > 0.f) {
    float m[3];
    x_max(true, m);
    const double f = gauss_scale(rec, m);
    const uint64_t key = rec.noise_key;
    const int tid = opaque(tid0);
#pragma unroll 1
    for (int c = 0; c < 3; ++c)
#pragma unroll 1
      for (int t = tid; t < T; t += GEN_NTH) xs[c][t] = gauss_add(xs[c][t], f, key, c, t);
  }

  // 6. the gap in x, 7. the second normalisation
  const int g0 = rec.gap_lo, g1 = rec.gap_hi;
  const int tid = opaque(tid0);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int t = tid + k * GEN_NTH;
      v[c][k] = t < T && !(t >= g0 && t < g1) ? xs[c][t] : 0.f;
    }
  store_normalised(a, v, w, tid, sh);
  write_aug_labels<E, K>(a, rec, pr, w, tid0);
}

}  // namespace

int RowRing::reserve(size_t bytes) {
  if (bytes <= cap) return VP_OK;
  for (int i = 0; i < N; ++i) {
    if (host[i]) VP_HIP(hipHostFree(host[i]));
    if (dev[i]) VP_HIP(hipFree(dev[i]));
    host[i] = nullptr;
    dev[i] = nullptr;
  }
  cap = 0;
  for (int i = 0; i < N; ++i) {
    VP_HIP(hipHostMalloc(&host[i], bytes, hipHostMallocDefault));
    VP_HIP(hipMalloc(&dev[i], bytes));
  }
  cap = bytes;
  return VP_OK;
}

void* RowRing::stage(int slot, std::initializer_list<Piece> pieces, hipStream_t s) {
  size_t bytes = 0;
  for (const Piece& piece : pieces) {
    if (piece.bytes) memcpy(static_cast<char*>(host[slot]) + bytes, piece.p, piece.bytes);
    bytes += piece.bytes;
  }
  if (hipMemcpyAsync(dev[slot], host[slot], bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
    set_error("plan rows: hipMemcpyAsync failed");
    return nullptr;
  }
  return dev[slot];
}

RowRing::~RowRing() {
  for (int i = 0; i < N; ++i) {
    if (host[i]) (void)hipHostFree(host[i]);
    if (dev[i]) (void)hipFree(dev[i]);
  }
}

int StagingRing::acquire(size_t bytes, size_t at_least) {
  if (!ev[0])
    for (hipEvent_t& e : ev) VP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (bytes > ring.cap) {  // every slot idle before the ring is reallocated
    for (int i = 0; i < RowRing::N; ++i)
      if (ev_used[i]) VP_HIP(hipEventSynchronize(ev[i]));
    return ring.reserve(std::max(bytes, at_least));
  }
  // the launches that read this slot last (and so the copy into it) have run: N uses back, long so in the steady state
  if (ev_used[slot()]) VP_HIP(hipEventSynchronize(ev[slot()]));
  return VP_OK;
}

int StagingRing::retire(hipStream_t s) {
  VP_HIP(hipEventRecord(ev[slot()], s));
  ev_used[slot()] = true;
  ++uses;
  return VP_OK;
}

StagingRing::~StagingRing() {
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
}

Bank::~Bank() {
  for (void* p : {(void*)data, (void*)off_dev, (void*)len_dev, (void*)onset_dev})
    if (p) (void)hipFree(p);
}

namespace {

// B and the spec's own fields; `pre` names the kind of batch in the messages ("bank batch", "bank windows").  A batch
// without labels has no label rows and no sigma to check.
int args_check(const char* pre, int B, const BatchSpec& sp) {
  const bool labelled = sp.labels != LABEL_NONE;
  VP_REQUIRE(!labelled || sp.label_rows, "%s: null label_rows", pre);
  VP_REQUIRE(B >= 1, "%s: B = %d", pre, B);
  VP_REQUIRE(sp.T >= 1 && sp.T <= GEN_MAX_T, "%s: T = %d outside [1, %d]", pre, sp.T, GEN_MAX_T);
  VP_REQUIRE(!labelled || (std::isfinite(sp.sigma) && sp.sigma > 0.f), "%s: sigma = %g must be finite and > 0", pre, (double)sp.sigma);
  VP_REQUIRE(sp.norm == VP_NORM_PEAK || sp.norm == VP_NORM_STD, "%s: norm %d is neither VP_NORM_PEAK nor VP_NORM_STD", pre, sp.norm);
  int seen = labelled ? 0 : 7;
  for (int i = 0; labelled && i < 3; ++i) {
    VP_REQUIRE(sp.label_rows[i] >= 0 && sp.label_rows[i] < 3, "%s: label_rows[%d] = %d outside [0, 3)", pre, i, sp.label_rows[i]);
    seen |= 1 << sp.label_rows[i];
  }
  VP_REQUIRE(seen == 7, "%s: label_rows is not a permutation of 0, 1, 2", pre);
  return VP_OK;
}

// One vp_plan_row against the bank (`what`: where it sits in the batch, for the message).
int row_check(const Bank& bk, const vp_plan_row& r, int b, const char* what) {
  VP_REQUIRE(r.trace >= 0 && r.trace < bk.n_written, "bank batch: %s %d: trace %d outside [0, %lld)", what, b, (int)r.trace,
             bk.n_written);
  const long long L = bk.len[r.trace];
  VP_REQUIRE(r.lo >= 0 && r.lo <= r.hi && r.hi <= L, "bank batch: %s %d: [lo, hi) = [%lld, %lld) outside [0, %lld]", what,
             b, (long long)r.lo, (long long)r.hi, L);
  // start + t must not overflow for t < T (the kernel's index arithmetic)
  VP_REQUIRE(r.start > -(1LL << 62) && r.start < (1LL << 62), "bank batch: %s %d: start %lld out of range", what, b,
             (long long)r.start);
  return VP_OK;
}

bool row_is_zero(const vp_plan_row& r) { return !r.trace && !r.reserved && !r.start && !r.lo && !r.hi; }

// Every field of one augmented row.
int aug_row_check(const Bank& bk, const vp_aug_row& r, int b, int T) {
  int rc;
  if ((rc = row_check(bk, r.primary, b, "row")) != VP_OK) return rc;
  for (int i = 0; i < 2; ++i) {
    const vp_aug_event& e = r.event[i];
    VP_REQUIRE(e.kind >= VP_AUG_NONE && e.kind <= VP_AUG_SELF, "bank batch: row %d: event %d: kind %d", b, i, (int)e.kind);
    if (e.kind == VP_AUG_NONE) {
      VP_REQUIRE(row_is_zero(e.row) && !e.zero_before && !e.shift && e.scale == 0.f,
                 "bank batch: row %d: event %d is unused but not zero", b, i);
      continue;
    }
    if (e.kind == VP_AUG_BANK) {
      if ((rc = row_check(bk, e.row, b, "event source of row")) != VP_OK) return rc;
    } else {
      VP_REQUIRE(row_is_zero(e.row), "bank batch: row %d: event %d duplicates the window but has a source row", b, i);
    }
    VP_REQUIRE(e.zero_before >= 0 && e.zero_before <= T, "bank batch: row %d: event %d: zero_before %d outside [0, %d]",
               b, i, (int)e.zero_before, T);
    VP_REQUIRE(e.shift >= -T && e.shift <= T, "bank batch: row %d: event %d: |shift| = |%d| > T = %d", b, i, (int)e.shift,
               T);
    VP_REQUIRE(std::isfinite(e.scale) && e.scale >= 0.f, "bank batch: row %d: event %d: scale %g", b, i, (double)e.scale);
  }
  for (int j = 0; j < 2; ++j) {
    const vp_aug_noise& n = r.noise[j];
    VP_REQUIRE(n.kind == VP_AUG_NONE || n.kind == VP_AUG_BANK, "bank batch: row %d: noise %d: kind %d", b, j, (int)n.kind);
    if (n.kind == VP_AUG_NONE) {
      VP_REQUIRE(row_is_zero(n.row) && n.scale == 0.f, "bank batch: row %d: noise %d is unused but not zero", b, j);
      continue;
    }
    if ((rc = row_check(bk, n.row, b, "noise source of row")) != VP_OK) return rc;
    VP_REQUIRE(std::isfinite(n.scale) && n.scale >= 0.f, "bank batch: row %d: noise %d: scale %g", b, j, (double)n.scale);
  }
  VP_REQUIRE(std::isfinite(r.gauss) && r.gauss >= 0.f, "bank batch: row %d: gauss %g", b, (double)r.gauss);
  VP_REQUIRE(r.gauss > 0.f || r.noise_key == 0, "bank batch: row %d: a noise key without Gaussian noise", b);
  VP_REQUIRE(r.cut >= 0 && r.cut <= T, "bank batch: row %d: cut %d outside [0, %d]", b, (int)r.cut, T);
  VP_REQUIRE(r.gap_lo >= 0 && r.gap_lo <= r.gap_hi && r.gap_hi <= T, "bank batch: row %d: gap [%d, %d) outside [0, %d]", b,
             (int)r.gap_lo, (int)r.gap_hi, T);
  return VP_OK;
}

}  // namespace

int bank_check(const Bank& bk, const BatchSpec& sp, BatchRows rows, int B) {
  const char* pre = sp.labels == LABEL_NONE ? "bank windows" : "bank batch";
  VP_REQUIRE(rows.p, "%s: null rows", pre);
  int rc = args_check(pre, B, sp);
  if (rc != VP_OK) return rc;
  if (rows.aug) {
    VP_REQUIRE(sp.labels != LABEL_NONE, "%s: augmented rows carry labels", pre);
    const int max_T = sp.labels == LABEL_PSN ? AUG_MAX_T : GEN_MAX_T;  // what the executing kernel holds
    VP_REQUIRE(sp.T <= max_T, "bank batch: augmented rows: T = %d outside [1, %d]", sp.T, max_T);
  }
  for (int b = 0; b < B; ++b) {
    rc = rows.aug ? aug_row_check(bk, static_cast<const vp_aug_row*>(rows.p)[b], b, sp.T)
                  : row_check(bk, static_cast<const vp_plan_row*>(rows.p)[b], b, "row");
    if (rc != VP_OK) return rc;
  }
  VP_REQUIRE(sp.labels != LABEL_DET || sp.det_fixed_window < 0.f || std::isfinite(sp.det_fixed_window),
             "bank batch: det_fixed_window = %g is neither negative nor a finite length", (double)sp.det_fixed_window);  // (a NaN fails both)
  return VP_OK;
}

int bank_launch(const Bank& bk, const BatchSpec& sp, BatchRows rows_dev, int B, float* x, float* y, hipStream_t s) {
  struct Kernel {
    void (*fn)(GenArgs);
    const char* name;
  };
  static const Kernel kernels[2][3] = {  // [augmented rows][label kind]
      {{bank_block1_kernel<LABEL_NONE>, "bank_block1_kernel<LABEL_NONE>"},
       {bank_block1_kernel<LABEL_PSN>, "bank_block1_kernel<LABEL_PSN>"},
       {bank_block1_kernel<LABEL_DET>, "bank_block1_kernel<LABEL_DET>"}},
      {{nullptr, "no kernel for augmented rows without labels"},
       {bank_aug_psn_kernel, "bank_aug_psn_kernel"},
       {bank_aug_kernel<GEN_MAXE, LABEL_DET>, "bank_aug_kernel<6, LABEL_DET>"}}};
  const Kernel& k = kernels[rows_dev.aug][sp.labels];
  if (!k.fn) {  // (bank_check refuses them)
    set_error("%s", k.name);
    return VP_ERR_INVALID;
  }
  GenArgs a{};
  a.data = bk.data;
  a.off = bk.off_dev;
  a.len = bk.len_dev;
  a.onset = bk.onset_dev;
  if (rows_dev.aug)
    a.aug = static_cast<const vp_aug_row*>(rows_dev.p);
  else
    a.rows = static_cast<const vp_plan_row*>(rows_dev.p);
  a.x = x;
  a.y = y;
  a.T = sp.T;
  a.norm = sp.norm;
  a.sigma = sp.sigma;
  const int* lr = sp.label_rows;
  a.row_p = a.row_s = a.row_n = a.row_det = -1;  // a kernel reads the rows of its label kind alone
  if (sp.labels == LABEL_PSN) a.row_p = lr[0], a.row_s = lr[1], a.row_n = lr[2];
  if (sp.labels == LABEL_DET) a.row_det = lr[0], a.row_p = lr[1], a.row_s = lr[2];
  a.fixed_window = sp.det_fixed_window < 0.f ? -1.0 : (double)sp.det_fixed_window;
  hipLaunchKernelGGL(k.fn, dim3(B), dim3(GEN_NTH), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s launch failed: %s", k.name, hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp

using namespace vp;

namespace {

// The four vp_bank_make_batch* entry points: the rows staged through the bank's ring, slot k reused once the kernel that
// last read it has run.
int make_batch(vp_bank* h, const char* who, const BatchSpec& sp, BatchRows rows, int B, float* x, float* y, void* stream) {
  VP_REQUIRE(h && x && y, "%s: null argument", who);
  Bank& bk = *reinterpret_cast<Bank*>(h);
  int rc = bank_check(bk, sp, rows, B);
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(bk.device));
  if ((rc = bk.ring.acquire(rows.bytes(B))) != VP_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const void* rd = bk.ring.stage({{rows.p, rows.bytes(B)}}, s);
  if (!rd) return VP_ERR_HIP;
  if ((rc = bank_launch(bk, sp, rows.at(rd), B, x, y, s)) != VP_OK) return rc;
  return bk.ring.retire(s);
}

}  // namespace

extern "C" {

int vp_bank_create(int device_id, long long n_traces, long long n_floats_total, vp_bank** out) {
  VP_REQUIRE(out && n_traces >= 1 && n_traces <= INT32_MAX && n_floats_total >= 0, "vp_bank_create: bad argument");
  auto bk = std::make_unique<Bank>();
  bk->device = device_id;
  bk->n_traces = n_traces;
  bk->n_floats = n_floats_total;
  bk->len.reserve((size_t)n_traces);
  VP_HIP(hipSetDevice(device_id));
  VP_HIP(hipMalloc((void**)&bk->data, (size_t)std::max(n_floats_total, 1LL) * sizeof(float)));
  VP_HIP(hipMalloc((void**)&bk->off_dev, (size_t)n_traces * sizeof(long long)));
  VP_HIP(hipMalloc((void**)&bk->len_dev, (size_t)n_traces * sizeof(long long)));
  VP_HIP(hipMalloc((void**)&bk->onset_dev, (size_t)n_traces * 4 * sizeof(double)));
  *out = reinterpret_cast<vp_bank*>(bk.release());
  return VP_OK;
}

int vp_bank_write(vp_bank* h, long long first_trace, long long n_traces, const float* data, int mem,
                  const int64_t* trace_lengths, const double* onsets) {
  VP_REQUIRE(h && data && trace_lengths && onsets && n_traces >= 1, "vp_bank_write: bad argument");
  VP_REQUIRE(mem == VP_MEM_HOST || mem == VP_MEM_DEVICE, "vp_bank_write: mem %d", mem);
  Bank& bk = *reinterpret_cast<Bank*>(h);
  VP_REQUIRE(first_trace == bk.n_written, "vp_bank_write: traces are written in order: next is %lld, got %lld",
             bk.n_written, first_trace);
  VP_REQUIRE(n_traces <= bk.n_traces - bk.n_written, "vp_bank_write: %lld traces past the bank's %lld", n_traces, bk.n_traces);
  long long floats = 0;
  std::vector<long long> off((size_t)n_traces), len((size_t)n_traces);
  for (long long i = 0; i < n_traces; ++i) {
    VP_REQUIRE(trace_lengths[i] >= 0, "vp_bank_write: trace %lld has length %lld", first_trace + i, (long long)trace_lengths[i]);
    off[i] = bk.floats_written + floats;
    len[i] = trace_lengths[i];
    floats += 3 * trace_lengths[i];
  }
  VP_REQUIRE(floats <= bk.n_floats - bk.floats_written, "vp_bank_write: %lld floats past the bank's %lld", floats, bk.n_floats);
  VP_HIP(hipSetDevice(bk.device));
  VP_HIP(hipDeviceSynchronize());  // a device source is complete, whichever stream produced it
  VP_HIP(hipMemcpy(bk.data + bk.floats_written, data, (size_t)floats * sizeof(float),
                   mem == VP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  VP_HIP(hipMemcpy(bk.off_dev + first_trace, off.data(), (size_t)n_traces * sizeof(long long), hipMemcpyHostToDevice));
  VP_HIP(hipMemcpy(bk.len_dev + first_trace, len.data(), (size_t)n_traces * sizeof(long long), hipMemcpyHostToDevice));
  VP_HIP(hipMemcpy(bk.onset_dev + 4 * first_trace, onsets, (size_t)n_traces * 4 * sizeof(double), hipMemcpyHostToDevice));
  VP_HIP(hipDeviceSynchronize());  // batches enqueued on any stream afterwards see the data
  bk.len.insert(bk.len.end(), len.begin(), len.end());
  bk.off.insert(bk.off.end(), off.begin(), off.end());
  bk.n_written += n_traces;
  bk.floats_written += floats;
  return VP_OK;
}

int vp_bank_read(vp_bank* h, long long trace, float* out, int mem) {
  VP_REQUIRE(h && out, "vp_bank_read: null argument");
  VP_REQUIRE(mem == VP_MEM_HOST || mem == VP_MEM_DEVICE, "vp_bank_read: mem %d", mem);
  Bank& bk = *reinterpret_cast<Bank*>(h);
  VP_REQUIRE(trace >= 0 && trace < bk.n_written, "vp_bank_read: trace %lld outside [0, %lld)", trace, bk.n_written);
  VP_HIP(hipSetDevice(bk.device));
  VP_HIP(hipDeviceSynchronize());  // the trace is complete, whichever stream assembled it
  VP_HIP(hipMemcpy(out, bk.data + bk.off[(size_t)trace], (size_t)(3 * bk.len[(size_t)trace]) * sizeof(float),
                   mem == VP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return VP_OK;
}

int vp_bank_destroy(vp_bank* h) {
  if (!h) return VP_OK;
  Bank* bk = reinterpret_cast<Bank*>(h);
  const hipError_t e1 = hipSetDevice(bk->device);
  const hipError_t e2 = e1 == hipSuccess ? hipDeviceSynchronize() : e1;
  delete bk;
  if (e2 != hipSuccess) {
    set_error("vp_bank_destroy: %s", hipGetErrorString(e2));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

int vp_bank_make_batch(vp_bank* h, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                       float* x, float* y, void* stream) {
  return make_batch(h, "vp_bank_make_batch", {T, sigma, norm, LABEL_PSN, label_rows}, rows, B, x, y, stream);
}

int vp_bank_make_batch_eqt(vp_bank* h, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                           float det_fixed_window, float* x, float* y, void* stream) {
  return make_batch(h, "vp_bank_make_batch_eqt", {T, sigma, norm, LABEL_DET, label_rows, det_fixed_window}, rows, B, x, y, stream);
}

int vp_bank_make_batch_aug(vp_bank* h, const vp_aug_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                           float* x, float* y, void* stream) {
  return make_batch(h, "vp_bank_make_batch_aug", {T, sigma, norm, LABEL_PSN, label_rows}, rows, B, x, y, stream);
}

int vp_bank_make_batch_eqt_aug(vp_bank* h, const vp_aug_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                               float det_fixed_window, float* x, float* y, void* stream) {
  return make_batch(h, "vp_bank_make_batch_eqt_aug", {T, sigma, norm, LABEL_DET, label_rows, det_fixed_window}, rows, B, x, y,
                    stream);
}

}  // extern "C"
