// Training batches from a device-resident waveform bank (include/volpick_hip.h, vp_bank_*): window cut with zero fill,
// demean + peak / std normalisation and Gaussian phase labels, one workgroup per window.  The host plans every random
// choice (volpick_amd/generate.py); this file only executes the plan rows.
#include "batchgen.h"

#include <cmath>
#include <memory>

namespace vp {

namespace {

struct GenArgs {
  const float* data;
  const long long* off;
  const long long* len;
  const double* onset;  // [trace][4]
  const vp_plan_row* rows;
  float* x;
  float* y;
  int T;
  int norm;
  float sigma;
  int row_p, row_s, row_n;
};

constexpr int GEN_NTH = 1024, GEN_NWV = GEN_NTH / 64, GEN_MAXE = 6;  // T <= 6144: the window lives in registers
constexpr int GEN_MAX_T = GEN_NTH * GEN_MAXE;

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

// Statistics in float64: a constant channel demeans to exact zeros (as numpy's float64 mean of float32 samples does), and
// the quotient is rounded to fp32 once.  The gather reads [lo, hi) of the row's trace only; lo / hi were checked against
// the trace's length on the host (bank_check).
__global__ __launch_bounds__(GEN_NTH) void bank_batch_kernel(const GenArgs a) {
  __shared__ double red[3][GEN_NWV];
  __shared__ double stat[3];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T;
  const vp_plan_row r = a.rows[w];
  const long long L = a.len[r.trace];
  const float* src = a.data + a.off[r.trace];

  float v[3][GEN_MAXE];
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < GEN_MAXE; ++k) {
    const int t = tid + k * GEN_NTH;
    const long long i = r.start + t;
    const bool in = t < T && i >= r.lo && i < r.hi;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c][k] = in ? src[c * L + i] : 0.f;
      s[c] += (double)v[c][k];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double ws = wave_sum_d(s[c]);
    if (lane == 0) red[c][wave] = ws;
  }
  __syncthreads();
  if (tid < 3) {
    double acc = 0.0;
    for (int i = 0; i < GEN_NWV; ++i) acc += red[tid][i];
    stat[tid] = acc / (double)T;
  }
  __syncthreads();
  const double mean[3] = {stat[0], stat[1], stat[2]};
  const bool peak = a.norm == VP_NORM_PEAK;  // uniform
  double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < GEN_MAXE; ++k)
      if (tid + k * GEN_NTH < T) {
        const double d = (double)v[c][k] - mean[c];
        m[c] = peak ? fmax(m[c], fabs(d)) : m[c] + d * d;
      }
  __syncthreads();  // every thread has read stat[] before it is overwritten below
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double wm = peak ? wave_max_d(m[c]) : wave_sum_d(m[c]);
    if (lane == 0) red[c][wave] = wm;
  }
  __syncthreads();
  if (tid < 3) {
    double acc = 0.0;
    for (int i = 0; i < GEN_NWV; ++i) acc = peak ? fmax(acc, red[tid][i]) : acc + red[tid][i];
    stat[tid] = (peak ? acc : sqrt(acc / (double)T)) + 1e-10;
  }
  __syncthreads();
  float* xw = a.x + (long long)w * 3 * T;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double den = stat[c];
#pragma unroll
    for (int k = 0; k < GEN_MAXE; ++k) {
      const int t = tid + k * GEN_NTH;
      if (t < T) xw[(long long)c * T + t] = (float)(((double)v[c][k] - mean[c]) / den);
    }
  }

  // labels: the onsets relative to the window start in float64 (traces of 10^6+ samples keep the fraction), the
  // distance to each sample narrowed to fp32 only once it is small where the Gaussian is not
  double o[4];
  bool has[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double on = a.onset[(long long)r.trace * 4 + j];
    has[j] = isfinite(on);
    o[j] = on - (double)r.start;
  }
  const float two_s2 = 2.f * a.sigma * a.sigma;
  float* yw = a.y + (long long)w * 3 * T;
  for (int t = tid; t < T; t += GEN_NTH) {
    float ph[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (has[j]) {
        const float d = (float)((double)t - o[j]);
        ph[j >> 1] = fmaxf(ph[j >> 1], expf(-(d * d) / two_s2));
      }
    yw[(long long)a.row_p * T + t] = ph[0];
    yw[(long long)a.row_s * T + t] = ph[1];
    yw[(long long)a.row_n * T + t] = fminf(fmaxf(1.f - ph[0] - ph[1], 0.f), 1.f);
  }
}

}  // namespace

int RowRing::reserve(int n) {
  if (n <= cap) return VP_OK;
  for (int i = 0; i < N; ++i) {
    if (host[i]) VP_HIP(hipHostFree(host[i]));
    if (dev[i]) VP_HIP(hipFree(dev[i]));
    host[i] = nullptr;
    dev[i] = nullptr;
  }
  cap = 0;
  for (int i = 0; i < N; ++i) {
    VP_HIP(hipHostMalloc((void**)&host[i], (size_t)n * sizeof(vp_plan_row), hipHostMallocDefault));
    VP_HIP(hipMalloc((void**)&dev[i], (size_t)n * sizeof(vp_plan_row)));
  }
  cap = n;
  return VP_OK;
}

vp_plan_row* RowRing::stage(int slot, const vp_plan_row* rows, int n, hipStream_t s) {
  memcpy(host[slot], rows, (size_t)n * sizeof(vp_plan_row));
  if (hipMemcpyAsync(dev[slot], host[slot], (size_t)n * sizeof(vp_plan_row), hipMemcpyHostToDevice, s) != hipSuccess) {
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

Bank::~Bank() {
  for (void* p : {(void*)data, (void*)off_dev, (void*)len_dev, (void*)onset_dev})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
}

int bank_check(const Bank& bk, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows) {
  VP_REQUIRE(rows && label_rows, "bank batch: null rows or label_rows");
  VP_REQUIRE(B >= 1, "bank batch: B = %d", B);
  VP_REQUIRE(T >= 1 && T <= GEN_MAX_T, "bank batch: T = %d outside [1, %d]", T, GEN_MAX_T);
  VP_REQUIRE(std::isfinite(sigma) && sigma > 0.f, "bank batch: sigma = %g must be finite and > 0", (double)sigma);
  VP_REQUIRE(norm == VP_NORM_PEAK || norm == VP_NORM_STD, "bank batch: norm %d is neither VP_NORM_PEAK nor VP_NORM_STD", norm);
  int seen = 0;
  for (int i = 0; i < 3; ++i) {
    VP_REQUIRE(label_rows[i] >= 0 && label_rows[i] < 3, "bank batch: label_rows[%d] = %d outside [0, 3)", i, label_rows[i]);
    seen |= 1 << label_rows[i];
  }
  VP_REQUIRE(seen == 7, "bank batch: label_rows is not a permutation of 0, 1, 2");
  for (int b = 0; b < B; ++b) {
    const vp_plan_row& r = rows[b];
    VP_REQUIRE(r.trace >= 0 && r.trace < bk.n_written, "bank batch: row %d: trace %d outside [0, %lld)", b, (int)r.trace,
               bk.n_written);
    const long long L = bk.len[r.trace];
    VP_REQUIRE(r.lo >= 0 && r.lo <= r.hi && r.hi <= L, "bank batch: row %d: [lo, hi) = [%lld, %lld) outside [0, %lld]", b,
               (long long)r.lo, (long long)r.hi, L);
    // start + t must not overflow for t < T (the kernel's index arithmetic)
    VP_REQUIRE(r.start > -(1LL << 62) && r.start < (1LL << 62), "bank batch: row %d: start %lld out of range", b,
               (long long)r.start);
  }
  return VP_OK;
}

int bank_launch(const Bank& bk, const vp_plan_row* rows_dev, int B, int T, float sigma, int norm, const int* label_rows,
                float* x, float* y, hipStream_t s) {
  GenArgs a{};
  a.data = bk.data;
  a.off = bk.off_dev;
  a.len = bk.len_dev;
  a.onset = bk.onset_dev;
  a.rows = rows_dev;
  a.x = x;
  a.y = y;
  a.T = T;
  a.norm = norm;
  a.sigma = sigma;
  a.row_p = label_rows[0];
  a.row_s = label_rows[1];
  a.row_n = label_rows[2];
  hipLaunchKernelGGL(bank_batch_kernel, dim3(B), dim3(GEN_NTH), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("bank_batch_kernel launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp

using namespace vp;

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
  for (hipEvent_t& e : bk->ev) VP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
  bk.n_written += n_traces;
  bk.floats_written += floats;
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
  VP_REQUIRE(h && x && y, "vp_bank_make_batch: null argument");
  Bank& bk = *reinterpret_cast<Bank*>(h);
  const int rc = bank_check(bk, rows, B, T, sigma, norm, label_rows);
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(bk.device));
  const int slot = (int)(bk.batches % RowRing::N);
  if (B > bk.ring.cap) {  // every slot idle before the ring is reallocated
    for (int i = 0; i < RowRing::N; ++i)
      if (bk.ev_used[i]) VP_HIP(hipEventSynchronize(bk.ev[i]));
    const int r = bk.ring.reserve(B);
    if (r != VP_OK) return r;
  } else if (bk.ev_used[slot]) {
    VP_HIP(hipEventSynchronize(bk.ev[slot]));  // the kernel that read this slot last (and so the copy into it) has run
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const vp_plan_row* rd = bk.ring.stage(slot, rows, B, s);
  if (!rd) return VP_ERR_HIP;
  const int r = bank_launch(bk, rd, B, T, sigma, norm, label_rows, x, y, s);
  if (r != VP_OK) return r;
  VP_HIP(hipEventRecord(bk.ev[slot], s));
  bk.ev_used[slot] = true;
  ++bk.batches;
  return VP_OK;
}

}  // extern "C"
