// Frequency index and signal-to-noise ratio of picks and bank traces, on the device (include/volpick_hip.h,
// vp_attributes / vp_bank_attributes): what the reference stores with every trace it writes (trace_frequency_index,
// trace_snr_db, trace_mean_snr_db).  The rule is restated in tests/attributes_f64.py; the host plans everything that
// depends on lengths alone (volpick_amd/attributes.py: the windows, the first bin and bin count of each band from
// fftfreq's own float64 values, the percentile's two indices and weight), so the device never re-derives a comparison
// that decides a bin or an index.
//
// Three kernels, everything float64, no atomics, every sum in a fixed order (results are identical from run to run):
//
//   flat_partial_kernel / flat_final_kernel   sum |diff(x)| over each WHOLE component of every trace the rows name (the
//       reference's dead-component test is a property of the trace, not of the window): blocks of FLAT_CHUNK samples,
//       then one thread per component adds the blocks' sums in order.
//   attributes_kernel   one workgroup of 256 threads per row.
//       demean (a row flag): per component the mean over the span from the row's earliest window start to its latest
//           window end, subtracted before both computations below.
//       frequency index: the three components' windowed samples (symmetric Hann) and the n unit roots exp(-2 pi i r / n)
//           (sincospi of 2 r / n, r an integer below n) are staged in LDS.  A thread owns one (component, bin) pair and
//           walks j with r = (r + k) mod n in integers -- x[j] is an LDS broadcast, the root a per-lane read.  Only the
//           planned bins are evaluated (61 of 350 at the default 700-sample window), so no FFT: 61 x 700 fused
//           multiply-adds per component.  Magnitudes go to LDS, six threads take the band means in bin order, then log10,
//           the skip rules and the mean over the remaining components.
//       percentiles: |x| of a window staged in LDS for the three components; a thread counts the elements smaller than
//           its own (ties broken by index), the two threads whose ranks are the planned indices publish their values, and
//           the interpolation follows numpy's operation order with contraction off.  A NaN in a window makes that
//           window's percentile NaN.
//
// LDS: 3 nmax doubles (samples) + nmax complex doubles (roots) + 3 nbmax doubles (magnitudes), nmax / nbmax the row set's
// largest window / bin count: 29 KB at the defaults (five workgroups per CU), 80 KB + magnitudes at the cap of 2048.
#include <algorithm>
#include <cmath>

#include "batchgen.h"
#include "device_scratch.h"

namespace vp {
namespace {

constexpr int AT = 256;               // threads per workgroup
constexpr int ANW = AT / 64;          // waves
constexpr int ATTR_MAX_N = 2048;      // longest window of either kind
constexpr int FLAT_CHUNK = 16384;     // samples per block of the dead-component pass
constexpr int ATTR_OUT = 14;          // doubles per row

typedef double2 cd;

struct AttrArgs {
  const float* data;
  const long long* off;  // per trace (bank); NULL: one trace at data, n_samples long
  const long long* len;
  long long n_samples;
  const vp_attr_row* rows;
  const int* row_unit;   // row -> index into flat
  const double* flat;    // [unit][3]: sum |diff| over the whole component
  double* out;           // [row][14]
  int nmax, nbmax;       // LDS layout (nmax even)
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sum of v over the workgroup, the waves' sums added in wave order.  red: [ANW] doubles; two barriers.
__device__ __forceinline__ double block_sum(double v, double* red, const int tid) {
  const double ws = wave_sum(v);
  __syncthreads();  // the previous call's readers are done
  if ((tid & 63) == 0) red[tid >> 6] = ws;
  __syncthreads();
  double acc = red[0];
#pragma unroll
  for (int i = 1; i < ANW; ++i) acc += red[i];
  return acc;
}

__global__ __launch_bounds__(AT) void flat_partial_kernel(const float* __restrict__ data, const long long* __restrict__ off,
                                                          const long long* __restrict__ len, const long long n_samples,
                                                          const int* __restrict__ units, double* __restrict__ partial) {
  __shared__ double red[ANW];
  const int u = blockIdx.x / 3, c = blockIdx.x % 3, tid = threadIdx.x;
  const int trace = units[u];
  const long long L = len ? len[trace] : n_samples;
  const float* x = data + (off ? off[trace] : 0) + c * L;
  const long long i0 = (long long)blockIdx.y * FLAT_CHUNK;
  const long long i1 = i0 + FLAT_CHUNK < L - 1 ? i0 + FLAT_CHUNK : L - 1;  // differences i0 .. i1 - 1 read x[i], x[i + 1]
  double s = 0.0;
  for (long long i = i0 + tid; i < i1; i += AT) s += fabs((double)x[i + 1] - (double)x[i]);
  s = block_sum(s, red, tid);
  if (tid == 0) partial[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = s;
}

__global__ __launch_bounds__(AT) void flat_final_kernel(const double* __restrict__ partial, const int chunks, const int n,
                                                        double* __restrict__ flat) {
  const int i = blockIdx.x * AT + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += partial[(size_t)i * chunks + k];
  flat[i] = s;
}

// numpy's _lerp: a + (b - a) g, replaced by b - (b - a) (1 - g) where g >= 0.5; no fused multiply-add
__device__ __forceinline__ double lerp_np(const double a, const double b, const double g) {
#pragma clang fp contract(off)
  const double d = b - a;
  const double lo = a + d * g;
  const double hi = b - d * (1.0 - g);
  return g >= 0.5 ? hi : lo;
}

// The planned percentile of |x - mean| over samples [start, start + m) of the three components.  sel: [3][2] doubles,
// nanflag: [3] ints (static LDS).  Uniform control flow: every thread of the workgroup calls it with the same arguments.
__device__ __forceinline__ void percentile3(const float* __restrict__ src, const long long L, const long long start, const int m,
                                            const int ilo, const int iup, const double g, const double mean[3],
                                            double* xw, const int nmax, double (*sel)[2], int* nanflag, const int tid,
                                            double out[3]) {
  const double nan = __builtin_nan("");
  if (m <= 0) {
    out[0] = out[1] = out[2] = nan;
    return;
  }
  __syncthreads();  // whoever used xw / sel before is done
  if (tid < 3) {
    nanflag[tid] = 0;
    sel[tid][0] = sel[tid][1] = nan;
  }
  for (int j = tid; j < m; j += AT)
#pragma unroll
    for (int c = 0; c < 3; ++c) xw[c * nmax + j] = fabs((double)src[c * L + start + j] - mean[c]);
  __syncthreads();
  for (int e = tid; e < 3 * m; e += AT) {
    const int c = e / m, j = e - c * m;
    const double* x = xw + c * nmax;
    const double v = x[j];
    if (v != v) {
      nanflag[c] = 1;  // every writer writes the same word
      continue;
    }
    int rank = 0;
    for (int i = 0; i < m; ++i) {
      const double u = x[i];
      rank += (u < v) | ((u == v) & (i < j));
    }
    if (rank == ilo) sel[c][0] = v;
    if (rank == iup) sel[c][1] = v;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = nanflag[c] ? nan : lerp_np(sel[c][0], sel[c][1], g);
}

__global__ __launch_bounds__(AT) void attributes_kernel(const AttrArgs a) {
  extern __shared__ double at_lds[];
  __shared__ double red[ANW];
  __shared__ double sel[3][2];
  __shared__ double band[3][2];
  __shared__ int nanflag[3];
  const int tid = threadIdx.x, nmax = a.nmax, nbmax = a.nbmax;
  double* xw = at_lds;                               // [3][nmax]
  cd* roots = reinterpret_cast<cd*>(at_lds + 3 * nmax);  // [nmax]
  double* mag = at_lds + 5 * nmax;                   // [3][nbmax]
  const vp_attr_row r = a.rows[blockIdx.x];
  const long long L = a.len ? a.len[r.trace] : a.n_samples;
  const float* src = a.data + (a.off ? a.off[r.trace] : 0);
  const double nan = __builtin_nan("");

  // ---- demean: the span of the row's windows
  double mean[3] = {0.0, 0.0, 0.0};
  if (r.flags & VP_ATTR_DEMEAN) {
    long long lo = L, hi = 0;
    if (r.fi_n > 0) lo = min(lo, (long long)r.fi_start), hi = max(hi, (long long)r.fi_start + r.fi_n);
    if (r.noise_n > 0) lo = min(lo, (long long)r.noise_start), hi = max(hi, (long long)r.noise_start + r.noise_n);
    if (r.signal_n > 0) lo = min(lo, (long long)r.signal_start), hi = max(hi, (long long)r.signal_start + r.signal_n);
    if (hi > lo) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (long long i = lo + tid; i < hi; i += AT) s += (double)src[c * L + i];
        mean[c] = block_sum(s, red, tid) / (double)(hi - lo);
      }
    }
  }

  // ---- frequency index
  double fi[3] = {nan, nan, nan};
  const int n = r.fi_n, nb = r.lo_count + r.hi_count;
  if (n > 0 && r.lo_count > 0 && r.hi_count > 0) {
    for (int j = tid; j < n; j += AT) {
      double w = 1.0;  // scipy's hann(1) is [1.0]
      if (n > 1) {
        const double sj = sinpi((double)j / (double)(n - 1));
        w = sj * sj;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) xw[c * nmax + j] = ((double)src[c * L + r.fi_start + j] - mean[c]) * w;
      double s, co;
      sincospi((double)(2 * j) / (double)n, &s, &co);
      roots[j] = make_double2(co, -s);
    }
    __syncthreads();
    for (int pr = tid; pr < 3 * nb; pr += AT) {
      const int c = pr / nb, b = pr - c * nb;
      const int k = b < r.lo_count ? r.lo_first + b : r.hi_first + (b - r.lo_count);
      const double* x = xw + c * nmax;
      double re = 0.0, im = 0.0;
      int rr = 0;
      for (int j = 0; j < n; ++j) {
        const cd w = roots[rr];
        const double v = x[j];
        re = fma(v, w.x, re);
        im = fma(v, w.y, im);
        rr += k;  // k < n
        if (rr >= n) rr -= n;
      }
      mag[c * nbmax + b] = hypot(re, im);
    }
    __syncthreads();
    if (tid < 6) {
      const int c = tid >> 1, up = tid & 1;
      const int first = up ? r.lo_count : 0, cnt = up ? r.hi_count : r.lo_count;
      double s = 0.0;
      for (int b = 0; b < cnt; ++b) s += mag[c * nbmax + first + b];
      band[c][up] = s / (double)cnt;
    }
    __syncthreads();
    const double* fl = a.flat + 3 * a.row_unit[blockIdx.x];
#pragma unroll
    for (int c = 0; c < 3; ++c) fi[c] = fl[c] <= 1e-9 ? nan : log10(band[c][1] / band[c][0]);  // a NaN sum does not skip
  }
  double fi_sum = 0.0;
  int fi_cnt = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (fi[c] == fi[c]) fi_sum += fi[c], ++fi_cnt;
  const double fi_trace = fi_cnt ? fi_sum / (double)fi_cnt : nan;

  // ---- percentiles and signal-to-noise ratio
  double noi[3], sig[3], snr[3];
  percentile3(src, L, r.noise_start, r.noise_n, r.noise_lo, r.noise_up, r.noise_g, mean, xw, nmax, sel, nanflag, tid, noi);
  percentile3(src, L, r.signal_start, r.signal_n, r.signal_lo, r.signal_up, r.signal_g, mean, xw, nmax, sel, nanflag, tid,
              sig);
  double snr_sum = 0.0;
  int snr_cnt = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    snr[c] = (fabs(noi[c]) <= 1e-8 || fabs(sig[c]) <= 1e-8) ? nan : 20.0 * log10(sig[c] / noi[c]);  // np.isclose(v, 0)
    if (snr[c] == snr[c]) snr_sum += snr[c], ++snr_cnt;
  }
  if (tid == 0) {
    double* o = a.out + (size_t)blockIdx.x * ATTR_OUT;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = fi[c];
      o[4 + c] = noi[c];
      o[7 + c] = sig[c];
      o[10 + c] = snr[c];
    }
    o[3] = fi_trace;
    o[13] = snr_cnt ? snr_sum / (double)snr_cnt : nan;
  }
}

// Per device, grow-only, reused from call to call: the staged rows, the dead-component sums and, for a host `out`, the
// result.
DeviceScratch<1>& attr_scratch(int device) {
  static DeviceScratch<1> pool[64];
  return pool[(unsigned)device % 64];
}

int check_window(const char* who, int i, const char* what, long long start, int n, long long L) {
  VP_REQUIRE(n >= 0 && n <= ATTR_MAX_N, "%s: row %d: %s window of %d samples, the kernel takes 0..%d", who, i, what, n,
             ATTR_MAX_N);
  VP_REQUIRE(n == 0 || (start >= 0 && start <= L - n), "%s: row %d: %s window [%lld, %lld) outside the trace's %lld samples", who,
             i, what, start, start + n, L);
  return VP_OK;
}

int check_percentile(const char* who, int i, const char* what, int m, int lo, int up, double g) {
  if (m == 0) return VP_OK;
  VP_REQUIRE(lo >= 0 && lo <= up && up <= lo + 1 && up < m, "%s: row %d: %s percentile indices %d, %d of %d samples", who, i, what,
             lo, up, m);
  VP_REQUIRE(g >= 0.0 && g <= 1.0, "%s: row %d: %s percentile weight %g outside [0, 1]", who, i, what, g);
  return VP_OK;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// data / off / len: device.  host_len: the traces' lengths on the host (bank), or NULL with n_samples for one trace.
int run_attributes(const char* who, int device, const float* data, const long long* off, const long long* len,
                   const std::vector<long long>* host_len, long long n_samples, const vp_attr_row* rows, int n_rows,
                   double* out, hipStream_t s) {
  VP_REQUIRE(data && rows && out, "%s: null argument", who);
  VP_REQUIRE(n_rows >= 1, "%s: n_rows = %d, need at least one row", who, n_rows);
  VP_REQUIRE(device >= 0, "%s: device index", who);
  int nmax = 2, nbmax = 1;
  long long longest = 0;
  std::vector<int> units;
  units.reserve((size_t)n_rows);
  for (int i = 0; i < n_rows; ++i) {
    const vp_attr_row& r = rows[i];
    long long L = n_samples;
    if (host_len) {
      VP_REQUIRE(r.trace >= 0 && (size_t)r.trace < host_len->size(), "%s: row %d: trace %d, the bank holds %zu", who, i,
                 (int)r.trace, host_len->size());
      L = (*host_len)[(size_t)r.trace];
    } else {
      VP_REQUIRE(r.trace == 0, "%s: row %d: trace %d, a single array is trace 0", who, i, (int)r.trace);
    }
    VP_REQUIRE((r.flags & ~VP_ATTR_DEMEAN) == 0, "%s: row %d: flags %d", who, i, (int)r.flags);
    int rc;
    if ((rc = check_window(who, i, "frequency-index", r.fi_start, r.fi_n, L)) != VP_OK) return rc;
    if ((rc = check_window(who, i, "noise", r.noise_start, r.noise_n, L)) != VP_OK) return rc;
    if ((rc = check_window(who, i, "signal", r.signal_start, r.signal_n, L)) != VP_OK) return rc;
    const int half = r.fi_n / 2;
    VP_REQUIRE(r.lo_count >= 0 && r.lo_first >= 0 && r.lo_first <= half - r.lo_count, "%s: row %d: low band bins [%d, +%d) of %d",
               who, i, (int)r.lo_first, (int)r.lo_count, half);
    VP_REQUIRE(r.hi_count >= 0 && r.hi_first >= 0 && r.hi_first <= half - r.hi_count, "%s: row %d: high band bins [%d, +%d) of %d",
               who, i, (int)r.hi_first, (int)r.hi_count, half);
    if ((rc = check_percentile(who, i, "noise", r.noise_n, r.noise_lo, r.noise_up, r.noise_g)) != VP_OK) return rc;
    if ((rc = check_percentile(who, i, "signal", r.signal_n, r.signal_lo, r.signal_up, r.signal_g)) != VP_OK) return rc;
    nmax = std::max(nmax, std::max((int)r.fi_n, std::max((int)r.noise_n, (int)r.signal_n)));
    nbmax = std::max(nbmax, (int)(r.lo_count + r.hi_count));
    longest = std::max(longest, L);
    units.push_back((int)r.trace);
  }
  nmax += nmax & 1;  // the roots behind 3 nmax doubles stay 16-byte aligned
  // the traces the rows name, each once
  std::vector<int> uniq(units);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (int& u : units) u = (int)(std::lower_bound(uniq.begin(), uniq.end(), u) - uniq.begin());
  const int n_units = (int)uniq.size();
  const long long chunks_ll = std::max(1LL, (longest - 1 + FLAT_CHUNK - 1) / FLAT_CHUNK);
  VP_REQUIRE(chunks_ll <= 65535, "%s: a trace of %lld samples is beyond the dead-component pass (%d x 65535)", who, longest,
             FLAT_CHUNK);
  const int chunks = (int)chunks_ll;

  VP_HIP(hipSetDevice(device));
  bool out_on_device = false;
  hipPointerAttribute_t pa;
  if (hipPointerGetAttributes(&pa, out) == hipSuccess)
    out_on_device = pa.type == hipMemoryTypeDevice || pa.type == hipMemoryTypeManaged;
  else
    (void)hipGetLastError();  // plain host memory the runtime has never seen

  const size_t lds = ((size_t)5 * nmax + (size_t)3 * nbmax) * sizeof(double);
  VP_HIP(hipFuncSetAttribute((const void*)attributes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

  DeviceScratch<1>& sc = attr_scratch(device);
  std::lock_guard<std::mutex> lock(sc.mu);
  const size_t b_rows = align256((size_t)n_rows * sizeof(vp_attr_row)), b_ru = align256((size_t)n_rows * sizeof(int));
  const size_t b_un = align256((size_t)n_units * sizeof(int));
  const size_t b_part = align256((size_t)n_units * 3 * chunks * sizeof(double));
  const size_t b_flat = align256((size_t)n_units * 3 * sizeof(double));
  const size_t b_out = out_on_device ? 0 : align256((size_t)n_rows * ATTR_OUT * sizeof(double));
  const size_t bytes = b_rows + b_ru + b_un + b_part + b_flat + b_out;
  void* p = nullptr;
  if (const int rc = sc.b[0].grow(who, bytes, bytes / 8 + 4096, &p)) return rc;
  char* q = (char*)p;
  vp_attr_row* rows_dev = (vp_attr_row*)q;
  int* ru_dev = (int*)(q += b_rows);
  int* un_dev = (int*)(q += b_ru);
  double* part_dev = (double*)(q += b_un);
  double* flat_dev = (double*)(q += b_part);
  double* out_dev = out_on_device ? out : (double*)(q += b_flat);

  // pageable sources: each copy has left the host buffers when the call returns
  VP_HIP(hipMemcpyAsync(rows_dev, rows, (size_t)n_rows * sizeof(vp_attr_row), hipMemcpyHostToDevice, s));
  VP_HIP(hipMemcpyAsync(ru_dev, units.data(), (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice, s));
  VP_HIP(hipMemcpyAsync(un_dev, uniq.data(), (size_t)n_units * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(flat_partial_kernel, dim3((unsigned)(3 * n_units), (unsigned)chunks), dim3(AT), 0, s, data, off, len,
                     n_samples, un_dev, part_dev);
  VP_HIP(hipGetLastError());
  hipLaunchKernelGGL(flat_final_kernel, dim3((unsigned)((3 * n_units + AT - 1) / AT)), dim3(AT), 0, s, part_dev, chunks,
                     3 * n_units, flat_dev);
  VP_HIP(hipGetLastError());
  AttrArgs a;
  a.data = data;
  a.off = off;
  a.len = len;
  a.n_samples = n_samples;
  a.rows = rows_dev;
  a.row_unit = ru_dev;
  a.flat = flat_dev;
  a.out = out_dev;
  a.nmax = nmax;
  a.nbmax = nbmax;
  hipLaunchKernelGGL(attributes_kernel, dim3((unsigned)n_rows), dim3(AT), lds, s, a);
  VP_HIP(hipGetLastError());
  if (!out_on_device)
    VP_HIP(hipMemcpyAsync(out, out_dev, (size_t)n_rows * ATTR_OUT * sizeof(double), hipMemcpyDeviceToHost, s));
  VP_HIP(hipStreamSynchronize(s));  // the scratch is free for the next call, `out` is complete
  return VP_OK;
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_attributes(int device_id, const float* data, int64_t n_samples, const vp_attr_row* rows, int n_rows,
                             double* out, void* stream) {
  VP_REQUIRE(n_samples >= 1 && n_samples <= (int64_t)1 << 40, "vp_attributes: n_samples = %lld", (long long)n_samples);
  return run_attributes("vp_attributes", device_id, data, nullptr, nullptr, nullptr, (long long)n_samples, rows, n_rows, out,
                        reinterpret_cast<hipStream_t>(stream));
}

extern "C" int vp_bank_attributes(vp_bank* h, const vp_attr_row* rows, int n_rows, double* out, void* stream) {
  VP_REQUIRE(h, "vp_bank_attributes: null bank");
  const Bank& bk = *reinterpret_cast<Bank*>(h);
  return run_attributes("vp_bank_attributes", bk.device, bk.data, bk.off_dev, bk.len_dev, &bk.len, 0, rows, n_rows, out,
                        reinterpret_cast<hipStream_t>(stream));
}
