// Spectrograms of device-resident series (include/volpick_hip.h, vp_spectrogram): the numeric content of the reference's
// spectrogram() (volpick/data/utils.py:1251-1440) up to the point where it starts to draw -- matplotlib.mlab.specgram of the
// demeaned series with a symmetric Hann window of nfft samples, zero-padded to pad, bins 1 .. pad / 2, then sqrt or
// 10 log10.  The rule is restated in tests/spectrogram_f64.py; the host plans everything that depends on lengths alone
// (volpick_amd/spectrogram.py: nfft, pad, hop, the frame count, both axes).
//
// The one named deviation: for float32 input the reference's own data.mean() accumulates in float32; the mean here is a
// float64 sum whatever the input kind.
//
// Everything float64, no atomics, every sum in a fixed order (results are identical from run to run, and a frame range equals
// the same columns of the full result bit for bit: a column depends on the series' mean and its own samples only).
//
//   mean_partial_kernel / mean_final_kernel   the mean over each WHOLE series: blocks of MEAN_CHUNK samples, then one wave per
//       series adds the blocks' sums in a fixed order.
//   spec_table_kernel   the tables every workgroup reads: for the residues r = 0 .. ratio / 2 (ratio = pad / nfft) the
//       twisted window w[n] exp(-2 pi i r n / pad), then the nfft / 2 unit roots exp(-2 pi i j / nfft) -- sincospi of exact
//       integer ratios.
//   spectrogram_kernel   one workgroup of 512 threads per tile of jp = min(32, 4096 / nfft) consecutive frames of one series.
//       Their hop (jp - 1) + nfft contiguous samples are staged in LDS once, minus the mean (at 90 % overlap every sample
//       is read by ten frames).  Only nfft of a frame's pad inputs are non-zero, so the first log2(ratio) stages of the
//       pad-point transform collapse: bins k = ratio m + r are the nfft-point transform of x[n] w[n] exp(-2 pi i r n / pad).
//       The input is real, so residue ratio - r is the mirror of residue r: ratio / 2 + 1 transforms per frame instead of
//       ratio (5 instead of 8 at the defaults), every output of the inner residues used.  Per residue: the tile's frames are
//       transformed in an LDS image (jp rows of nfft + 1 complex) by decimation in frequency -- three radix-2 stages per
//       pass through LDS, fused in registers (two where four or two stages remain: 3 + 2 + 2 at nfft 128), the first pass
//       reading the staged samples times the twisted window; a row's columns are permuted (swz) so that the late passes
//       spread over all LDS banks -- and read back transposed (bit-reversed position, consecutive lanes on consecutive
//       frames), so that a frequency row's stores run along the time axis: jp contiguous floats per row and tile.
//
// LDS per workgroup: the samples, the tables and the image -- 80 KB at the defaults (nfft 128, pad 1024, hop 13), 140 KB at
// the corner nfft 512, pad 4096, hop 512.
#include <cmath>

#include "device_scratch.h"
#include "spectrogram_host.h"

namespace vp {
namespace {

constexpr int ST = 512;            // threads per workgroup
constexpr int SNW = ST / 64;       // waves
constexpr int MEAN_CHUNK = 16384;  // samples per block of the mean pass

typedef double2 cd;

struct SpecArgs {
  const void* in;
  long long stride;     // samples from one series to the next
  const double* mean;   // [series]
  const cd* tables;     // nres * nfft twisted windows, nfft / 2 unit roots
  float* out;           // [series][pad / 2][count]
  double scale;
  long long first, count;  // the frame range
  int nfft, lg, pad, ratio, nres, hop, jp, lgjp, xs_cap, dbscale;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__global__ __launch_bounds__(ST) void mean_partial_kernel(const T* __restrict__ in, const long long stride, const long long n,
                                                          const int chunks, double* __restrict__ partial) {
  __shared__ double red[SNW];
  const int tid = threadIdx.x;
  const T* x = in + (size_t)blockIdx.y * stride;
  const long long i0 = (long long)blockIdx.x * MEAN_CHUNK;
  const long long i1 = i0 + MEAN_CHUNK < n ? i0 + MEAN_CHUNK : n;
  double s = 0.0;
  for (long long i = i0 + tid; i < i1; i += ST) s += (double)x[i];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double acc = red[0];
#pragma unroll
    for (int i = 1; i < SNW; ++i) acc += red[i];
    partial[(size_t)blockIdx.y * chunks + blockIdx.x] = acc;
  }
}

// One wave per series.
__global__ __launch_bounds__(64) void mean_final_kernel(const double* __restrict__ partial, const int chunks, const long long n,
                                                        double* __restrict__ mean) {
  const double* p = partial + (size_t)blockIdx.x * chunks;
  double s = 0.0;
  for (int k = threadIdx.x; k < chunks; k += 64) s += p[k];
  s = wave_sum(s);
  if (threadIdx.x == 0) mean[blockIdx.x] = s / (double)n;
}

__global__ __launch_bounds__(256) void spec_table_kernel(const int nfft, const int pad, const int nres, cd* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nt = nres * nfft;
  double s, c;
  if (i < nt) {
    const int r = i / nfft, n = i - r * nfft;
    const double h = sinpi((double)n / (double)(nfft - 1));  // np.hanning: 0.5 - 0.5 cos(2 pi n / (nfft - 1)) = sin^2(pi n / (nfft - 1))
    const double w = h * h;
    sincospi((double)(2 * ((r * n) % pad)) / (double)pad, &s, &c);
    tab[i] = make_double2(w * c, -(w * s));
  } else if (i < nt + nfft / 2) {
    sincospi((double)(2 * (i - nt)) / (double)nfft, &s, &c);
    tab[i] = make_double2(c, -s);
  }
}

__device__ __forceinline__ cd cadd(const cd a, const cd b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cd csub(const cd a, const cd b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cd cmul(const cd a, const cd b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// Where element `pos` of a frame's row lies in the image: bits 0-3 flipped by bits 4-5.  In the late passes a thread's
// elements are 4 or 16 apart and neighbouring lanes 16 or 4, so the 16 lanes of a 16-byte access would meet on 4 of the 16
// bank quads; with the flip they cover all 16.
__device__ __forceinline__ int swz(const int pos) { return pos ^ (((pos >> 4) & 3) * 5); }

// K stages of every frame's decimation-in-frequency transform in one pass through LDS: blocks of len = 2^lglen, a thread
// holds the 2^K elements i + u q (q = len / 2^K) of one block in registers.  Stage s pairs u with u + h (h = 2^(K - 1 - s)),
// inside sub-blocks of len / 2^s, with the root W_(len / 2^s)^(i + (u mod h) q).  tw != NULL: the first pass (len = nfft), which
// reads frame j as xs[j hop + n] tw[n] instead of the image.
template <int K>
__device__ __forceinline__ void fused_pass(cd* __restrict__ buf, const int bs, const double* __restrict__ xs, const int hop,
                                           const cd* __restrict__ tw, const cd* __restrict__ roots, const int nf, const int lg,
                                           const int lglen, const int tid) {
  constexpr int E = 1 << K;
  const int lgq = lglen - K, q = 1 << lgq;
  for (int e = tid; e < (nf << (lg - K)); e += ST) {
    const int j = e >> (lg - K), t = e & ((1 << (lg - K)) - 1);
    const int blk = t >> lgq, i = t & (q - 1);
    cd* row = buf + j * bs;
    const int pos = (blk << lglen) + i;
    cd v[E];
    if (tw) {
      const double* x = xs + j * hop + i;
#pragma unroll
      for (int u = 0; u < E; ++u) {
        const double xv = x[u << lgq];
        const cd w = tw[i + (u << lgq)];
        v[u] = make_double2(xv * w.x, xv * w.y);
      }
    } else {
#pragma unroll
      for (int u = 0; u < E; ++u) v[u] = row[swz(pos + (u << lgq))];
    }
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const int h = 1 << (K - 1 - s);
#pragma unroll
      for (int u = 0; u < E; ++u) {
        if (u & h) continue;
        const cd w = roots[(i + ((u & (h - 1)) << lgq)) << (lg - lglen + s)];
        const cd x0 = v[u], x1 = v[u + h];
        v[u] = cadd(x0, x1);
        v[u + h] = cmul(csub(x0, x1), w);
      }
    }
#pragma unroll
    for (int u = 0; u < E; ++u) row[swz(pos + (u << lgq))] = v[u];
  }
}

template <typename T>
__global__ __launch_bounds__(ST) void spectrogram_kernel(const SpecArgs a) {
  extern __shared__ double sp_lds[];
  const int tid = threadIdx.x;
  const int nfft = a.nfft, lg = a.lg, pad = a.pad, ratio = a.ratio, hop = a.hop, jp = a.jp;
  const int bs = nfft + 1;  // a frame's row in the image: the odd stride spreads the transposed read over the banks
  double* xs = sp_lds;                                    // [xs_cap]
  cd* twist = reinterpret_cast<cd*>(sp_lds + a.xs_cap);   // [nres][nfft]
  cd* roots = twist + a.nres * nfft;                      // [nfft / 2]
  cd* buf = roots + nfft / 2;                             // [jp][bs]

  const long long tile0 = (long long)blockIdx.x * jp;     // the tile's first frame within the range
  const int nf = (int)(a.count - tile0 < (long long)jp ? a.count - tile0 : (long long)jp);
  const int ns = (nf - 1) * hop + nfft;
  const T* src = (const T*)a.in + (size_t)blockIdx.y * a.stride + (a.first + tile0) * hop;
  const double mean = a.mean[blockIdx.y];
  const bool finite = fabs(mean) <= 1.7976931348623157e308;  // false for NaN and Inf: the whole series is NaN then
  const double nan = __builtin_nan("");
  for (int i = tid; i < ns; i += ST) xs[i] = finite ? (double)src[i] - mean : nan;
  const int nt = a.nres * nfft + nfft / 2;
  for (int i = tid; i < nt; i += ST) twist[i] = a.tables[i];
  __syncthreads();

  float* out = a.out + (size_t)blockIdx.y * (size_t)(pad / 2) * (size_t)a.count + (size_t)tile0;
  const double scale2 = 2.0 * a.scale;
  for (int r = 0; r < a.nres; ++r) {
    // ---- nfft-point transforms in place, decimation in frequency: X[m] ends at position bitrev(m).  The first pass reads
    // the frames from the samples, windowed and twisted, and writes the image; passes of three stages, two where four or two
    // stages remain.
    const cd* tw = twist + r * nfft;
    for (int lglen = lg; lglen > 0;) {
      const bool first = lglen == lg;
      if (lglen == 4 || lglen == 2) {
        fused_pass<2>(buf, bs, xs, hop, first ? tw : nullptr, roots, nf, lg, lglen, tid);
        lglen -= 2;
      } else {
        fused_pass<3>(buf, bs, xs, hop, first ? tw : nullptr, roots, nf, lg, lglen, tid);
        lglen -= 3;
      }
      __syncthreads();
    }
    // ---- bins ratio m + r (and their mirrors pad - k for the inner residues), consecutive lanes on consecutive frames
    for (int e = tid; e < (nfft << a.lgjp); e += ST) {
      const int fr = e & (jp - 1), m = e >> a.lgjp;
      if (fr >= nf) continue;
      const int k = ratio * m + r;
      const bool mirror = k > pad / 2;
      const int kk = mirror ? pad - k : k;
      if (kk < 1 || (mirror && (r == 0 || 2 * r == ratio))) continue;  // bin 0; residues that mirror onto themselves
      const cd v = buf[fr * bs + swz((int)(__brev((unsigned)m) >> (32 - lg)))];
      const double p = (v.x * v.x + v.y * v.y) * (kk == pad / 2 ? a.scale : scale2);
      out[(size_t)(kk - 1) * (size_t)a.count + fr] = a.dbscale ? (float)(10.0 * log10(p)) : (float)sqrt(p);
    }
    __syncthreads();  // the image is free for the next residue
  }
}

// Per device, grow-only, reused from call to call: the series' means, the mean pass's partial sums, the tables.
DeviceScratch<1>& spec_scratch(int device) {
  static DeviceScratch<1> pool[64];
  return pool[(unsigned)device % 64];
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// Where a call's arrays lie in the scratch.
struct Layout {
  int chunks;
  size_t b_mean, b_part, b_tab;
  double *mean = nullptr, *part = nullptr;
  cd* tab = nullptr;
  Layout(const SpecPlan& p, int n_series, long long n) {
    chunks = (int)((n + MEAN_CHUNK - 1) / MEAN_CHUNK);  // n <= 2^40
    b_mean = align256((size_t)n_series * sizeof(double));
    b_part = align256((size_t)n_series * chunks * sizeof(double));
    b_tab = align256(p.table_elems * sizeof(cd));
  }
  size_t bytes() const { return b_mean + b_part + b_tab; }
  void place(void* base) {
    char* q = (char*)base;
    mean = (double*)q;
    part = (double*)(q += b_mean);
    tab = (cd*)(q += b_part);
  }
};

struct Call {
  const void* in;
  int in_kind, n_series;
  long long stride, n, first, count;
  int dbscale;
  float* out;
};

template <typename T>
hipError_t launch_means_t(const Call& c, const Layout& L, hipStream_t s) {
  hipLaunchKernelGGL(mean_partial_kernel<T>, dim3((unsigned)L.chunks, (unsigned)c.n_series), dim3(ST), 0, s, (const T*)c.in,
                     c.stride, c.n, L.chunks, L.part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mean_final_kernel, dim3((unsigned)c.n_series), dim3(64), 0, s, L.part, L.chunks, c.n, L.mean);
  return hipGetLastError();
}

hipError_t launch_means(const Call& c, const Layout& L, hipStream_t s) {
  if (c.in_kind == VP_SAMPLES_INT32) return launch_means_t<int>(c, L, s);
  if (c.in_kind == VP_SAMPLES_FLOAT32) return launch_means_t<float>(c, L, s);
  return launch_means_t<double>(c, L, s);
}

hipError_t launch_tables(const SpecPlan& p, const Layout& L, hipStream_t s) {
  hipLaunchKernelGGL(spec_table_kernel, dim3((unsigned)((p.table_elems + 255) / 256)), dim3(256), 0, s, p.nfft, p.pad, p.nres,
                     L.tab);
  return hipGetLastError();
}

const void* frame_kernel(int in_kind) {
  if (in_kind == VP_SAMPLES_INT32) return (const void*)spectrogram_kernel<int>;
  if (in_kind == VP_SAMPLES_FLOAT32) return (const void*)spectrogram_kernel<float>;
  return (const void*)spectrogram_kernel<double>;
}

hipError_t launch_frames(const SpecPlan& p, const Call& c, const Layout& L, hipStream_t s) {
  SpecArgs a;
  a.in = c.in;
  a.stride = c.stride;
  a.mean = L.mean;
  a.tables = L.tab;
  a.out = c.out;
  a.scale = p.scale;
  a.first = c.first;
  a.count = c.count;
  a.nfft = p.nfft;
  a.lg = p.lg;
  a.pad = p.pad;
  a.ratio = p.ratio;
  a.nres = p.nres;
  a.hop = p.hop;
  a.jp = p.jp;
  a.lgjp = p.lgjp;
  a.xs_cap = p.xs_cap;
  a.dbscale = c.dbscale;
  void* args[] = {&a};
  const long long tiles = (c.count + p.jp - 1) / p.jp;  // count <= 2^40 / hop, jp >= 8: fits the grid
  return hipLaunchKernel(frame_kernel(c.in_kind), dim3((unsigned)tiles, (unsigned)c.n_series), dim3(ST), args, p.lds_bytes, s);
}

hipError_t launch_all(const SpecPlan& p, const Call& c, const Layout& L, hipStream_t s) {
  hipError_t e = launch_means(c, L, s);
  if (e == hipSuccess) e = launch_tables(p, L, s);
  if (e == hipSuccess) e = launch_frames(p, c, L, s);
  return e;
}

// The checks of both entry points, then the scratch: the caller holds sc.mu.
int prepare(const char* who, int device_id, const SpecPlan& p, const Call& c, DeviceScratch<1>& sc, Layout* L) {
  VP_HIP(hipSetDevice(device_id));
  VP_HIP(hipFuncSetAttribute(frame_kernel(c.in_kind), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  void* base = nullptr;
  if (const int rc = sc.b[0].grow(who, L->bytes(), L->bytes() / 8 + 4096, &base)) return rc;
  L->place(base);
  return VP_OK;
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_spectrogram(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                              double samp_rate, int nfft, int pad, int hop, int dbscale, int64_t first_frame, int64_t n_frames,
                              float* out_dev, void* stream) {
  SpecPlan p;
  if (const int rc = check_spectrogram("vp_spectrogram", in_dev, in_kind, n_series, series_stride, n, samp_rate, nfft, pad, hop,
                                       dbscale, first_frame, n_frames, out_dev, &p))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_spectrogram: device index");
  if (n_frames == 0) return VP_OK;
  const Call c = {in_dev, in_kind, n_series, (long long)series_stride, (long long)n, (long long)first_frame, (long long)n_frames,
                  dbscale, out_dev};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DeviceScratch<1>& sc = spec_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  Layout L(p, n_series, (long long)n);
  if (const int rc = prepare("vp_spectrogram", device_id, p, c, sc, &L)) return rc;
  VP_HIP(launch_all(p, c, L, s));
  VP_HIP(hipStreamSynchronize(s));  // the scratch is free for the next call, out_dev is complete
  return VP_OK;
}

extern "C" int vp_spectrogram_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_spectrogram_release_scratch", spec_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_spectrogram_bench(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                                    double samp_rate, int nfft, int pad, int hop, int dbscale, int64_t first_frame,
                                    int64_t n_frames, float* out_dev, int iters, float* ms_total, float* ms_frames) {
  VP_REQUIRE(ms_total && iters > 0 && n_frames > 0, "vp_spectrogram_bench: bad argument");
  SpecPlan p;
  if (const int rc = check_spectrogram("vp_spectrogram_bench", in_dev, in_kind, n_series, series_stride, n, samp_rate, nfft, pad,
                                       hop, dbscale, first_frame, n_frames, out_dev, &p))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_spectrogram_bench: device index");
  const Call c = {in_dev, in_kind, n_series, (long long)series_stride, (long long)n, (long long)first_frame, (long long)n_frames,
                  dbscale, out_dev};
  DeviceScratch<1>& sc = spec_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  Layout L(p, n_series, (long long)n);
  if (const int rc = prepare("vp_spectrogram_bench", device_id, p, c, sc, &L)) return rc;
  BenchTimer t;
  VP_HIP(t.init());
  const auto all = [&] { return launch_all(p, c, L, t.s); };
  float t_all = 0.f, t_frames = 0.f;
  VP_HIP(t.run(2, all));
  VP_HIP(t.time(iters, all, &t_all));
  VP_HIP(t.time(iters, [&] { return launch_frames(p, c, L, t.s); }, &t_frames));  // over the means and tables the last pass left
  *ms_total = t_all;
  if (ms_frames) *ms_frames = t_frames;
  return VP_OK;
}
