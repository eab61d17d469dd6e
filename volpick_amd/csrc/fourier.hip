// Fourier resampling on the device: what volpick_amd/resample.py:resample_fourier computes on the host with scipy for
// traces whose rate is no integer multiple of the model's (SeisBench's annotate(): trace.resample(rate, no_filter=True),
// ObsPy's Fourier method with a Hann window):
//
//     X = rfft(x) * ifftshift(hann(N))[:N/2+1];  Y = interp(large_f, f, X) (Re and Im apart);  y = irfft(Y) * num / N
//
// N and num are arbitrary (primes, a day with one sample missing), so both transforms run as Bluestein chirp-z
// convolutions over power-of-two complex float64 FFTs of size M >= 2 L - 1 (L = N forward, L = num inverse):
//
//     DFT_s(v)[k] = c[k] * sum_n (v[n] c[n]) conj(c[k - n]),   c[j] = exp(s i pi j^2 / L),  s = -1 forward, +1 inverse
//
// The phase j^2 / L is reduced in 64-bit integers ((j * j) mod 2 L) before it is divided: j^2 reaches 4.7e14, and a
// float64 phase reduced after the multiply would lose its low bits.  Everything is float64; the one rounding to float32
// is the final store.
//
// The FFT of size M ("Fourier resampling ahead of the picker"): M = P0 * P1 * P2 with the last factor up to
// TILE = 4096, run as one pass per factor (the four-step scheme applied twice).  A pass transforms P elements at stride S
// inside segments of G = P * S elements and then multiplies element (k, c) by exp(-/+ 2 pi i c k / G); the next pass works
// inside the rows of S elements.  The forward FFT therefore leaves the spectrum in a digit-permuted order, the point-wise
// product with the chirp filter's spectrum (same order) does not care, and the inverse FFT runs the passes backwards and
// lands in natural order: no transposes, every pass in place.  A workgroup of a strided pass takes nb = TILE / P >= 16
// adjacent columns (>= 256-byte runs in global memory) and keeps them interleaved in LDS (element (j, b) at j * nb + b),
// so that every ds_read_b128 / ds_write_b128 lane group of a Stockham stage touches contiguous bytes.  The contiguous
// pass (nb = 1) pads the image by one element in eight: the first radix-4 stage stores at a lane stride of 64 bytes,
// which unpadded is a 4-way conflict on the 8 x 8-lane groups of ds_write_b128.
#include <cmath>

#include "device_scratch.h"
#include "sos_host.h"  // check_sample_kind

namespace vp {
namespace {

typedef double2 cd;

constexpr int FT = 256;                       // threads per workgroup
constexpr int LOG_TILE = 12;
constexpr int TILE = 1 << LOG_TILE;           // the largest transform done inside LDS (tests/fourier_f64.py: FFT_TILE)
constexpr int LOG_COLS = 4;                   // a strided pass takes at least 2^4 adjacent columns (FFT_COLS)
constexpr int MAX_LOG_M = 27;
constexpr int PER_THREAD = TILE / FT;         // elements a thread holds in registers during a stage
constexpr size_t LDS_BYTES = (size_t)(TILE + TILE / 8) * sizeof(cd);  // 72 KiB: two workgroups per CU

enum { LM_PLAIN, LM_TWID, LM_INPUT, LM_CHIRPB, LM_SPEC };
enum { SM_PLAIN, SM_TWID, SM_MULB, SM_SPECTRUM, SM_OUTPUT };

struct PassArg {
  int logP;     // transform length of this pass
  int lognb;    // transforms per workgroup (adjacent columns); 0 for the contiguous pass
  int logS;     // stride between the elements of one transform
  int log_tps;  // workgroups per segment of G = P * S elements: S / nb
};

struct Ctx {
  const void* in;  // LM_INPUT: the trace
  int in_kind;
  long long n;     // input samples
  long long num;   // output samples
  long long L;     // length of the DFT this convolution computes (n forward, num inverse)
  double sgn;      // sign of its exponent: -1 forward, +1 inverse
  int logM;
  const cd* B;     // SM_MULB: spectrum of the chirp filter, in the forward FFT's output order
  cd* X;           // SM_SPECTRUM writes, LM_SPEC reads: the windowed half spectrum, n / 2 + 1 bins
  float* out;
  int* flag;
  double df, dlf;
};

__device__ __forceinline__ cd cmul(const cd a, const cd b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// exp(sgn i pi j^2 / L), the phase reduced in integers
__device__ __forceinline__ cd chirp(const long long j, const long long L, const double sgn) {
  const unsigned long long r = (unsigned long long)(j * j) % (unsigned long long)(2 * L);
  double s, c;
  sincospi((double)r / (double)L, &s, &c);
  return make_double2(c, sgn * s);
}

// exp(sgn 2 pi i a / 2^logG), 0 <= a < 2^logG
__device__ __forceinline__ cd unit_root(const long long a, const int logG, const double sgn) {
  double s, c;
  sincospi(ldexp((double)a, 1 - logG), &s, &c);
  return make_double2(c, sgn * s);
}

// numpy.interp(dlf * m, df * arange(K), X), real and imaginary parts apart: same float64 products for the two grids, same
// comparisons for the interval, slope * (x - xp[j]) + fp[j] without contraction.
__device__ cd spectrum_at(const cd* __restrict__ X, const long long K, const long long m, const double df, const double dlf) {
#pragma clang fp contract(off)
  const double xq = dlf * (double)m;
  if (xq > df * (double)(K - 1)) return X[K - 1];  // beyond the old Nyquist: np.interp holds the last value
  long long j = (long long)(xq / df);
  j = j < 0 ? 0 : (j > K - 1 ? K - 1 : j);
  while (j > 0 && df * (double)j > xq) --j;
  while (j < K - 1 && df * (double)(j + 1) <= xq) ++j;
  if (j == K - 1) return X[j];
  const double x0 = df * (double)j;
  const cd a = X[j];
  if (x0 == xq) return a;
  const cd b = X[j + 1];
  const double dx = df * (double)(j + 1) - x0;
  const double t = xq - x0;
  const double sr = (b.x - a.x) / dx, si = (b.y - a.y) / dx;
  return make_double2(sr * t + a.x, si * t + a.y);
}

__device__ __forceinline__ int phys(const int e, const int padmask) { return e + ((e >> 3) & padmask); }

// One Stockham stage of radix R over the tile: butterfly jj of transform b reads elements jj + r P / R, multiplies by
// exp(DIR 2 pi i r (jj mod Ns) / (Ns R)) and writes the R-point DFT to (jj / Ns) Ns R + jj mod Ns + r Ns.  Every thread
// holds its PER_THREAD elements in registers across the barrier, so the stage runs in place.
template <int R, int DIR>
__device__ __forceinline__ void stage(cd* tile, const cd* __restrict__ wt, const int t, const int logP, const int lognb,
                                      const int logNs, const int padmask) {
  constexpr int LOGR = R == 4 ? 2 : 1;
  constexpr int IT = PER_THREAD / R;
  const int nbf = 1 << (logP - LOGR + lognb);  // butterflies in the tile
  const int q = 1 << (logP - LOGR);            // P / R
  const int nbm = (1 << lognb) - 1, nsm = (1 << logNs) - 1;
  cd v[IT][R];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int w = t + it * FT;
    if (w < nbf) {
      const int b = w & nbm, jj = w >> lognb;
#pragma unroll
      for (int r = 0; r < R; ++r) v[it][r] = tile[phys(((jj + r * q) << lognb) + b, padmask)];
      if (logNs > 0) {
        const int step = (jj & nsm) << (LOG_TILE - logNs - LOGR);  // (jj mod Ns) / (Ns R) in units of 1 / TILE
#pragma unroll
        for (int r = 1; r < R; ++r) {
          cd tw = wt[step * r];
          if (DIR > 0) tw.y = -tw.y;
          v[it][r] = cmul(v[it][r], tw);
        }
      }
      if (R == 2) {
        const cd a = v[it][0], c = v[it][1];
        v[it][0] = make_double2(a.x + c.x, a.y + c.y);
        v[it][1] = make_double2(a.x - c.x, a.y - c.y);
      } else {
        const cd a = v[it][0], b1 = v[it][1], c = v[it][2], d = v[it][3];
        const cd t0 = make_double2(a.x + c.x, a.y + c.y), t1 = make_double2(a.x - c.x, a.y - c.y);
        const cd t2 = make_double2(b1.x + d.x, b1.y + d.y);
        const cd u = make_double2(b1.x - d.x, b1.y - d.y);
        // (b - d) times -i (forward) or +i (inverse)
        const cd t3 = DIR < 0 ? make_double2(u.y, -u.x) : make_double2(-u.y, u.x);
        v[it][0] = make_double2(t0.x + t2.x, t0.y + t2.y);
        v[it][1] = make_double2(t1.x + t3.x, t1.y + t3.y);
        v[it][2] = make_double2(t0.x - t2.x, t0.y - t2.y);
        v[it][3] = make_double2(t1.x - t3.x, t1.y - t3.y);
      }
    }
  }
  __syncthreads();  // every butterfly has read its inputs
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int w = t + it * FT;
    if (w < nbf) {
      const int b = w & nbm, jj = w >> lognb;
      const int d0 = ((jj >> logNs) << (logNs + LOGR)) + (jj & nsm);
#pragma unroll
      for (int r = 0; r < R; ++r) tile[phys(((d0 + (r << logNs)) << lognb) + b, padmask)] = v[it][r];
    }
  }
  __syncthreads();
}

// One pass of the FFT of size 2^logM (file comment).  LM: what the load computes; SM: what the store computes; DIR: sign
// of the FFT's exponent.  Element (j, b) of the workgroup's tile is buf[base + j S + b], column c = c0 + b of its segment.
template <int LM, int SM, int DIR>
__global__ __launch_bounds__(FT) void fft_pass_kernel(cd* __restrict__ buf, const cd* __restrict__ wt, const PassArg pa,
                                                      const Ctx cx) {
  extern __shared__ double2 fft_tile[];
  const int t = threadIdx.x;
  const int te = 1 << (pa.logP + pa.lognb);  // elements of the tile
  const int nbm = (1 << pa.lognb) - 1;
  const int padmask = pa.lognb >= 3 ? 0 : ~0;
  const long long seg = (long long)blockIdx.x >> pa.log_tps;
  const long long c0 = ((long long)blockIdx.x & ((1ll << pa.log_tps) - 1)) << pa.lognb;
  const int logG = pa.logP + pa.logS;
  const long long base = (seg << logG) + c0;
  const long long M = 1ll << cx.logM;

  bool bad = false;
  for (int e = t; e < te; e += FT) {
    const int b = e & nbm, j = e >> pa.lognb;
    const long long p = base + ((long long)j << pa.logS) + b;
    cd v = make_double2(0.0, 0.0);
    if (LM == LM_PLAIN) {
      v = buf[p];
    } else if (LM == LM_TWID) {
      v = cmul(buf[p], unit_root((c0 + b) * j, logG, 1.0));
    } else if (LM == LM_INPUT) {
      if (p < cx.n) {
        double x;
        if (cx.in_kind == VP_SAMPLES_INT32) x = (double)((const int*)cx.in)[p];
        else if (cx.in_kind == VP_SAMPLES_FLOAT32) x = (double)((const float*)cx.in)[p];
        else x = ((const double*)cx.in)[p];
        bad |= !(fabs(x) <= 1.7976931348623157e308);
        const cd c = chirp(p, cx.L, cx.sgn);
        v = make_double2(x * c.x, x * c.y);
      }
    } else if (LM == LM_CHIRPB) {
      const long long jj = p < cx.L ? p : (p > M - cx.L ? M - p : -1);
      if (jj >= 0) v = chirp(jj, cx.L, -cx.sgn);
    } else if (LM == LM_SPEC) {
      if (p < cx.num) {
        const long long half = cx.num / 2;
        const long long m = p <= half ? p : cx.num - p;
        cd y = spectrum_at(cx.X, cx.n / 2 + 1, m, cx.df, cx.dlf);
        if (m == 0 || 2 * m == cx.num) y.y = 0.0;  // what a real inverse transform ignores
        if (p > half) y.y = -y.y;                  // Hermitian extension
        v = cmul(y, chirp(p, cx.L, cx.sgn));
      }
    }
    fft_tile[phys(e, padmask)] = v;
  }
  if (LM == LM_INPUT && bad) *cx.flag = 1;  // plain vector store; every writer writes the same word
  __syncthreads();

  int logNs = 0;
  for (; logNs + 2 <= pa.logP; logNs += 2) stage<4, DIR>(fft_tile, wt, t, pa.logP, pa.lognb, logNs, padmask);
  if (logNs < pa.logP) stage<2, DIR>(fft_tile, wt, t, pa.logP, pa.lognb, logNs, padmask);

  const bool poisoned = SM == SM_OUTPUT ? *cx.flag != 0 : false;
  for (int e = t; e < te; e += FT) {
    const int b = e & nbm, j = e >> pa.lognb;
    const long long p = base + ((long long)j << pa.logS) + b;
    const cd v = fft_tile[phys(e, padmask)];
    if (SM == SM_PLAIN) {
      buf[p] = v;
    } else if (SM == SM_TWID) {
      buf[p] = cmul(v, unit_root((c0 + b) * j, logG, -1.0));
    } else if (SM == SM_MULB) {
      const cd r = cmul(v, cx.B[p]);
      const double s = ldexp(1.0, -cx.logM);  // the inverse FFT's 1 / M, exact
      buf[p] = make_double2(r.x * s, r.y * s);
    } else if (SM == SM_SPECTRUM) {
      if (p <= cx.n / 2) {
        cd x = cmul(v, chirp(p, cx.L, cx.sgn));
        if (p == 0 || 2 * p == cx.n) x.y = 0.0;  // a real transform's DC and Nyquist bins
        double w = 1.0;                          // scipy's get_window("hann", 1) is [1.0]
        if (cx.n > 1) {
          const long long jw = (p + cx.n / 2) % cx.n;  // ifftshift of the periodic Hann window
          w = 0.5 - 0.5 * cospi((double)(2 * jw) / (double)cx.n);
        }
        cx.X[p] = make_double2(x.x * w, x.y * w);
      }
    } else if (SM == SM_OUTPUT) {
      if (p < cx.num) {
        const cd c = chirp(p, cx.L, cx.sgn);
        const double y = (v.x * c.x - v.y * c.y) / (double)cx.n;
        cx.out[p] = poisoned ? __builtin_nanf("") : (float)y;
      }
    }
  }
}

__global__ __launch_bounds__(FT) void twiddle_table_kernel(cd* __restrict__ wt) {
  const int i = blockIdx.x * FT + threadIdx.x;  // grid covers TILE exactly
  double s, c;
  sincospi(ldexp((double)i, 1 - LOG_TILE), &s, &c);
  wt[i] = make_double2(c, -s);
}

#define VP_FFT_KERNELS(K)                                                                                              \
  K(LM_INPUT, SM_TWID, -1) K(LM_INPUT, SM_MULB, -1) K(LM_SPEC, SM_TWID, -1) K(LM_SPEC, SM_MULB, -1)                     \
  K(LM_CHIRPB, SM_TWID, -1) K(LM_CHIRPB, SM_PLAIN, -1) K(LM_PLAIN, SM_TWID, -1) K(LM_PLAIN, SM_MULB, -1)                \
  K(LM_PLAIN, SM_PLAIN, -1) K(LM_PLAIN, SM_PLAIN, 1) K(LM_PLAIN, SM_SPECTRUM, 1) K(LM_PLAIN, SM_OUTPUT, 1)              \
  K(LM_TWID, SM_PLAIN, 1) K(LM_TWID, SM_SPECTRUM, 1) K(LM_TWID, SM_OUTPUT, 1)

const void* pass_kernel(int lm, int sm, int dir) {
#define K(l, s, d) \
  if (lm == l && sm == s && dir == d) return (const void*)fft_pass_kernel<l, s, d>;
  VP_FFT_KERNELS(K)
#undef K
  return nullptr;
}

int prepare_kernels() {
#define K(l, s, d) \
  VP_HIP(hipFuncSetAttribute((const void*)fft_pass_kernel<l, s, d>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
  VP_FFT_KERNELS(K)
#undef K
  return VP_OK;
}

// The passes of the FFT that a Bluestein convolution of length L needs: M = 2^logM >= 2 L - 1.
struct FftPlan {
  int logM = 0, npass = 0;
  PassArg pass[3];
};

FftPlan plan_fft(long long L) {
  FftPlan f;
  while ((1ll << f.logM) < 2 * L - 1) ++f.logM;
  int logp[3];
  if (f.logM <= LOG_TILE) {
    f.npass = 1;
    logp[0] = f.logM;
  } else {
    const int r = f.logM - LOG_TILE;  // what the strided passes share
    if (r <= LOG_TILE - LOG_COLS) {
      f.npass = 2;
      logp[0] = r;
    } else {
      f.npass = 3;
      logp[0] = (r + 1) / 2;
      logp[1] = r / 2;
    }
    logp[f.npass - 1] = LOG_TILE;
  }
  int logS = f.logM;
  for (int i = 0; i < f.npass; ++i) {
    logS -= logp[i];
    PassArg& a = f.pass[i];
    a.logP = logp[i];
    a.logS = logS;
    a.lognb = logS == 0 ? 0 : LOG_TILE - logp[i];
    a.log_tps = logS - a.lognb;
  }
  return f;
}

hipError_t launch(int lm, int sm, int dir, cd* buf, const cd* wt, const PassArg& pa, const Ctx& cx, hipStream_t s) {
  const void* k = pass_kernel(lm, sm, dir);
  if (!k) return hipErrorInvalidDeviceFunction;
  PassArg a = pa;
  Ctx c = cx;
  void* args[] = {&buf, &wt, &a, &c};
  const int log_te = pa.logP + pa.lognb;
  const size_t te = (size_t)1 << log_te;
  return hipLaunchKernel(k, dim3((unsigned)(1u << (cx.logM - log_te))), dim3(FT), args, (te + te / 8) * sizeof(cd), s);
}

// One DFT by Bluestein's convolution: bufB <- FFT(chirp filter); bufA <- FFT(first_lm load) * bufB / M; inverse FFT of bufA
// with `final_sm` as its last store.
hipError_t launch_transform(const FftPlan& f, int first_lm, int final_sm, cd* bufA, cd* bufB, const cd* wt, Ctx cx,
                            hipStream_t s) {
  cx.logM = f.logM;
  cx.B = bufB;
  const int np = f.npass;
  hipError_t e = hipSuccess;
  for (int i = 0; i < np && e == hipSuccess; ++i)
    e = launch(i == 0 ? LM_CHIRPB : LM_PLAIN, i == np - 1 ? SM_PLAIN : SM_TWID, -1, bufB, wt, f.pass[i], cx, s);
  for (int i = 0; i < np && e == hipSuccess; ++i)
    e = launch(i == 0 ? first_lm : LM_PLAIN, i == np - 1 ? SM_MULB : SM_TWID, -1, bufA, wt, f.pass[i], cx, s);
  for (int i = np - 1; i >= 0 && e == hipSuccess; --i)
    e = launch(i == np - 1 ? LM_PLAIN : LM_TWID, i == 0 ? final_sm : SM_PLAIN, 1, bufA, wt, f.pass[i], cx, s);
  return e;
}

// Per device, grow-only, reused from call to call: flag word, twiddle table, half spectrum, the two FFT buffers.
DeviceScratch<1>& resample_scratch(int device) {
  static DeviceScratch<1> pool[64];
  return pool[(unsigned)device % 64];
}

struct Job {
  FftPlan fwd, inv;
  Ctx cx;
  size_t off_wt, off_x, off_a, off_b, bytes;
};

int make_job(const char* who, const void* in_dev, int in_kind, int64_t n, double rate_in, double rate_out, int64_t num,
             double df, double d_large_f, float* out_dev, int64_t out_len, Job* job) {
  VP_REQUIRE(in_dev && out_dev, "%s: null argument", who);
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n >= 1, "%s: n = %lld, need at least one sample", who, (long long)n);
  VP_REQUIRE(num >= 1, "%s: num = %lld, need at least one output sample", who, (long long)num);
  VP_REQUIRE(out_len == num, "%s: out_len = %lld, num = %lld", who, (long long)out_len, (long long)num);
  VP_REQUIRE(std::isfinite(rate_in) && rate_in > 0 && std::isfinite(rate_out) && rate_out > 0,
             "%s: rates %g -> %g Hz, need finite positive rates", who, rate_in, rate_out);
  VP_REQUIRE(std::isfinite(df) && df > 0 && std::isfinite(d_large_f) && d_large_f > 0,
             "%s: frequency steps %g and %g, need finite positive steps", who, df, d_large_f);
  const int64_t lmax = n > num ? n : num;
  if (2 * lmax - 1 > (1ll << MAX_LOG_M)) {
    set_error("%s: %lld -> %lld samples needs an FFT beyond 2^%d points", who, (long long)n, (long long)num, MAX_LOG_M);
    return VP_ERR_UNSUPPORTED;
  }
  job->fwd = plan_fft(n);
  job->inv = plan_fft(num);
  const int logmax = job->fwd.logM > job->inv.logM ? job->fwd.logM : job->inv.logM;
  const size_t buf = sizeof(cd) << logmax;
  job->off_wt = 64;
  job->off_x = job->off_wt + sizeof(cd) * TILE;
  job->off_a = job->off_x + (((size_t)n / 2 + 1) * sizeof(cd) + 255) / 256 * 256;
  job->off_b = job->off_a + buf;
  job->bytes = job->off_b + buf;
  Ctx& c = job->cx;
  c.in = in_dev;
  c.in_kind = in_kind;
  c.n = n;
  c.num = num;
  c.out = out_dev;
  c.df = df;
  c.dlf = d_large_f;
  c.L = 0, c.sgn = 0, c.logM = 0, c.B = nullptr, c.X = nullptr, c.flag = nullptr;
  return VP_OK;
}

// binds the job to the scratch; the table is written per call
void bind(Job& job, void* p, cd** wt, cd** a, cd** b) {
  job.cx.flag = (int*)p;
  *wt = (cd*)((char*)p + job.off_wt);
  job.cx.X = (cd*)((char*)p + job.off_x);
  *a = (cd*)((char*)p + job.off_a);
  *b = (cd*)((char*)p + job.off_b);
}

hipError_t launch_forward(const Job& job, cd* wt, cd* a, cd* b, hipStream_t s) {
  Ctx cx = job.cx;
  cx.L = cx.n;
  cx.sgn = -1.0;
  return launch_transform(job.fwd, LM_INPUT, SM_SPECTRUM, a, b, wt, cx, s);
}

hipError_t launch_all(const Job& job, cd* wt, cd* a, cd* b, hipStream_t s) {
  hipError_t e = hipMemsetAsync(job.cx.flag, 0, sizeof(int), s);  // the flag does not outlive the call
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(twiddle_table_kernel, dim3(TILE / FT), dim3(FT), 0, s, wt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_forward(job, wt, a, b, s)) != hipSuccess) return e;
  Ctx cx = job.cx;
  cx.L = cx.num;
  cx.sgn = 1.0;
  return launch_transform(job.inv, LM_SPEC, SM_OUTPUT, a, b, wt, cx, s);
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_resample_fourier(int device_id, const void* in_dev, int in_kind, int64_t n, double rate_in, double rate_out,
                                   int64_t num, double df, double d_large_f, float* out_dev, int64_t out_len) {
  const char* who = "vp_resample_fourier";
  Job job;
  if (const int rc = make_job(who, in_dev, in_kind, n, rate_in, rate_out, num, df, d_large_f, out_dev, out_len, &job)) return rc;
  VP_REQUIRE(device_id >= 0, "vp_resample_fourier: device index");
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels()) return rc;
  hipStream_t s = nullptr;  // the null stream, one synchronisation at the end: as vp_decimate_lowpass
  DeviceScratch<1>& sc = resample_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  if (const int rc = sc.b[0].grow(who, job.bytes, 0, &p)) return rc;  // exact: 2 GiB after a 250 Hz component-day
  cd *wt, *a, *b;
  bind(job, p, &wt, &a, &b);
  VP_HIP(launch_all(job, wt, a, b, s));
  VP_HIP(hipStreamSynchronize(s));
  return VP_OK;
}

extern "C" int vp_resample_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_resample_release_scratch", resample_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_resample_fourier_bench(int device_id, const void* in_dev, int in_kind, int64_t n, double rate_in,
                                         double rate_out, int64_t num, double df, double d_large_f, float* out_dev,
                                         int64_t out_len, int iters, float* ms_total, float* ms_forward) {
  const char* who = "vp_resample_fourier_bench";
  VP_REQUIRE(ms_total && iters > 0, "vp_resample_fourier_bench: bad argument");
  Job job;
  if (const int rc = make_job(who, in_dev, in_kind, n, rate_in, rate_out, num, df, d_large_f, out_dev, out_len, &job)) return rc;
  VP_REQUIRE(device_id >= 0, "vp_resample_fourier_bench: device index");
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels()) return rc;
  DeviceScratch<1>& sc = resample_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  if (const int rc = sc.b[0].grow(who, job.bytes, 0, &p)) return rc;  // exact: 2 GiB after a 250 Hz component-day
  cd *wt, *a, *b;
  bind(job, p, &wt, &a, &b);
  BenchTimer t;
  VP_HIP(t.init());
  const auto all = [&] { return launch_all(job, wt, a, b, t.s); };
  float t_all = 0.f, t_fwd = 0.f;
  VP_HIP(t.run(3, all));
  VP_HIP(t.time(iters, all, &t_all));
  VP_HIP(t.time(iters, [&] { return launch_forward(job, wt, a, b, t.s); }, &t_fwd));
  *ms_total = t_all;
  if (ms_forward) *ms_forward = t_fwd;
  return VP_OK;
}
