// Integer-factor decimation behind a zero-phase low-pass, on the device: what volpick_amd/resample.py computes on the
// host with scipy for traces whose rate is an integer multiple of the model's (SeisBench's annotate():
// trace.filter("lowpass", zerophase=True) + trace.decimate(no_filter=True)):
//
//     f = sosfilt(sos, x);  g = sosfilt(sos, f[::-1])[::-1];  y = g[::k]
//
// Two launches of one kernel template.  The forward pass reads x (int32 / float32 / float64) and writes f as float64
// into a scratch array; the backward pass reads f in reversed order and writes float32 at the kept samples only.
// Coefficients, state and f are float64: the reference filters in float64, and counts with a large offset lose
// several bits in an fp32 recursion (tests/test_decimate_f64_cpu.py).
//
// Parallel over the trace by warm-up ("Decimation"): a pass is cut into pieces of DC samples, one per
// thread; a thread starts `warm` samples ahead of its piece from zero state, `warm` chosen on the host from the
// largest pole radius r of the sections so that r^warm <= 2^-40.  A thread whose piece lies less than `warm` samples
// behind the start of the pass starts AT the start, from the true zero state: that reproduces the edge transients.
//
// Memory access: a workgroup of DT threads stages the DT * DC samples of its pieces and the DHALO samples ahead of
// them through LDS as float64 with coalesced loads; each thread then recurses over LDS.  Piece p of the image
// starts at double (DC + 1) p: lane l of a wave reads byte address 8 (DC + 1) l + const, dword (2 DC + 2) l = 2 l
// (mod 64) for DC = 32, so the 32 lanes of a ds_read_b64 group cover the 64 banks once -- no conflicts, where the
// unpadded image (stride 256 B) would put every lane on the same two banks.  Results go back into the image (a
// thread's own piece, after a barrier: its neighbours' warm-up has read the inputs there) and out with coalesced
// stores.
#include "device_scratch.h"
#include "sos_tile.h"  // DT, DC, DTILE, SosArg, phys(): shared with sosfilt.hip

namespace vp {
namespace {

constexpr int DHALO = 1024;         // room for the warm-up ahead of a tile (a multiple of DC)
constexpr int DLDS = (DHALO + DTILE) / DC * (DC + 1);  // doubles
constexpr size_t DLDS_BYTES = (size_t)DLDS * sizeof(double);
static_assert(DHALO % DC == 0, "the halo is a whole number of pieces");

// One pass.  Position m counts samples in the order the pass visits them: element m of the pass is in[m] (forward) or
// in[n - 1 - m] (REV).  Forward: f_out[m] for every m.  REV: y_out[j] = (float) result at element j * factor of the
// ORIGINAL order, for every j < ceil(n / factor); if *flag is set, NaN instead.
template <typename InT, int NS, bool REV>
__global__ __launch_bounds__(DT) void decimate_pass_kernel(const InT* __restrict__ in, const long long n, const SosArg sos,
                                                           const int warm, double* __restrict__ f_out,
                                                           float* __restrict__ y_out, const int factor,
                                                           int* __restrict__ flag) {
  extern __shared__ double dec_tile[];
  const int t = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * DTILE;  // first element of the tile; m0 < n by the grid size
  // kept outputs of this tile (REV): original indices [g_lo, g_hi] hold elements [m0, m0 + DTILE) of the pass
  long long j_lo = 0, j_hi = -1;
  if (REV) {
    const long long g_hi = n - 1 - m0;
    const long long g_lo = n - m0 - DTILE > 0 ? n - m0 - DTILE : 0;
    j_lo = (g_lo + factor - 1) / factor;
    j_hi = g_hi / factor;
    if (*flag) {  // a non-finite input sample: the whole-trace filter answers NaN everywhere (uniform branch)
      for (long long j = j_lo + t; j <= j_hi; j += DT) y_out[j] = __builtin_nanf("");
      return;
    }
  }
  // ---- stage elements [m0 - back, m0 + DTILE) as float64: image index q <-> element m0 - DHALO + q
  const int back = m0 < warm ? (int)m0 : warm;
  bool bad = false;
  for (int q = DHALO - back + t; q < DHALO + DTILE; q += DT) {
    const long long m = m0 - DHALO + q;
    double v = 0.0;
    if (m < n) v = static_cast<double>(in[REV ? n - 1 - m : m]);
    if (!REV) bad |= !(fabs(v) <= 1.7976931348623157e308);
    dec_tile[phys(q)] = v;
  }
  if (!REV && bad) *flag = 1;  // plain vector store; every writer writes the same word
  __syncthreads();
  // ---- this thread's piece: warm-up from zero state, then DC results kept in registers
  const int q0 = DHALO + t * DC;
  const long long ms = m0 + (long long)t * DC;
  const int w = ms < warm ? (int)ms : warm;
  double s1[NS], s2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) s1[s] = s2[s] = 0.0;
  // sos_step<NS> of sos_tile.h, kept as a local lambda: with the shared function the compiler schedules twelve of the
  // instantiations differently (LOG.md, section 33)
  auto step = [&](double v) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {  // direct form II transposed, the recurrence of scipy's sosfilt
      const double y = sos.c[s][0] * v + s1[s];
      s1[s] = sos.c[s][1] * v - sos.c[s][3] * y + s2[s];
      s2[s] = sos.c[s][2] * v - sos.c[s][4] * y;
      v = y;
    }
    return v;
  };
  double r[DC];
  if (ms < n) {
#pragma unroll 8
    for (int q = q0 - w; q < q0; ++q) (void)step(dec_tile[phys(q)]);
    const int p0 = phys(q0);  // q0 is a multiple of DC: the piece is contiguous in the image
#pragma unroll
    for (int i = 0; i < DC; ++i) r[i] = step(dec_tile[p0 + i]);
  }
  __syncthreads();  // every warm-up has read its inputs
  if (ms < n) {
    const int p0 = phys(q0);
#pragma unroll
    for (int i = 0; i < DC; ++i) dec_tile[p0 + i] = r[i];
  }
  __syncthreads();
  if (!REV) {
    for (int q = DHALO + t; q < DHALO + DTILE; q += DT) {
      const long long m = m0 - DHALO + q;
      if (m < n) f_out[m] = dec_tile[phys(q)];
    }
  } else {
    for (long long j = j_lo + t; j <= j_hi; j += DT) {
      const long long m = n - 1 - j * factor;  // in [m0, m0 + DTILE) and < n by the choice of j_lo, j_hi
      y_out[j] = static_cast<float>(dec_tile[phys(DHALO + (int)(m - m0))]);
    }
  }
}

template <typename InT, bool REV>
const void* pass_kernel(int ns) {
  switch (ns) {
    case 1: return (const void*)decimate_pass_kernel<InT, 1, REV>;
    case 2: return (const void*)decimate_pass_kernel<InT, 2, REV>;
    case 3: return (const void*)decimate_pass_kernel<InT, 3, REV>;
    default: return (const void*)decimate_pass_kernel<InT, 4, REV>;
  }
}

const void* forward_kernel(int in_kind, int ns) {
  if (in_kind == VP_SAMPLES_INT32) return pass_kernel<int, false>(ns);
  if (in_kind == VP_SAMPLES_FLOAT32) return pass_kernel<float, false>(ns);
  return pass_kernel<double, false>(ns);
}

// Per device, grow-only, reused from call to call: f (8 bytes per input sample) and the flag word.
DeviceScratch<1>& decimate_scratch(int device) {
  static DeviceScratch<1> pool[64];
  return pool[(unsigned)device % 64];
}

// the flag word and f of a call of n samples
int grow_scratch(const char* who, DeviceScratch<1>& sc, int64_t n, int** flag, double** f) {
  const size_t bytes = 64 + (size_t)n * sizeof(double);
  void* p = nullptr;
  if (const int rc = sc.b[0].grow(who, bytes, bytes / 8 + 4096, &p)) return rc;
  *flag = (int*)p;
  *f = (double*)((char*)p + 64);
  return VP_OK;
}

struct Plan {
  SosArg arg;
  int warm;
  const void *fwd, *bwd;
};

int make_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections, int factor,
              const float* out_dev, int64_t out_len, Plan* plan) {
  VP_REQUIRE(in_dev && sos && out_dev, "%s: null argument", who);
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n >= 1, "%s: n = %lld, need at least one sample", who, (long long)n);
  VP_REQUIRE(factor >= 2, "%s: factor = %d, need >= 2", who, factor);
  VP_REQUIRE(out_len == (n + factor - 1) / factor, "%s: out_len = %lld, ceil(n / factor) = %lld", who, (long long)out_len,
             (long long)((n + factor - 1) / factor));
  double r = 0.0;
  if (const int rc = load_sos(who, sos, n_sections, &plan->arg, &r)) return rc;
  plan->warm = warmup_length(sos, n_sections, &r);  // the same radius again, and what it asks for
  VP_REQUIRE(plan->warm >= 0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  if (plan->warm > DHALO) {
    set_error("%s: largest pole radius %g needs a warm-up of %d samples, the tile has room for %d", who, r, plan->warm, DHALO);
    return VP_ERR_UNSUPPORTED;
  }
  plan->fwd = forward_kernel(in_kind, n_sections);
  plan->bwd = pass_kernel<double, true>(n_sections);
  return VP_OK;
}

int prepare_kernels(const Plan& plan) {
  VP_HIP(hipFuncSetAttribute(plan.fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DLDS_BYTES));
  VP_HIP(hipFuncSetAttribute(plan.bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DLDS_BYTES));
  return VP_OK;
}

// every instantiation takes the same argument list (the input pointer's type aside)
hipError_t launch_pass(const void* kernel, const Plan& plan, const void* in, long long n, double* f_out, float* y_out,
                       int factor, int* flag, hipStream_t s) {
  SosArg arg = plan.arg;
  int warm = plan.warm;
  void* args[] = {&in, &n, &arg, &warm, &f_out, &y_out, &factor, &flag};
  return hipLaunchKernel(kernel, dim3((unsigned)((n + DTILE - 1) / DTILE)), dim3(DT), args, DLDS_BYTES, s);
}

hipError_t launch_passes(const Plan& plan, const void* in_dev, long long n, int factor, double* f, int* flag, float* out,
                         hipStream_t s) {
  const hipError_t e = launch_pass(plan.fwd, plan, in_dev, n, f, nullptr, factor, flag, s);
  return e != hipSuccess ? e : launch_pass(plan.bwd, plan, f, n, nullptr, out, factor, flag, s);
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_decimate_lowpass(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos,
                                   int n_sections, int factor, float* out_dev, int64_t out_len) {
  Plan plan;
  if (const int rc = make_plan("vp_decimate_lowpass", in_dev, in_kind, n, sos, n_sections, factor, out_dev, out_len, &plan))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_decimate_lowpass: device index");
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels(plan)) return rc;
  hipStream_t s = nullptr;  // the null stream, one synchronisation at the end: as vp_mseed_decode
  DeviceScratch<1>& sc = decimate_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  int* flag;
  double* f;
  if (const int rc = grow_scratch("vp_decimate_lowpass", sc, n, &flag, &f)) return rc;
  VP_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
  VP_HIP(launch_passes(plan, in_dev, (long long)n, factor, f, flag, out_dev, s));
  VP_HIP(hipStreamSynchronize(s));
  return VP_OK;
}

extern "C" int vp_decimate_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_decimate_release_scratch", decimate_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_decimate_lowpass_bench(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos,
                                         int n_sections, int factor, float* out_dev, int64_t out_len, int iters,
                                         float* ms_total, float* ms_forward) {
  VP_REQUIRE(ms_total && iters > 0, "vp_decimate_lowpass_bench: bad argument");
  Plan plan;
  if (const int rc = make_plan("vp_decimate_lowpass_bench", in_dev, in_kind, n, sos, n_sections, factor, out_dev, out_len,
                               &plan))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_decimate_lowpass_bench: device index");
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels(plan)) return rc;
  DeviceScratch<1>& sc = decimate_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  int* flag;
  double* f;
  if (const int rc = grow_scratch("vp_decimate_lowpass_bench", sc, n, &flag, &f)) return rc;
  BenchTimer t;
  VP_HIP(t.init());
  VP_HIP(hipMemsetAsync(flag, 0, sizeof(int), t.s));
  const auto both = [&] { return launch_passes(plan, in_dev, (long long)n, factor, f, flag, out_dev, t.s); };
  const auto forward = [&] { return launch_pass(plan.fwd, plan, in_dev, (long long)n, f, nullptr, factor, flag, t.s); };
  float t_all = 0.f, t_fwd = 0.f;
  VP_HIP(t.run(3, both));
  VP_HIP(t.time(iters, both, &t_all));
  VP_HIP(t.time(iters, forward, &t_fwd));
  *ms_total = t_all;
  if (ms_forward) *ms_forward = t_fwd;
  return VP_OK;
}
