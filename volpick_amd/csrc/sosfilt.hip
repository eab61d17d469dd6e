// General IIR filtering (second-order sections) and detrending of device-resident traces: what ObsPy's
// trace.filter(...) and trace.detrend(...) compute on the host with scipy (volpick_amd/signal.py restates them):
//
//     y = sosfilt(sos, x)                       one pass
//     y = sosfilt(sos, sosfilt(sos, x)[::-1])[::-1]     zerophase
//
// Input int32 / float32 / float64; coefficients, state and the intermediate of the zero-phase form float64; output
// float32, rounded once at the end.
//
// Parallel over the trace by an EXACT carry of the filter state ("Filtering"); the warm-up of resample.hip
// cannot serve a 0.3 Hz high-pass, whose start-state response outlives any halo.  The state z (2 doubles per section,
// d = 2 NS <= 8) is linear in itself: one sample does z <- A z + B x, so a run of L samples from state z0 ends in
// A^L z0 + e, e being the end of the same run from zero state.  The host squares A into the table
// M_k = A^(DC 2^k), k = 0..15 (sos_matrices.h: in double-double, plain float64 squaring is not good enough), and a pass is
// three launches:
//
//   reduce  one workgroup per tile (all but the last): every thread runs its piece of DC samples from zero state; an
//           inclusive scan over the DT threads, S_p <- M_k S_(p - 2^k) + S_p for k = 0..7, leaves in the last thread
//           the tile's zero-state end E_t.
//   carry   one workgroup: Z_(t+1) = A^DTILE Z_t + E_t, Z_0 = 0, as the same scan with M_8..M_15 over 256 tiles at a
//           time, the chunk's last state carried into the next chunk's first element.
//   apply   one workgroup per tile: the pieces again from zero state, thread 0 from Z_t, so the same scan now leaves
//           the TRUE end state of every piece; each thread takes its left neighbour's, runs its piece a second time
//           from it and keeps the DC results, which leave through the tile image with coalesced stores.
//
// Order between tiles comes from the launch boundaries alone: no flags, no atomics, no grid barrier; the same call gives
// the same bits every time.  A matrix is block lower triangular (a section feeds only later ones) and the products skip
// the zero blocks.  A NaN needs no flag: it stays in the state of its section and of every later one through each product
// (0 * NaN is NaN), so everything behind it in the order of the pass is NaN, and in a zero-phase call everything.
//
// Detrending: float64 sums in a fixed order (per-workgroup partials, then one workgroup), then one subtracting pass.
#include "device_scratch.h"
#include "sos_matrices.h"
#include "sos_tile.h"

namespace vp {
namespace {

constexpr int SLEV = 16;       // doubling matrices: 0..7 span the pieces of a tile, 8..15 the tiles of a carry chunk
constexpr int SMAT = 64;       // doubles per matrix: row-major d x d in the first d * d
constexpr int SD = 2 * DMAXS;  // doubles per state row in E and Z, whatever d is
constexpr int SXW = DT - 64;   // exchange slots: the steps of 64 and 128 threads read that far to the left
constexpr int SIMG = DTILE / DC * (DC + 1);  // doubles of a tile image
constexpr size_t SLDS_BYTES = (size_t)(SIMG + SD * SXW) * sizeof(double);  // 79,872: two workgroups per CU
constexpr size_t SCARRY_LDS_BYTES = (size_t)(SD * SXW + SD) * sizeof(double);
static_assert(DT == 256, "the scan is written for four waves of 64");
static_assert(DC == 32 && SMAT == sosmat::STRIDE && SD == sosmat::MAXD, "the host's table is laid out for these");

// S += M U for the lower block triangular M (2 x 2 blocks)
template <int NS>
__device__ __forceinline__ void combine(double (&S)[2 * NS], const double (&U)[2 * NS], const double* __restrict__ M) {
#pragma unroll
  for (int i = 0; i < 2 * NS; ++i) {
    double acc = S[i];
#pragma unroll
    for (int j = 0; j < 2 * (i / 2 + 1); ++j) acc += M[i * 2 * NS + j] * U[j];
    S[i] = acc;
  }
}

// Inclusive scan over the workgroup: on return S of thread p is sum over q <= p of M_0^(p - q) S_q, M = the table from
// the level whose span is one thread.  Step k takes the state of thread t - 2^k: for 2^k < 64 by a shuffle within the
// wave, and for the lanes whose source lies in the wave to the left from the exchange, where the upper half of every
// wave has put its states (slot 32 wave + lane - 32); for 2^k >= 64 from the exchange alone (slot t).  Every thread of
// the workgroup must call it (barriers inside).
template <int NS>
__device__ __forceinline__ void scan_states(double (&S)[2 * NS], const double* __restrict__ M, double* xch, const int t) {
  constexpr int D = 2 * NS;
  const int lane = t & 63, wave = t >> 6;
  double U[D];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = 1 << k;
    __syncthreads();  // the step before has read the exchange
    if (k < 6) {
      if (lane >= 32 && wave < DT / 64 - 1) {
#pragma unroll
        for (int c = 0; c < D; ++c) xch[c * SXW + wave * 32 + lane - 32] = S[c];
      }
    } else if (t < SXW) {
#pragma unroll
      for (int c = 0; c < D; ++c) xch[c * SXW + t] = S[c];
    }
    __syncthreads();
    if (k < 6) {
#pragma unroll
      for (int c = 0; c < D; ++c) U[c] = __shfl_up(S[c], (unsigned)o, 64);
      if (lane < o && wave > 0) {  // thread t - o is lane 64 - o + lane (>= 32) of the wave to the left
#pragma unroll
        for (int c = 0; c < D; ++c) U[c] = xch[c * SXW + (wave - 1) * 32 + 32 - o + lane];
      }
    } else if (t >= o) {
#pragma unroll
      for (int c = 0; c < D; ++c) U[c] = xch[c * SXW + t - o];
    }
    if (t >= o) combine<NS>(S, U, M + k * SMAT);
  }
}

// Element m of a pass is in[m] (forward) or in[n - 1 - m] (REV); elements past the end read as zero.
template <typename InT, bool REV>
__device__ __forceinline__ void stage_tile(const InT* __restrict__ in, const long long n, const long long m0, double* img,
                                           const int t) {
  for (int q = t; q < DTILE; q += DT) {
    const long long m = m0 + q;
    img[phys(q)] = m < n ? static_cast<double>(in[REV ? n - 1 - m : m]) : 0.0;
  }
}

template <int NS>
__device__ __forceinline__ void run_piece(const SosArg& sos, double (&S)[2 * NS], const double* piece) {
  double s1[NS], s2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) s1[s] = S[2 * s], s2[s] = S[2 * s + 1];
#pragma unroll 8
  for (int i = 0; i < DC; ++i) (void)sos_step<NS>(sos, s1, s2, piece[i]);
#pragma unroll
  for (int s = 0; s < NS; ++s) S[2 * s] = s1[s], S[2 * s + 1] = s2[s];
}

template <typename InT, int NS, bool REV>
__global__ __launch_bounds__(DT) void sos_reduce_kernel(const InT* __restrict__ in, const long long n, const SosArg sos,
                                                        const double* __restrict__ mats, double* __restrict__ E) {
  extern __shared__ double sos_lds[];
  double* img = sos_lds;
  double* xch = sos_lds + SIMG;
  const int t = threadIdx.x;
  stage_tile<InT, REV>(in, n, (long long)blockIdx.x * DTILE, img, t);
  __syncthreads();
  double S[2 * NS];
#pragma unroll
  for (int c = 0; c < 2 * NS; ++c) S[c] = 0.0;
  run_piece<NS>(sos, S, img + phys(t * DC));
  scan_states<NS>(S, mats, xch, t);
  if (t == DT - 1) {
#pragma unroll
    for (int c = 0; c < 2 * NS; ++c) E[(size_t)blockIdx.x * SD + c] = S[c];
  }
}

// Z[t + 1] = A^DTILE Z[t] + E[t] for t < ne; Z[0] is the caller's (zero).  One workgroup.
template <int NS>
__global__ __launch_bounds__(DT) void sos_carry_kernel(const double* __restrict__ E, const long long ne,
                                                       const double* __restrict__ mats, double* __restrict__ Z) {
  extern __shared__ double sos_lds[];
  double* xch = sos_lds;
  double* last = sos_lds + SD * SXW;
  const int t = threadIdx.x;
  const double* M = mats + 8 * SMAT;  // M[0] = A^DTILE
  double C[2 * NS];
#pragma unroll
  for (int c = 0; c < 2 * NS; ++c) C[c] = 0.0;
  for (long long base = 0; base < ne; base += DT) {
    const long long tt = base + t;
    double S[2 * NS];
#pragma unroll
    for (int c = 0; c < 2 * NS; ++c) S[c] = tt < ne ? E[tt * SD + c] : 0.0;
    if (t == 0) combine<NS>(S, C, M);
    scan_states<NS>(S, M, xch, t);
    if (tt < ne) {
#pragma unroll
      for (int c = 0; c < 2 * NS; ++c) Z[(tt + 1) * SD + c] = S[c];
    }
    __syncthreads();
    if (t == DT - 1) {
#pragma unroll
      for (int c = 0; c < 2 * NS; ++c) last[c] = S[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2 * NS; ++c) C[c] = last[c];
  }
}

// Result at element m of the pass goes to out[m] (forward) or out[n - 1 - m] (REV).
template <typename InT, typename OutT, int NS, bool REV>
__global__ __launch_bounds__(DT) void sos_apply_kernel(const InT* __restrict__ in, const long long n, const SosArg sos,
                                                       const double* __restrict__ mats, const double* __restrict__ Z,
                                                       OutT* __restrict__ out) {
  extern __shared__ double sos_lds[];
  double* img = sos_lds;
  double* xch = sos_lds + SIMG;
  const int t = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * DTILE;  // m0 < n by the grid size
  stage_tile<InT, REV>(in, n, m0, img, t);
  __syncthreads();
  double S[2 * NS], Z0[2 * NS];
#pragma unroll
  for (int c = 0; c < 2 * NS; ++c) S[c] = Z0[c] = t == 0 ? Z[(size_t)blockIdx.x * SD + c] : 0.0;
  double* piece = img + phys(t * DC);
  run_piece<NS>(sos, S, piece);
  scan_states<NS>(S, mats, xch, t);  // S: the true state behind this thread's piece
  // ---- the state ahead of the piece: the left neighbour's S (across a wave boundary through LDS), the tile's for thread 0
  __syncthreads();
  if ((t & 63) == 63 && t < SXW) {
#pragma unroll
    for (int c = 0; c < 2 * NS; ++c) xch[c * SXW + t] = S[c];
  }
  __syncthreads();
  double s1[NS], s2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    double a = __shfl_up(S[2 * s], 1u, 64), b = __shfl_up(S[2 * s + 1], 1u, 64);
    if ((t & 63) == 0) {
      a = t == 0 ? Z0[2 * s] : xch[(2 * s) * SXW + t - 1];
      b = t == 0 ? Z0[2 * s + 1] : xch[(2 * s + 1) * SXW + t - 1];
    }
    s1[s] = a, s2[s] = b;
  }
  double r[DC];
#pragma unroll
  for (int i = 0; i < DC; ++i) r[i] = sos_step<NS>(sos, s1, s2, piece[i]);
#pragma unroll
  for (int i = 0; i < DC; ++i) piece[i] = r[i];  // a thread's own piece: nobody else reads it
  __syncthreads();
  for (int q = t; q < DTILE; q += DT) {
    const long long m = m0 + q;
    if (m < n) out[REV ? n - 1 - m : m] = static_cast<OutT>(img[phys(q)]);
  }
}

struct PassKernels {
  const void *reduce, *apply;
};

template <typename InT, typename OutT, bool REV>
PassKernels pass_kernels(int ns) {
  switch (ns) {
    case 1: return {(const void*)sos_reduce_kernel<InT, 1, REV>, (const void*)sos_apply_kernel<InT, OutT, 1, REV>};
    case 2: return {(const void*)sos_reduce_kernel<InT, 2, REV>, (const void*)sos_apply_kernel<InT, OutT, 2, REV>};
    case 3: return {(const void*)sos_reduce_kernel<InT, 3, REV>, (const void*)sos_apply_kernel<InT, OutT, 3, REV>};
    default: return {(const void*)sos_reduce_kernel<InT, 4, REV>, (const void*)sos_apply_kernel<InT, OutT, 4, REV>};
  }
}

template <typename OutT>
PassKernels first_pass_kernels(int in_kind, int ns) {
  if (in_kind == VP_SAMPLES_INT32) return pass_kernels<int, OutT, false>(ns);
  if (in_kind == VP_SAMPLES_FLOAT32) return pass_kernels<float, OutT, false>(ns);
  return pass_kernels<double, OutT, false>(ns);
}

const void* carry_kernel(int ns) {
  switch (ns) {
    case 1: return (const void*)sos_carry_kernel<1>;
    case 2: return (const void*)sos_carry_kernel<2>;
    case 3: return (const void*)sos_carry_kernel<3>;
    default: return (const void*)sos_carry_kernel<4>;
  }
}

// ---- detrend
__device__ __forceinline__ void reduce_pair(double& a0, double& a1, double* red, const int t) {
  red[t] = a0;
  red[DT + t] = a1;
  for (int o = DT / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (t < o) {
      red[t] += red[t + o];
      red[DT + t] += red[DT + t + o];
    }
  }
  __syncthreads();
  a0 = red[0];
  a1 = red[DT];
}

// part[2 b], part[2 b + 1]: sum of x and of (i - (n - 1) / 2) x over tile b
template <typename InT>
__global__ __launch_bounds__(DT) void detrend_partial_kernel(const InT* __restrict__ in, const long long n,
                                                             double* __restrict__ part) {
  __shared__ double red[2 * DT];
  const int t = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * DTILE;
  const double centre = 0.5 * (double)(n - 1);
  double a0 = 0.0, a1 = 0.0;
  for (int i = 0; i < DC; ++i) {
    const long long m = m0 + i * DT + t;
    if (m < n) {
      const double v = static_cast<double>(in[m]);
      a0 += v;
      a1 += ((double)m - centre) * v;
    }
  }
  reduce_pair(a0, a1, red, t);
  if (t == 0) part[2 * (size_t)blockIdx.x] = a0, part[2 * (size_t)blockIdx.x + 1] = a1;
}

// prm[0], prm[1]: what detrend_apply_kernel subtracts.  One workgroup.
template <typename InT>
__global__ __launch_bounds__(DT) void detrend_final_kernel(const InT* __restrict__ in, const long long n,
                                                           const double* __restrict__ part, const long long nb, const int type,
                                                           double* __restrict__ prm) {
  __shared__ double red[2 * DT];
  const int t = threadIdx.x;
  if (type == VP_DETREND_SIMPLE) {
    if (t == 0) {
      const double x0 = static_cast<double>(in[0]);
      prm[0] = x0;
      prm[1] = static_cast<double>(in[n - 1]) - x0;
    }
    return;
  }
  double a0 = 0.0, a1 = 0.0;
  for (long long b = t; b < nb; b += DT) a0 += part[2 * b], a1 += part[2 * b + 1];
  reduce_pair(a0, a1, red, t);
  if (t == 0) {
    const double dn = (double)n;
    prm[0] = a0 / dn;
    prm[1] = type == VP_DETREND_LINEAR ? a1 / (dn * (dn * dn - 1.0) / 12.0) : 0.0;  // sum of (i - centre)^2
  }
}

template <typename InT>
__global__ __launch_bounds__(DT) void detrend_apply_kernel(const InT* __restrict__ in, const long long n, const int type,
                                                           const double* __restrict__ prm, float* __restrict__ out) {
  const long long m = (long long)blockIdx.x * DT + threadIdx.x;
  if (m >= n) return;
  const double v = static_cast<double>(in[m]);
  const double p0 = prm[0], p1 = prm[1];
  double line;
  if (type == VP_DETREND_SIMPLE)
    line = p0 + (double)m * p1 / (double)(n - 1);
  else if (type == VP_DETREND_LINEAR)
    line = p0 + p1 * ((double)m - 0.5 * (double)(n - 1));
  else
    line = p0;
  out[m] = static_cast<float>(v - line);
}

template <typename InT>
hipError_t launch_detrend(const InT* in, long long n, int type, double* part, double* prm, float* out, hipStream_t s) {
  const long long nb = (n + DTILE - 1) / DTILE;
  if (type != VP_DETREND_SIMPLE) {
    hipLaunchKernelGGL(detrend_partial_kernel<InT>, dim3((unsigned)nb), dim3(DT), 0, s, in, n, part);
  }
  hipLaunchKernelGGL(detrend_final_kernel<InT>, dim3(1), dim3(DT), 0, s, in, n, (const double*)part, nb, type, prm);
  hipLaunchKernelGGL(detrend_apply_kernel<InT>, dim3((unsigned)((n + DT - 1) / DT)), dim3(DT), 0, s, in, n, type,
                     (const double*)prm, out);
  return hipGetLastError();
}

// Per device, grow-only, reused from call to call: the matrix table, E and Z, the float64 intermediate of a zero-phase
// call; a detrend's partial sums.
DeviceScratch<1>& sos_scratch(int device) {
  static DeviceScratch<1> pool[64];
  return pool[(unsigned)device % 64];
}
int grow_scratch(const char* who, DeviceScratch<1>& sc, size_t bytes, void** out) {
  return sc.b[0].grow(who, bytes, bytes / 8 + 4096, out);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

struct Plan {
  SosArg arg;
  int ns;
  double mats[SLEV * SMAT];
  PassKernels first, first_final, second;  // first pass into the float64 intermediate / into out; the reversed pass
  const void* carry;
};

int make_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
              const float* out_dev, Plan* plan) {
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
  VP_REQUIRE(sos, "%s: null argument", who);
  VP_REQUIRE(n == 0 || (in_dev && out_dev), "%s: null argument", who);
  double r = 0.0;
  if (const int rc = load_sos(who, sos, n_sections, &plan->arg, &r)) return rc;
  VP_REQUIRE(r < 1.0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  VP_REQUIRE(n == 0 || !overlap(in_dev, (size_t)n * elem_bytes(in_kind), out_dev, (size_t)n * sizeof(float)),
             "%s: out_dev overlaps in_dev", who);
  plan->ns = n_sections;
  sosmat::doubling_matrices(sos, n_sections, 5, SLEV, plan->mats);  // DC == 2^5
  plan->first = first_pass_kernels<double>(in_kind, n_sections);
  plan->first_final = first_pass_kernels<float>(in_kind, n_sections);
  plan->second = pass_kernels<double, float, true>(n_sections);
  plan->carry = carry_kernel(n_sections);
  return VP_OK;
}

int prepare_kernels(const Plan& plan, bool zerophase) {
  const PassKernels* used[2] = {zerophase ? &plan.first : &plan.first_final, zerophase ? &plan.second : nullptr};
  for (const PassKernels* k : used) {
    if (!k) continue;
    VP_HIP(hipFuncSetAttribute(k->reduce, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SLDS_BYTES));
    VP_HIP(hipFuncSetAttribute(k->apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SLDS_BYTES));
  }
  return VP_OK;
}

// Where a call's arrays lie in the scratch.
struct Layout {
  double *mats, *Z, *E, *f;
  static size_t bytes(long long n, bool zerophase) {
    const size_t nt = (size_t)((n + DTILE - 1) / DTILE);
    return sizeof(double) * ((size_t)SLEV * SMAT + 2 * nt * SD + (zerophase ? (size_t)n : 0));
  }
  Layout(void* p, long long n) {
    const size_t nt = (size_t)((n + DTILE - 1) / DTILE);
    mats = (double*)p;
    Z = mats + SLEV * SMAT;
    E = Z + nt * SD;
    f = E + nt * SD;
  }
};

hipError_t launch_carry(const Plan& plan, const Layout& L, long long ne, hipStream_t s) {
  const double* E = L.E;
  const double* mats = L.mats;
  double* Z = L.Z;
  void* args[] = {&E, &ne, &mats, &Z};
  return hipLaunchKernel(plan.carry, dim3(1), dim3(DT), args, SCARRY_LDS_BYTES, s);
}

// One pass: reduce over every tile but the last, carry, apply.  Z[0] is zero already.
hipError_t launch_pass(const Plan& plan, const PassKernels& k, const Layout& L, const void* in, long long n, void* out,
                       hipStream_t s) {
  SosArg arg = plan.arg;
  const double* mats = L.mats;
  const long long nt = (n + DTILE - 1) / DTILE;
  if (nt > 1) {
    double* E = L.E;
    void* args[] = {&in, &n, &arg, &mats, &E};
    hipError_t e = hipLaunchKernel(k.reduce, dim3((unsigned)(nt - 1)), dim3(DT), args, SLDS_BYTES, s);
    if (e != hipSuccess) return e;
    e = launch_carry(plan, L, nt - 1, s);
    if (e != hipSuccess) return e;
  }
  const double* Z = L.Z;
  void* args[] = {&in, &n, &arg, &mats, &Z, &out};
  return hipLaunchKernel(k.apply, dim3((unsigned)nt), dim3(DT), args, SLDS_BYTES, s);
}

hipError_t launch_filter(const Plan& plan, const Layout& L, const void* in, long long n, bool zerophase, float* out,
                         hipStream_t s) {
  if (!zerophase) return launch_pass(plan, plan.first_final, L, in, n, out, s);
  const hipError_t e = launch_pass(plan, plan.first, L, in, n, L.f, s);
  return e != hipSuccess ? e : launch_pass(plan, plan.second, L, L.f, n, out, s);
}

hipError_t upload_tables(const Plan& plan, const Layout& L, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(L.mats, plan.mats, sizeof(plan.mats), hipMemcpyHostToDevice, s);
  return e != hipSuccess ? e : hipMemsetAsync(L.Z, 0, SD * sizeof(double), s);
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_sos_filter(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                             int zerophase, float* out_dev) {
  Plan plan;
  if (const int rc = make_plan("vp_sos_filter", in_dev, in_kind, n, sos, n_sections, out_dev, &plan)) return rc;
  VP_REQUIRE(device_id >= 0, "vp_sos_filter: device index");
  if (n == 0) return VP_OK;
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels(plan, zerophase != 0)) return rc;
  hipStream_t s = nullptr;  // the null stream, one synchronisation at the end: as vp_decimate_lowpass
  DeviceScratch<1>& sc = sos_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  if (const int rc = grow_scratch("vp_sos_filter", sc, Layout::bytes(n, zerophase != 0), &p)) return rc;
  const Layout L(p, n);
  VP_HIP(upload_tables(plan, L, s));
  VP_HIP(launch_filter(plan, L, in_dev, (long long)n, zerophase != 0, out_dev, s));
  VP_HIP(hipStreamSynchronize(s));
  return VP_OK;
}

extern "C" int vp_sos_filter_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_sos_filter_release_scratch", sos_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_sos_filter_bench(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos,
                                   int n_sections, int zerophase, float* out_dev, int iters, float* ms_total,
                                   float* ms_carry) {
  VP_REQUIRE(ms_total && iters > 0 && n > 0, "vp_sos_filter_bench: bad argument");
  Plan plan;
  if (const int rc = make_plan("vp_sos_filter_bench", in_dev, in_kind, n, sos, n_sections, out_dev, &plan)) return rc;
  VP_REQUIRE(device_id >= 0, "vp_sos_filter_bench: device index");
  VP_HIP(hipSetDevice(device_id));
  if (const int rc = prepare_kernels(plan, zerophase != 0)) return rc;
  DeviceScratch<1>& sc = sos_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  if (const int rc = grow_scratch("vp_sos_filter_bench", sc, Layout::bytes(n, zerophase != 0), &p)) return rc;
  const Layout L(p, n);
  BenchTimer t;
  VP_HIP(t.init());
  VP_HIP(upload_tables(plan, L, t.s));
  const long long ne = (n + DTILE - 1) / DTILE - 1;
  const auto filter = [&] { return launch_filter(plan, L, in_dev, (long long)n, zerophase != 0, out_dev, t.s); };
  float t_all = 0.f, t_carry = 0.f;
  VP_HIP(t.run(3, filter));
  VP_HIP(t.time(iters, filter, &t_all));
  if (ne > 0)  // one pass's carry launch alone, over the E the last pass left
    VP_HIP(t.time(iters, [&] { return launch_carry(plan, L, ne, t.s); }, &t_carry));
  *ms_total = t_all;
  if (ms_carry) *ms_carry = t_carry;
  return VP_OK;
}

extern "C" int vp_detrend(int device_id, const void* in_dev, int in_kind, int64_t n, int type, float* out_dev) {
  if (const int rc = check_sample_kind("vp_detrend", in_kind)) return rc;
  VP_REQUIRE(type == VP_DETREND_DEMEAN || type == VP_DETREND_LINEAR || type == VP_DETREND_SIMPLE,
             "vp_detrend: type %d is none of VP_DETREND_DEMEAN / LINEAR / SIMPLE", type);
  VP_REQUIRE(n >= 0, "vp_detrend: n = %lld is negative", (long long)n);
  VP_REQUIRE(type == VP_DETREND_DEMEAN || n >= 2, "vp_detrend: a line needs two samples, n = %lld", (long long)n);
  VP_REQUIRE(device_id >= 0, "vp_detrend: device index");
  if (n == 0) return VP_OK;
  VP_REQUIRE(in_dev && out_dev, "vp_detrend: null argument");
  VP_REQUIRE(!overlap(in_dev, (size_t)n * elem_bytes(in_kind), out_dev, (size_t)n * sizeof(float)),
             "vp_detrend: out_dev overlaps in_dev");
  VP_HIP(hipSetDevice(device_id));
  hipStream_t s = nullptr;
  DeviceScratch<1>& sc = sos_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  const size_t nb = (size_t)((n + DTILE - 1) / DTILE);
  if (const int rc = grow_scratch("vp_detrend", sc, sizeof(double) * (2 + 2 * nb), &p)) return rc;
  double* prm = (double*)p;
  double* part = prm + 2;
  if (in_kind == VP_SAMPLES_INT32)
    VP_HIP(launch_detrend((const int*)in_dev, (long long)n, type, part, prm, out_dev, s));
  else if (in_kind == VP_SAMPLES_FLOAT32)
    VP_HIP(launch_detrend((const float*)in_dev, (long long)n, type, part, prm, out_dev, s));
  else
    VP_HIP(launch_detrend((const double*)in_dev, (long long)n, type, part, prm, out_dev, s));
  VP_HIP(hipStreamSynchronize(s));
  return VP_OK;
}
