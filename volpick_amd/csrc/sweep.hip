// The threshold sweep of the reference's task 0 (volpick/model/eval_taks0.py:46-56, :96-142, :497-518) on probabilities
// that are already on the device: for window b, its border [lo, hi), phase ph (0 = P, 1 = S) and EVERY threshold pair j of
// the launch
//   count[b][ph][j]        the triggers of ObsPy's trigger_onset(x[lo:hi], thr_on[j], thr_off[j]): one per run of
//                          consecutive samples > thr_off that holds a sample > thr_on, runs cut at the border;
//   peak[b][ph][j][0..K)   per trigger the first argmax of [first sample > thr_on of the run, run end], relative to lo,
//                          ascending; the first K triggers; -1 from slot `count` on;
//   value[b][ph][j][0..K)  the maxima (0 from slot `count` on), when asked for.
// Every comparison is a strict fp32 `>`, so a NaN ends a run and never is a maximum.
//
// One workgroup of SW_NTH threads per window, the phases one after the other.  A row's border slice is read from memory
// once, coalesced, into LDS; thread t then owns the samples [t C, (t + 1) C) and keeps them in registers for all NT
// thresholds (C = 13 up to T = 3328, else 25: odd, so that the threads' strided LDS reads fall into distinct banks).  The
// thresholds are taken SW_JB at a time, so that the scans of a group -- chains of dependent shuffles -- overlap and share
// their two barriers.  Per threshold:
//   1. every thread walks its samples from "outside a run": the runs that end in its chunk and have their own sample
//      > thr_on are its triggers whatever entered; whether the FIRST run that ends here is one as well depends on what
//      entered.  The walk also summarises the chunk as a function of the run state at its left edge (Elem below);
//   2. an inclusive scan of those functions -- __shfl_up inside the wave, an LDS step across the four waves -- gives every
//      thread the state that enters its chunk, however long the run: a run over the whole border costs what any other row
//      costs.  That settles the thread's trigger count; an exclusive scan of the counts numbers the triggers in sample
//      order (a run that touches the border's end ends there);
//   3. threads that have triggers walk again, from the entering state and out of LDS, and store them; slots past the
//      count are filled.
// No atomics, and the order of the combination is fixed: the same input gives the same bits.
//
// What bounds it: vector instruction issue, not the 2 (hi - lo) 4 bytes a window reads (about 1,900 vector instructions per
// group and wave with 13-sample chunks, four SIMD cycles each, four waves per SIMD at B = 1024).  Per group of three thresholds a thread
// walks C samples three times without a branch, takes part in 6 x 2 x 3 + 6 x 3 shuffles and two barriers, and -- only
// where it has triggers -- walks its chunk again out of LDS.  Measured (tools/sweep_timing.py, B = 1024, NT = 9, K = 8):
// 85 us for PhaseNet's and 151 us for EQTransformer's windows, about twenty times the byte floor and a quarter and an
// eighth of the forward pass of the same batch; 1.3 times that when every row is one run over the whole border (one thread
// then stores for every threshold).
#include <cmath>

#include "predict.h"
#include "sweep.h"

namespace vp {
namespace {

constexpr int SW_WAVES = SW_NTH / 64;
constexpr int SW_JB = 3;  // thresholds in flight
// Flags above the 16 bits of a border index (SW_MAX_T < 65536): inside a run; the run has had a sample > thr_on (then `mx`
// is the maximum from that sample on and the index where it is); and, of a stretch, every sample is > thr_off.
enum { F_RUN = 1 << 16, F_ON = 1 << 17, F_ALL = 1 << 18, ARG_MASK = 0xffff };
static_assert(SW_MAX_T <= ARG_MASK, "a border index and the flags share a word");

// The state of the run a sample sits in -- and, with F_ALL, a stretch of samples as a function of the state that enters it:
// with F_ALL the entering run goes on through the stretch, without it the run that leaves is this one whatever entered.
// (A stretch needs no maximum of its own: when the entering run has had its sample > thr_on, its maximum is above thr_on,
// and so above every sample in front of the stretch's first one > thr_on.)
struct Elem {
  float mx;
  int fa;  // flags | index
};

// a, then b.
__device__ __forceinline__ Elem combine(const Elem& a, const Elem& b) {
  if (!(b.fa & F_ALL)) return b;
  // (strict >: the earlier of equal maxima stays.  A thread past the border's end has no samples and is F_ALL with no run:
  // it drops a run without F_ON here, and nothing reads what follows it.)
  const bool take_b = !(a.fa & F_ON) || ((b.fa & F_ON) && b.mx > a.mx);
  Elem r;
  r.mx = take_b ? b.mx : a.mx;
  r.fa = ((take_b ? b.fa : a.fa) & ~F_ALL) | (a.fa & F_ALL);
  return r;
}

__device__ __forceinline__ Elem shfl_up(const Elem& e, int d) {
  return Elem{__shfl_up(e.mx, d, 64), __shfl_up(e.fa, d, 64)};
}

// The thread's C samples (border indices g0 ...; -inf behind the border's end, which ends a run as the border does) walked
// from outside a run, without a branch: `count` the runs that end here with their own sample > on, s the state that leaves.
// `last`: the chunk holds the border's last sample, where an open run ends.  Returns F_ALL if every sample was > off, and
// F_ON if the first run to end here (if any does) was counted.
template <int C>
__device__ __forceinline__ int summarise(const float (&x)[C], int g0, bool last, float on, float off, Elem& s, int& count) {
  bool all = true, first = false;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const float v = x[k];
    const bool above = v > off, had_on = (s.fa & F_ON) != 0;
    const bool ends = !above && had_on;
    count += ends;
    first |= ends && all;
    all &= above;
    const bool top = above && (had_on ? v > s.mx : v > on);
    s.mx = top ? v : s.mx;
    s.fa = above ? (top ? (F_RUN | F_ON | (g0 + k)) : (s.fa | F_RUN)) : 0;
  }
  if (last && (s.fa & F_ON)) {
    ++count;
    first |= all;
  }
  return (all ? F_ALL : 0) | (first ? F_ON : 0);
}

// The same walk from the state s that enters the chunk, over its m samples in LDS, for the threads that have triggers:
// the first `todo` of them stored from `slot` on.
__device__ __forceinline__ void store_triggers(const float* chunk, int m, int g0, bool last, float on, float off, Elem s, int todo,
                                               int* peak, float* value) {
  for (int k = 0; k < m && todo > 0; ++k) {
    const float v = chunk[k];
    if (v > off) {
      if (s.fa & F_ON ? v > s.mx : v > on) s.mx = v, s.fa = F_RUN | F_ON | (g0 + k);
    } else {
      if (s.fa & F_ON) {
        *peak++ = s.fa & ARG_MASK;
        if (value) *value++ = s.mx;
        --todo;
      }
      s.fa = 0;
    }
  }
  if (todo > 0 && last && (s.fa & F_ON)) {
    *peak = s.fa & ARG_MASK;
    if (value) *value = s.mx;
  }
}

template <int C>
__global__ __launch_bounds__(SW_NTH) void sweep_windows_kernel(const SweepArgs a) {
  __shared__ float row[SW_NTH * C];
  __shared__ float tot_mx[SW_JB][SW_WAVES];
  __shared__ int tot_fa[SW_JB][SW_WAVES], tot_n[SW_JB][SW_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = a.lo ? a.lo[b] : 0;
  const int n = (a.hi ? a.hi[b] : a.T) - lo;  // 1 <= n <= T <= SW_NTH * C (sweep_check, sweep_launch)
  const int g0 = tid * C;
  const int m = min(max(n - g0, 0), C);
  const bool last = m > 0 && g0 + m == n;

  for (int ph = 0; ph < 2; ++ph) {
    const float* p = a.prob + ((long long)b * a.n_rows + (ph ? a.s_row : a.p_row)) * a.T + lo;
    __syncthreads();  // (the other phase's row has been taken into registers everywhere)
    for (int i = tid; i < n; i += SW_NTH) row[i] = p[i];
    __syncthreads();
    float x[C];
#pragma unroll
    for (int k = 0; k < C; ++k) x[k] = k < m ? row[g0 + k] : -INFINITY;

#pragma unroll 1
    for (int j0 = 0; j0 < a.NT; j0 += SW_JB) {
      // a group's thresholds; behind the last one: +inf, above which nothing is
      float on[SW_JB], off[SW_JB];
#pragma unroll
      for (int g = 0; g < SW_JB; ++g) {
        on[g] = j0 + g < a.NT ? a.thr_on[j0 + g] : INFINITY;
        off[g] = j0 + g < a.NT ? a.thr_off[j0 + g] : INFINITY;
      }
      // ---- 1. this thread's samples from outside a run -----------------------------------------------------------------------
      Elem e[SW_JB];
      int mine[SW_JB], ends[SW_JB];  // triggers whatever enters; F_ALL / F_ON of the walk
#pragma unroll
      for (int g = 0; g < SW_JB; ++g) {
        e[g] = Elem{0.f, 0};
        mine[g] = 0;
        ends[g] = summarise<C>(x, g0, last, on[g], off[g], e[g], mine[g]);
        e[g].fa |= ends[g] & F_ALL;
      }
      // ---- 2. the run state that enters them; the triggers numbered -----------------------------------------------------------
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        Elem o[SW_JB];
#pragma unroll
        for (int g = 0; g < SW_JB; ++g) o[g] = shfl_up(e[g], d);
#pragma unroll
        for (int g = 0; g < SW_JB; ++g)
          if (lane >= d) e[g] = combine(o[g], e[g]);
      }
      if (lane == 63) {
#pragma unroll
        for (int g = 0; g < SW_JB; ++g) tot_mx[g][wave] = e[g].mx, tot_fa[g][wave] = e[g].fa;
      }
      __syncthreads();
      Elem in[SW_JB];
      int upto[SW_JB];
#pragma unroll
      for (int g = 0; g < SW_JB; ++g) {
        Elem pre{0.f, 0};  // in front of the border: outside a run
        for (int w = 0; w < wave; ++w) pre = combine(pre, Elem{tot_mx[g][w], tot_fa[g][w]});
        const Elem left = shfl_up(e[g], 1);
        in[g] = lane == 0 ? pre : combine(pre, left);
        // the first run that ends here, if it was not a trigger by itself, is one when what enters has had its sample
        // (a thread past the border's end ends nothing: the border's last thread has done that)
        const bool ends_one = m > 0 && (!(ends[g] & F_ALL) || last);
        if ((in[g].fa & F_ON) && ends_one && !(ends[g] & F_ON)) ++mine[g];
        upto[g] = mine[g];
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int g = 0; g < SW_JB; ++g) {
          const int o = __shfl_up(upto[g], d, 64);
          if (lane >= d) upto[g] += o;
        }
      }
      if (lane == 63) {
#pragma unroll
        for (int g = 0; g < SW_JB; ++g) tot_n[g][wave] = upto[g];
      }
      __syncthreads();

      // ---- 3. store ---------------------------------------------------------------------------------------------------------
#pragma unroll
      for (int g = 0; g < SW_JB; ++g) {
        if (j0 + g < a.NT) {
          int slot = upto[g] - mine[g], total = 0;
          for (int w = 0; w < SW_WAVES; ++w) {
            if (w < wave) slot += tot_n[g][w];
            total += tot_n[g][w];
          }
          const long long at = (((long long)b * 2 + ph) * a.NT + j0 + g);
          int* peak = a.peak + at * a.K;
          float* value = a.value ? a.value + at * a.K : nullptr;
          if (mine[g] > 0 && slot < a.K)
            store_triggers(row + g0, m, g0, last, on[g], off[g], Elem{in[g].mx, in[g].fa & ~F_ALL}, min(mine[g], a.K - slot),
                           peak + slot, value ? value + slot : nullptr);
          if (tid < a.K && tid >= total) {
            peak[tid] = -1;
            if (value) value[tid] = 0.f;
          }
          if (tid == 0) a.count[at] = total;
        }
      }
    }
  }
}

}  // namespace

int sweep_check(int B, int n_rows, int T, int p_row, int s_row, const int32_t* lo, const int32_t* hi, const float* thr_on,
                const float* thr_off, int NT, int K, const char* who) {
  VP_REQUIRE(thr_on && thr_off, "%s: null thresholds", who);
  VP_REQUIRE(B >= 1, "%s: B = %d", who, B);
  VP_REQUIRE(T >= 1 && T <= SW_MAX_T, "%s: T = %d outside [1, %d], the border the kernel's LDS row holds", who, T, SW_MAX_T);
  VP_REQUIRE(NT >= 1 && NT <= SW_MAX_NT, "%s: NT = %d outside [1, %d]", who, NT, SW_MAX_NT);
  VP_REQUIRE(K >= 1 && K <= SW_MAX_K, "%s: K = %d outside [1, %d]", who, K, SW_MAX_K);
  VP_REQUIRE(n_rows >= 2 && n_rows <= 64, "%s: n_rows = %d outside [2, 64]", who, n_rows);
  for (int r : {p_row, s_row}) VP_REQUIRE(r >= 0 && r < n_rows, "%s: row %d outside [0, %d)", who, r, n_rows);
  VP_REQUIRE(p_row != s_row, "%s: p_row and s_row are both %d", who, p_row);
  for (int j = 0; j < NT; ++j) {
    VP_REQUIRE(std::isfinite(thr_on[j]) && std::isfinite(thr_off[j]), "%s: threshold %d is not finite", who, j);
    VP_REQUIRE(thr_off[j] <= thr_on[j], "%s: threshold %d: thr_off = %g exceeds thr_on = %g", who, j, (double)thr_off[j],
               (double)thr_on[j]);
  }
  return border_check(B, T, lo, hi, who);
}

int sweep_launch(const SweepArgs& a, hipStream_t s) {
  if (a.T <= SW_NTH * 13) {
    hipLaunchKernelGGL(sweep_windows_kernel<13>, dim3(a.B), dim3(SW_NTH), 0, s, a);
  } else {
    hipLaunchKernelGGL(sweep_windows_kernel<SW_MAX_CHUNK>, dim3(a.B), dim3(SW_NTH), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("sweep_windows_kernel launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

}  // namespace vp
