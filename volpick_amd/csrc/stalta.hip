// STA/LTA characteristic functions of device-resident series and the triggers cut from them (include/volpick_hip.h,
// vp_sta_lta, vp_trigger_onset): ObsPy's classic_sta_lta / recursive_sta_lta / trigger_onset, which volpick_amd/trigger.py
// restates on the host.  Input int32 / float32 / float64; every sum, state and quotient float64; output float32 or
// float64, rounded once at the store.  A series is cut into tiles of DTILE = 8192 samples and pieces of DC = 32, one
// piece per thread (sos_tile.h), and every term of every sum here is a square: non-negative, so no sum cancels.
//
// Recursive type.  Each state is s <- a s + c x^2 (a = 1 - c), the 1 x 1 case of the filter state of sosfilt.hip, and is
// carried across every seam the same way: a run of L samples from state s0 ends in a^L s0 + (its end from zero state).
// The host makes the table a^(32 2^k), k = 0..15 (stalta_host.h), and a call is three launches:
//   reduce  per tile but the last: every thread runs its piece from zero state, a scan over the 256 threads with levels
//           0..7 leaves the tile's zero-state end E_t in the last thread.
//   carry   one workgroup per series: Z_(t+1) = a^8192 Z_t + E_t with levels 8..15, 256 tiles at a time, the chunk's end
//           carried into the next chunk.  Z_0 = (0, tiny): the rule's start value rides the carry.
//   apply   per tile: the pieces again from zero state, thread 0 from Z_t, so the scan leaves the true state behind
//           every piece; every thread runs its piece a second time from its left neighbour's and keeps the 32 quotients.
// Step j of the recurrence reads sample j + 1: sample 0 never enters the sums (cft[0] = 0).
//
// Classic type.  A window sum is never a difference.  For a width w the series is cut into blocks of w samples; P[i] is the
// sum from the left edge of i's block to i, S[i] the sum from i to the right edge of its block, and the window ending at i
// is S[i - w + 1] + P[i] (P[i] alone where the window starts on a block edge or ahead of the series).  Both are segmented
// scans.  A call is four launches:
//   reduce  per tile, for both widths: the sum from the last block edge in the tile (or its start) to its end, the sum from
//           its start to the first block edge (or its end), and the index of its first non-finite sample.
//   carry   one workgroup per series: the segmented scans of those sums over the tiles, forward and backward, 256 tiles at
//           a time, and the first non-finite index of the series.
//   suffix  per tile, right to left: S for both widths into the scratch (0 on a block's left edge, where nobody reads it).
//   final   per tile, left to right: P for both widths, the two window sums, the means and the quotient.
// A window of w samples is summed by at most w - 1 additions of non-negative terms whatever w and the tile.
//
// Order between tiles comes from the launch boundaries alone: no flags, no atomics, no grid barrier; the same call gives
// the same bits every time.  A non-finite sample is read as NaN.  The recursion keeps it in both states through every
// product (0 * NaN is NaN); the classic type, whose windows would leave it behind, writes NaN from the first one on, as
// the whole-trace cumulative sum of the rule does.  This deviates from ObsPy for an Inf: there it stays Inf for the few
// samples until Inf - Inf or Inf / Inf makes it NaN, here those head samples are NaN at once.  Samples ahead of the
// first non-finite one are right either way, and the recursive type never reads sample 0.
#include "api_host.h"  // ScanLayout, collect_rows
#include "device_scratch.h"
#include "prepost.h"  // launch_pick_table
#include "sos_tile.h"
#include "stalta_host.h"

namespace vp {
namespace {

constexpr int TIMG = DTILE / DC * (DC + 1);  // doubles of a tile image
constexpr long long NO_BAD = 0x7fffffffffffffffLL;
static_assert(DT == 256 && DC == STALTA_PIECE, "the scans are written for 256 pieces of 32");

// x^2 of sample m of a series of n, 0 outside it; a non-finite sample reads as NaN
template <typename InT>
__device__ __forceinline__ double square_at(const InT* __restrict__ in, const long long n, const long long m) {
  if (m < 0 || m >= n) return 0.0;
  double v = static_cast<double>(in[m]);
  if (!(v - v == 0.0)) v = __builtin_nan("");
  return v * v;
}

// ---------------------------------------------------------------------------------------------------- recursive type
// Inclusive scan over the workgroup: on return S of thread p is sum over q <= p of a^(span (p - q)) S_q, span the samples
// of level `l0`.  Every thread must call it (barriers inside); xch: 2 DT doubles.
__device__ __forceinline__ void rec_scan(double (&S)[2], const StaLtaRec& r, const int l0, double* xch, const int t) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = 1 << k;
    __syncthreads();  // the step before has read the exchange
    xch[t] = S[0];
    xch[DT + t] = S[1];
    __syncthreads();
    if (t >= o) {
      S[0] = fma(r.pw[0][l0 + k], xch[t - o], S[0]);
      S[1] = fma(r.pw[1][l0 + k], xch[DT + t - o], S[1]);
    }
  }
}

__device__ __forceinline__ void rec_run_piece(const StaLtaRec& r, double (&S)[2], const double* piece) {
  double sta = S[0], lta = S[1];
#pragma unroll 8
  for (int i = 0; i < DC; ++i) {
    const double sq = piece[i];
    sta = r.c[0] * sq + r.a[0] * sta;
    lta = r.c[1] * sq + r.a[1] * lta;
  }
  S[0] = sta, S[1] = lta;
}

// step j of tile `blockIdx.x` reads sample j + 1
template <typename InT>
__device__ __forceinline__ void rec_stage(const InT* __restrict__ in, const long long n, const long long j0, double* img,
                                          const int t) {
  for (int q = t; q < DTILE; q += DT) img[phys(q)] = square_at(in, n, j0 + q + 1);
}

template <typename InT>
__global__ __launch_bounds__(DT) void rec_reduce_kernel(const InT* __restrict__ in, const long long stride, const long long n,
                                                        const long long nt, const StaLtaRec r, double* __restrict__ E) {
  extern __shared__ double st_lds[];
  __shared__ double xch[2 * DT];
  const int t = threadIdx.x;
  rec_stage(in + (size_t)blockIdx.y * stride, n, (long long)blockIdx.x * DTILE, st_lds, t);
  __syncthreads();
  double S[2] = {0.0, 0.0};
  rec_run_piece(r, S, st_lds + phys(t * DC));
  rec_scan(S, r, 0, xch, t);
  if (t == DT - 1) {
    double* e = E + 2 * ((size_t)blockIdx.y * nt + blockIdx.x);
    e[0] = S[0], e[1] = S[1];
  }
}

// Z[t + 1] = a^DTILE Z[t] + E[t] for t < nt - 1, Z[0] = (0, tiny).  One workgroup per series.
__global__ __launch_bounds__(DT) void rec_carry_kernel(const double* __restrict__ E, const long long nt, const StaLtaRec r,
                                                       double* __restrict__ Z) {
  __shared__ double xch[2 * DT];
  __shared__ double last[2];
  const int t = threadIdx.x;
  E += 2 * (size_t)blockIdx.x * nt;
  Z += 2 * (size_t)blockIdx.x * nt;
  double C[2] = {0.0, DBL_MIN};
  if (t == 0) Z[0] = C[0], Z[1] = C[1];
  for (long long base = 0; base < nt - 1; base += DT) {
    const long long tt = base + t;
    double S[2];
    S[0] = tt < nt - 1 ? E[2 * tt] : 0.0;
    S[1] = tt < nt - 1 ? E[2 * tt + 1] : 0.0;
    if (t == 0) {
      S[0] = fma(r.pw[0][8], C[0], S[0]);
      S[1] = fma(r.pw[1][8], C[1], S[1]);
    }
    rec_scan(S, r, 8, xch, t);
    if (tt < nt - 1) Z[2 * (tt + 1)] = S[0], Z[2 * (tt + 1) + 1] = S[1];
    __syncthreads();
    if (t == DT - 1) last[0] = S[0], last[1] = S[1];
    __syncthreads();
    C[0] = last[0], C[1] = last[1];
  }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(DT) void rec_apply_kernel(const InT* __restrict__ in, const long long stride, const long long n,
                                                       const long long nt, const long long nlta, const StaLtaRec r,
                                                       const double* __restrict__ Z, OutT* __restrict__ out) {
  extern __shared__ double st_lds[];
  __shared__ double xch[2 * DT];
  const int t = threadIdx.x;
  const long long j0 = (long long)blockIdx.x * DTILE;
  in += (size_t)blockIdx.y * stride;
  out += (size_t)blockIdx.y * stride;
  rec_stage(in, n, j0, st_lds, t);
  __syncthreads();
  double Z0[2] = {0.0, 0.0};
  if (t == 0) {
    if (blockIdx.x == 0) {
      Z0[1] = DBL_MIN;
    } else {
      const double* z = Z + 2 * ((size_t)blockIdx.y * nt + blockIdx.x);
      Z0[0] = z[0], Z0[1] = z[1];
    }
  }
  double S[2] = {Z0[0], Z0[1]};
  double* piece = st_lds + phys(t * DC);
  rec_run_piece(r, S, piece);
  rec_scan(S, r, 0, xch, t);  // S: the true state behind this thread's piece
  __syncthreads();
  xch[t] = S[0];
  xch[DT + t] = S[1];
  __syncthreads();
  double sta = t == 0 ? Z0[0] : xch[t - 1], lta = t == 0 ? Z0[1] : xch[DT + t - 1];
  const long long i0 = j0 + (long long)t * DC + 1;  // the sample of this thread's first step
#pragma unroll 8
  for (int i = 0; i < DC; ++i) {
    const double sq = piece[i];
    sta = r.c[0] * sq + r.a[0] * sta;
    lta = r.c[1] * sq + r.a[1] * lta;
    // 0 / lta is 0 even where lta itself, tiny a^i, has gone under the smallest double
    piece[i] = (i0 + i < nlta || sta == 0.0) ? 0.0 : sta / lta;  // a thread's own piece: nobody else reads it
  }
  __syncthreads();
  for (int q = t; q < DTILE; q += DT) {
    const long long m = j0 + q + 1;
    if (m < n) out[m] = static_cast<OutT>(st_lds[phys(q)]);
  }
  if (blockIdx.x == 0 && t == 0) out[0] = static_cast<OutT>(0.0);
}

// ------------------------------------------------------------------------------------------------------ classic type
// Tile summaries, per (series, tile): 4 sums -- width k (0: nsta, 1: nlta) forward tail at 2 k, backward head at 2 k + 1.
struct Widths {
  int w[2];
};

// The forward tail of tile [a, b): samples [max(a, last block edge <= b), b); whether that edge lies in [a, b].
__device__ __forceinline__ long long tail_start(const long long a, const long long b, const int w, bool* stops) {
  const long long e = b - b % w;
  *stops = e >= a;
  return e >= a ? e : a;
}
// The backward head of tile [a, b): samples [a, min(b, first block edge >= a)); whether that edge lies in [a, b].
__device__ __forceinline__ long long head_end(const long long a, const long long b, const int w, bool* stops) {
  const long long e = (a + w - 1) / w * w;
  *stops = e <= b;
  return e <= b ? e : b;
}

template <typename InT>
__global__ __launch_bounds__(DT) void cls_reduce_kernel(const InT* __restrict__ in, const long long stride, const long long n,
                                                        const long long nt, const Widths wd, double* __restrict__ sums,
                                                        long long* __restrict__ bad) {
  __shared__ double red[4][DT];
  __shared__ long long redb[DT];
  const int t = threadIdx.x;
  const long long a = (long long)blockIdx.x * DTILE, b = a + DTILE;
  in += (size_t)blockIdx.y * stride;
  long long lo[2], hi[2];
  for (int k = 0; k < 2; ++k) {
    bool stops;
    lo[k] = tail_start(a, b, wd.w[k], &stops);
    hi[k] = head_end(a, b, wd.w[k], &stops);
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  long long first = NO_BAD;
  for (int q = t; q < DTILE; q += DT) {
    const long long m = a + q;
    const double sq = square_at(in, n, m);
    if (sq != sq && m < first) first = m;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (m >= lo[k]) acc[2 * k] += sq;
      if (m < hi[k]) acc[2 * k + 1] += sq;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][t] = acc[k];
  redb[t] = first;
  for (int o = DT / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (t < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + o];
      if (redb[t + o] < redb[t]) redb[t] = redb[t + o];
    }
  }
  __syncthreads();
  const size_t tile = (size_t)blockIdx.y * nt + blockIdx.x;
  if (t < 4) sums[4 * tile + t] = red[t][0];
  if (t == 0) bad[tile] = redb[0];
}

// Inclusive segmented scan over the workgroup: an element with `stop` set starts a new sum.  xv: DT doubles, xf: DT ints.
__device__ __forceinline__ void seg_scan(double& v, int& stop, double* xv, int* xf, const int t) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = 1 << k;
    __syncthreads();
    xv[t] = v;
    xf[t] = stop;
    __syncthreads();
    if (t >= o) {
      if (!stop) v = xv[t - o] + v;
      stop |= xf[t - o];
    }
  }
}

// F[t][k]: the sum from the last block edge of width k at or before tile t's start to that start; R[t][k]: the sum from
// tile t's end to the first block edge at or after it; firstbad: the series' first non-finite sample.  One workgroup per
// series.
__global__ __launch_bounds__(DT) void cls_carry_kernel(const double* __restrict__ sums, const long long* __restrict__ bad,
                                                       const long long nt, const Widths wd, double* __restrict__ F,
                                                       double* __restrict__ R, long long* __restrict__ firstbad) {
  __shared__ double xv[DT];
  __shared__ int xf[DT];
  __shared__ long long redb[DT];
  __shared__ double last;
  const int t = threadIdx.x;
  sums += 4 * (size_t)blockIdx.x * nt;
  bad += (size_t)blockIdx.x * nt;
  F += 2 * (size_t)blockIdx.x * nt;
  R += 2 * (size_t)blockIdx.x * nt;
  for (int k = 0; k < 2; ++k) {
    const int w = wd.w[k];
    for (int rev = 0; rev < 2; ++rev) {
      // element e of the scan: tile e forward, tile nt - 1 - e backward; its result belongs to the next tile in that order
      double* dst = rev ? R : F;
      if (t == 0) dst[2 * (rev ? nt - 1 : 0) + k] = 0.0;
      double C = 0.0;
      for (long long base = 0; base < nt - 1; base += DT) {
        const long long e = base + t;
        const bool live = e < nt - 1;
        const long long tile = rev ? nt - 1 - e : e;
        double v = 0.0;
        int stop = 0;
        if (live) {
          bool s;
          const long long a = tile * DTILE;
          if (rev)
            (void)head_end(a, a + DTILE, w, &s);
          else
            (void)tail_start(a, a + DTILE, w, &s);
          stop = s;
          v = sums[4 * tile + 2 * k + rev];
        }
        if (t == 0 && !stop) v = C + v;
        seg_scan(v, stop, xv, xf, t);
        if (live) dst[2 * (rev ? tile - 1 : tile + 1) + k] = v;
        __syncthreads();
        if (t == DT - 1) last = v;
        __syncthreads();
        C = last;
      }
    }
  }
  long long first = NO_BAD;
  for (long long e = t; e < nt; e += DT)
    if (bad[e] < first) first = bad[e];
  redb[t] = first;
  for (int o = DT / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (t < o && redb[t + o] < redb[t]) redb[t] = redb[t + o];
  }
  __syncthreads();
  if (t == 0) firstbad[blockIdx.x] = redb[0];
}

// The segmented running sums of one tile for one width, in the thread's order of work: element q = DC t + i is sample
// a + q (forward, a new sum starts ON a block's left edge) or b - 1 - q (REV, a new sum starts on a block's right edge).
// v: the thread's 32 squares; `carry`: the tile's F or R; loc: the running sum at each element.
template <bool REV>
__device__ __forceinline__ void seg_tile(const double (&v)[DC], const int w, const long long p0, const double carry,
                                         double* xv, int* xf, const int t, double (&loc)[DC]) {
  int r = (int)(p0 % w);  // of element i: (p0 + i) % w forward, (p0 - i) % w backward
  const int edge = REV ? w - 1 : 0;
  double acc = 0.0;
  int first_edge = DC;
#pragma unroll
  for (int i = 0; i < DC; ++i) {
    if (r == edge) {
      acc = 0.0;
      if (first_edge == DC) first_edge = i;
    }
    acc += v[i];
    loc[i] = acc;
    if (REV)
      r = r == 0 ? w - 1 : r - 1;
    else
      r = r == w - 1 ? 0 : r + 1;
  }
  int stop = first_edge < DC;
  seg_scan(acc, stop, xv, xf, t);
  __syncthreads();
  xv[t] = acc;
  xf[t] = stop;
  __syncthreads();
  double ahead = t > 0 ? xv[t - 1] : 0.0;  // the sum that runs into this piece
  if (!(t > 0 && xf[t - 1])) ahead = carry + ahead;
#pragma unroll
  for (int i = 0; i < DC; ++i)
    if (i < first_edge) loc[i] = ahead + loc[i];
}

// S of both widths: Sarr[k][m] = sum of x^2 over [m, right edge of m's block], 0 where m is a block's left edge.
template <typename InT>
__global__ __launch_bounds__(DT) void cls_suffix_kernel(const InT* __restrict__ in, const long long stride, const long long n,
                                                        const long long nt, const Widths wd, const double* __restrict__ R,
                                                        double* __restrict__ S0, double* __restrict__ S1) {
  extern __shared__ double st_lds[];
  __shared__ double xv[DT];
  __shared__ int xf[DT];
  const int t = threadIdx.x;
  const long long a = (long long)blockIdx.x * DTILE, b = a + DTILE;
  in += (size_t)blockIdx.y * stride;
  for (int q = t; q < DTILE; q += DT) st_lds[phys(q)] = square_at(in, n, b - 1 - q);
  __syncthreads();
  double v[DC], loc[DC];
  double* piece = st_lds + phys(t * DC);
#pragma unroll
  for (int i = 0; i < DC; ++i) v[i] = piece[i];
  const long long p0 = b - 1 - (long long)t * DC;
  const double* carry = R + 2 * ((size_t)blockIdx.y * nt + blockIdx.x);
  for (int k = 0; k < 2; ++k) {
    const int w = wd.w[k];
    seg_tile<true>(v, w, p0, carry[k], xv, xf, t, loc);
    int r = (int)(p0 % w);
#pragma unroll
    for (int i = 0; i < DC; ++i) {
      piece[i] = r == 0 ? 0.0 : loc[i];
      r = r == 0 ? w - 1 : r - 1;
    }
    __syncthreads();
    double* dst = (k ? S1 : S0) + (size_t)blockIdx.y * n;
    for (int q = t; q < DTILE; q += DT) {
      const long long m = b - 1 - q;
      if (m < n) dst[m] = st_lds[phys(q)];
    }
    __syncthreads();
  }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(DT) void cls_final_kernel(const InT* __restrict__ in, const long long stride, const long long n,
                                                       const long long nt, const Widths wd, const double* __restrict__ F,
                                                       const double* __restrict__ S0, const double* __restrict__ S1,
                                                       const long long* __restrict__ firstbad, OutT* __restrict__ out) {
  extern __shared__ double st_lds[];  // two tile images: P of nsta, P of nlta
  __shared__ double xv[DT];
  __shared__ int xf[DT];
  const int t = threadIdx.x;
  const long long a = (long long)blockIdx.x * DTILE;
  in += (size_t)blockIdx.y * stride;
  out += (size_t)blockIdx.y * stride;
  for (int q = t; q < DTILE; q += DT) st_lds[phys(q)] = square_at(in, n, a + q);
  __syncthreads();
  double v[DC], loc[DC];
#pragma unroll
  for (int i = 0; i < DC; ++i) v[i] = st_lds[phys(t * DC) + i];
  const long long p0 = a + (long long)t * DC;
  const double* carry = F + 2 * ((size_t)blockIdx.y * nt + blockIdx.x);
  for (int k = 0; k < 2; ++k) {
    seg_tile<false>(v, wd.w[k], p0, carry[k], xv, xf, t, loc);
    double* piece = st_lds + k * TIMG + phys(t * DC);  // image 0 is read by its owner alone from here on
#pragma unroll
    for (int i = 0; i < DC; ++i) piece[i] = loc[i];
  }
  __syncthreads();
  const long long ns = wd.w[0], nl = wd.w[1];
  const long long fb = firstbad[blockIdx.y];
  S0 += (size_t)blockIdx.y * n;
  S1 += (size_t)blockIdx.y * n;
  for (int q = t; q < DTILE; q += DT) {
    const long long i = a + q;
    if (i >= n) break;
    double ws = st_lds[phys(q)], wl = st_lds[TIMG + phys(q)];
    if (i >= ns) ws = S0[i - ns + 1] + ws;
    if (i >= nl) wl = S1[i - nl + 1] + wl;
    double sta = ws / (double)ns, lta = wl / (double)nl;
    if (i < nl - 1) sta = 0.0;
    if (lta < DBL_MIN) lta = DBL_MIN;
    double c = sta / lta;
    if (i >= fb) c = __builtin_nan("");
    out[i] = static_cast<OutT>(c);
  }
}

// --------------------------------------------------------------------------------------------------------- host side
constexpr size_t IMG_BYTES = (size_t)TIMG * sizeof(double);  // 67,584

// Per device, grow-only, reused from call to call.  Block 0: vp_sta_lta's carries and suffix sums; block 1:
// vp_trigger_onset's row table and result block.
DeviceScratch<2>& stalta_scratch(int device) {
  static DeviceScratch<2> pool[64];
  return pool[(unsigned)device % 64];
}

struct Call {
  const void* in;
  void* out;
  int in_kind, out_kind, n_series, type;
  long long stride, n, nt, nsta, nlta;
  StaLtaRec rec;
  Widths wd;
};

// Where a call's arrays lie in block 0.
struct Layout {
  double *E, *Z;                // recursive: 2 doubles per (series, tile) each
  double *sums, *F, *R, *S[2];  // classic: 4, 2, 2 doubles per (series, tile); n per series and width
  long long *bad, *firstbad;
  static size_t bytes(const Call& c) {
    const size_t tiles = (size_t)c.n_series * c.nt;
    if (c.type == VP_STALTA_RECURSIVE) return 8 * (4 * tiles);
    return 8 * (9 * tiles + (size_t)c.n_series + 2 * (size_t)c.n_series * c.n);
  }
  Layout(void* p, const Call& c) {
    const size_t tiles = (size_t)c.n_series * c.nt;
    double* d = (double*)p;
    E = d, Z = d + 2 * tiles;
    sums = d, F = sums + 4 * tiles, R = F + 2 * tiles;
    bad = (long long*)(R + 2 * tiles);
    firstbad = bad + tiles;
    S[0] = (double*)(firstbad + c.n_series);
    S[1] = S[0] + (size_t)c.n_series * c.n;
  }
};

template <typename K>
hipError_t big_lds(K kernel, size_t bytes) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <typename InT, typename OutT>
hipError_t launch_typed(const Call& c, const Layout& L, hipStream_t s) {
  const InT* in = (const InT*)c.in;
  OutT* out = (OutT*)c.out;
  const dim3 tiles((unsigned)c.nt, (unsigned)c.n_series), series((unsigned)c.n_series), wg(DT);
  hipError_t e;
  if (c.type == VP_STALTA_RECURSIVE) {
    if (c.nt > 1) {
      if ((e = big_lds(rec_reduce_kernel<InT>, IMG_BYTES)) != hipSuccess) return e;
      hipLaunchKernelGGL(rec_reduce_kernel<InT>, dim3((unsigned)(c.nt - 1), (unsigned)c.n_series), wg, IMG_BYTES, s, in,
                         c.stride, c.n, c.nt, c.rec, L.E);
      hipLaunchKernelGGL(rec_carry_kernel, series, wg, 0, s, (const double*)L.E, c.nt, c.rec, L.Z);
    }
    if ((e = big_lds(rec_apply_kernel<InT, OutT>, IMG_BYTES)) != hipSuccess) return e;
    hipLaunchKernelGGL((rec_apply_kernel<InT, OutT>), tiles, wg, IMG_BYTES, s, in, c.stride, c.n, c.nt, c.nlta, c.rec,
                       (const double*)L.Z, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(cls_reduce_kernel<InT>, tiles, wg, 0, s, in, c.stride, c.n, c.nt, c.wd, L.sums, L.bad);
  hipLaunchKernelGGL(cls_carry_kernel, series, wg, 0, s, (const double*)L.sums, (const long long*)L.bad, c.nt, c.wd, L.F, L.R,
                     L.firstbad);
  if ((e = big_lds(cls_suffix_kernel<InT>, IMG_BYTES)) != hipSuccess) return e;
  hipLaunchKernelGGL(cls_suffix_kernel<InT>, tiles, wg, IMG_BYTES, s, in, c.stride, c.n, c.nt, c.wd, (const double*)L.R,
                     L.S[0], L.S[1]);
  if ((e = big_lds(cls_final_kernel<InT, OutT>, 2 * IMG_BYTES)) != hipSuccess) return e;
  hipLaunchKernelGGL((cls_final_kernel<InT, OutT>), tiles, wg, 2 * IMG_BYTES, s, in, c.stride, c.n, c.nt, c.wd,
                     (const double*)L.F, (const double*)L.S[0], (const double*)L.S[1], (const long long*)L.firstbad, out);
  return hipGetLastError();
}

template <typename InT>
hipError_t launch_in(const Call& c, const Layout& L, hipStream_t s) {
  return c.out_kind == VP_SAMPLES_FLOAT32 ? launch_typed<InT, float>(c, L, s) : launch_typed<InT, double>(c, L, s);
}

hipError_t launch_sta_lta(const Call& c, const Layout& L, hipStream_t s) {
  if (c.in_kind == VP_SAMPLES_INT32) return launch_in<int>(c, L, s);
  if (c.in_kind == VP_SAMPLES_FLOAT32) return launch_in<float>(c, L, s);
  return launch_in<double>(c, L, s);
}

int make_call(const char* who, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n, int type,
              int64_t nsta, int64_t nlta, void* out_dev, int out_kind, Call* c) {
  if (const int rc = check_sta_lta(who, in_dev, in_kind, n_series, series_stride, n, type, nsta, nlta, out_dev, out_kind))
    return rc;
  c->in = in_dev, c->out = out_dev;
  c->in_kind = in_kind, c->out_kind = out_kind, c->n_series = n_series, c->type = type;
  c->stride = series_stride, c->n = n, c->nt = (n + DTILE - 1) / DTILE, c->nsta = nsta, c->nlta = nlta;
  stalta_rec_table(nsta, nlta, &c->rec);
  c->wd.w[0] = (int)nsta, c->wd.w[1] = (int)nlta;
  return VP_OK;
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_sta_lta(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                          int type, int64_t nsta, int64_t nlta, void* out_dev, int out_kind) {
  Call c;
  if (const int rc = make_call("vp_sta_lta", in_dev, in_kind, n_series, series_stride, n, type, nsta, nlta, out_dev, out_kind, &c))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_sta_lta: device index");
  if (n == 0) return VP_OK;
  VP_HIP(hipSetDevice(device_id));
  hipStream_t s = nullptr;  // the null stream, one synchronisation at the end: as vp_sos_filter
  DeviceScratch<2>& sc = stalta_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  const size_t bytes = Layout::bytes(c);
  if (const int rc = sc.b[0].grow("vp_sta_lta", bytes, bytes / 8 + 4096, &p)) return rc;
  VP_HIP(launch_sta_lta(c, Layout(p, c), s));
  VP_HIP(hipStreamSynchronize(s));
  return VP_OK;
}

extern "C" int vp_sta_lta_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_sta_lta_release_scratch", stalta_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_sta_lta_bench(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                                int type, int64_t nsta, int64_t nlta, void* out_dev, int out_kind, int iters,
                                float* ms_total) {
  VP_REQUIRE(ms_total && iters > 0 && n > 0, "vp_sta_lta_bench: bad argument");
  Call c;
  if (const int rc = make_call("vp_sta_lta_bench", in_dev, in_kind, n_series, series_stride, n, type, nsta, nlta, out_dev,
                               out_kind, &c))
    return rc;
  VP_REQUIRE(device_id >= 0, "vp_sta_lta_bench: device index");
  VP_HIP(hipSetDevice(device_id));
  DeviceScratch<2>& sc = stalta_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  void* p = nullptr;
  const size_t bytes = Layout::bytes(c);
  if (const int rc = sc.b[0].grow("vp_sta_lta_bench", bytes, bytes / 8 + 4096, &p)) return rc;
  const Layout L(p, c);
  BenchTimer t;
  VP_HIP(t.init());
  const auto all = [&] { return launch_sta_lta(c, L, t.s); };
  float t_all = 0.f;
  VP_HIP(t.run(3, all));
  VP_HIP(t.time(iters, all, &t_all));
  *ms_total = t_all;
  return VP_OK;
}

extern "C" int vp_trigger_onset(int device_id, const float* cft_dev, int n_series, int64_t series_stride, int64_t n,
                                float thr_on, float thr_off, int64_t* on, int64_t* off, int64_t* peak, float* value,
                                int32_t* series_of, int cap_per_series, int cap, int* n_found) {
  VP_REQUIRE(n_found, "vp_trigger_onset: null argument");
  VP_REQUIRE(n >= 0, "vp_trigger_onset: n = %lld is negative", (long long)n);
  VP_REQUIRE(n_series >= 1, "vp_trigger_onset: n_series = %d, need at least 1", n_series);
  VP_REQUIRE(series_stride >= n, "vp_trigger_onset: series_stride = %lld is below n = %lld", (long long)series_stride,
             (long long)n);
  VP_REQUIRE(n == 0 || cft_dev, "vp_trigger_onset: null argument");
  VP_REQUIRE(thr_off <= thr_on, "vp_trigger_onset: thr_off = %g above thr_on = %g is the host rule's case (vp_pick_host)",
             (double)thr_off, (double)thr_on);
  VP_REQUIRE(cap >= 0 && cap_per_series >= 0 && (cap == 0 || (on && off && peak && value)),
             "vp_trigger_onset: null output arrays");
  VP_REQUIRE(device_id >= 0, "vp_trigger_onset: device index");
  *n_found = 0;
  if (n == 0) return VP_OK;
  VP_HIP(hipSetDevice(device_id));
  hipStream_t s = nullptr;
  DeviceScratch<2>& sc = stalta_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  const ScanLayout L(n_series, cap_per_series);
  const size_t table = ((size_t)n_series * sizeof(PickArgs) + 255) / 256 * 256;
  void* p = nullptr;
  if (const int rc = sc.b[1].grow("vp_trigger_onset", table + L.total, 4096, &p)) return rc;
  PickArgs* d_rows = (PickArgs*)p;
  char* block = (char*)p + table;
  std::vector<PickArgs> rows(n_series);
  for (int r = 0; r < n_series; ++r)
    rows[r] = L.args(block, r, cft_dev + (size_t)r * series_stride, n, thr_on, thr_off, cap_per_series);
  VP_HIP(hipMemsetAsync(block, 0, L.header, s));  // counters
  VP_HIP(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(PickArgs), hipMemcpyHostToDevice, s));
  launch_pick_table(d_rows, n_series, (long)n, s);
  VP_HIP(hipGetLastError());
  std::vector<char> host(L.total);
  VP_HIP(hipMemcpyAsync(host.data(), block, L.total, hipMemcpyDeviceToHost, s));
  VP_HIP(hipStreamSynchronize(s));
  // per series sorted by onset; a series that overflowed cap_per_series raises *n_found above cap: call again with more room
  *n_found = collect_rows(L, host.data(), n_series, cap_per_series, on, off, peak, value, cap, cap + 1, [&](int i, int r) {
    if (series_of) series_of[i] = r;
  });
  return VP_OK;
}
