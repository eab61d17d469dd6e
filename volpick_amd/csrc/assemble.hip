// Waveform-bank assembly from device-resident source traces (include/volpick_hip.h, vp_bank_assemble): detrend("demean")
// per source trace, the zero-filled (3, L) array of stream_to_array with its "last writer wins" overlap rule, the row-wise
// demean and the single rounding to fp32, for every (trace, component) row of any number of traces in three launches.
// The host plans which samples go where (volpick_amd/convert.py); this file executes the piece table.
//
// Bound by memory traffic: a source sample is read twice (stats, write), a bank sample written once, all as dwords (or
// qwords) that consecutive lanes take from consecutive addresses, a thread's AS_PER loads in flight together.  Who wins a destination sample follows from the table
// alone, so the row mean needs no pass over the assembled row:
//   mean_row = sum over the row's pieces of (sum of the x the piece wins - their count * mean_piece) / L.
#include "batchgen.h"

#include <algorithm>

namespace vp {

namespace {

constexpr int AS_NTH = 256, AS_PER = 16, AS_NWV = AS_NTH / 64;
constexpr int AS_TILE = AS_NTH * AS_PER;  // samples per workgroup, of a piece's mean range (stats) and of a row (write)
static_assert(AS_TILE == VP_ASSEMBLE_TILE, "the header documents the tile");
constexpr long long AS_MAX_N = 1LL << 40;  // per piece and row: index arithmetic and tile counts stay far from overflow

struct AsPiece {
  const void* src;
  long long mean_n, keep_lo, keep_n, dst;
  long long tile_first;  // its stats tiles: [tile_first, tile_first + ceil(mean_n / AS_TILE))
  int row, kind;
};
struct AsRow {
  long long out, L;       // the row is data[out .. out + L)
  long long tile_first;   // its write tiles
  int piece_first, piece_end;
};
struct AsArgs {
  const AsPiece* pieces;
  const AsRow* rows;
  const int* stat_tile_piece;  // [stats tiles]
  const int* write_tile_row;   // [write tiles]
  double* part;                // [stats tiles][3]: sum of x over the mean range, sum of won x, won count
  double* piece_mean;          // [pieces]
  double* row_mean;            // [rows]
  float* data;
};

// Whether a piece behind p in its row's table order covers row sample j (then p does not win it).
__device__ __forceinline__ bool as_overwritten(const AsPiece* pieces, int p, int end, long long j) {
  for (int q = p + 1; q < end; ++q) {
    const long long d = j - pieces[q].dst;
    if (d >= 0 && d < pieces[q].keep_n) return true;
  }
  return false;
}

__device__ __forceinline__ double as_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A tile's AS_PER samples per thread of a typed source of n samples, from i0 on, all loads in flight at once: an index past
// the end reads the last sample instead (the caller ignores it).
template <typename T>
__device__ __forceinline__ void as_load(const T* __restrict__ src, long long n, long long i0, int t, double x[AS_PER]) {
  T raw[AS_PER];
#pragma unroll
  for (int k = 0; k < AS_PER; ++k) {
    const long long i = i0 + k * AS_NTH + t;
    raw[k] = src[i < 0 ? 0 : (i < n ? i : n - 1)];
  }
#pragma unroll
  for (int k = 0; k < AS_PER; ++k) x[k] = (double)raw[k];
}
__device__ __forceinline__ void as_load(const void* src, int kind, long long n, long long i0, int t, double x[AS_PER]) {
  if (kind == VP_SAMPLES_INT32)  // (uniform over the workgroup: one piece)
    as_load(static_cast<const int*>(src), n, i0, t, x);
  else if (kind == VP_SAMPLES_FLOAT32)
    as_load(static_cast<const float*>(src), n, i0, t, x);
  else
    as_load(static_cast<const double*>(src), n, i0, t, x);
}

// One tile of one piece's mean range -> part[tile][0..2].  Per thread AS_PER samples in ascending order, the wave's
// butterfly, the waves in ascending order: the same order for every launch.
__global__ __launch_bounds__(AS_NTH) void assemble_stats_kernel(const AsArgs a) {
  __shared__ double red[3][AS_NWV];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = a.stat_tile_piece[blockIdx.x];
  const AsPiece pc = a.pieces[p];
  const int end = a.rows[pc.row].piece_end;
  const long long i0 = ((long long)blockIdx.x - pc.tile_first) * AS_TILE;
  double x[AS_PER];
  as_load(pc.src, pc.kind, pc.mean_n, i0, t, x);
  double s = 0.0, w = 0.0, c = 0.0;
#pragma unroll
  for (int k = 0; k < AS_PER; ++k) {
    const long long i = i0 + k * AS_NTH + t, d = i - pc.keep_lo;
    if (i < pc.mean_n) {
      s += x[k];
      if (d >= 0 && d < pc.keep_n && !(end > p + 1 && as_overwritten(a.pieces, p, end, pc.dst + d))) {
        w += x[k];
        c += 1.0;
      }
    }
  }
  s = as_wave_sum(s);
  w = as_wave_sum(w);
  c = as_wave_sum(c);
  if (lane == 0) red[0][wave] = s, red[1][wave] = w, red[2][wave] = c;
  __syncthreads();
  if (t < 3) {
    double acc = 0.0;
    for (int i = 0; i < AS_NWV; ++i) acc += red[t][i];
    a.part[3 * (size_t)blockIdx.x + t] = acc;
  }
}

// One wavefront per row: its pieces' means, then the row's.
__global__ __launch_bounds__(64) void assemble_means_kernel(const AsArgs a) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const AsRow row = a.rows[r];
  double acc = 0.0;
  for (int p = row.piece_first; p < row.piece_end; ++p) {
    const long long n = a.pieces[p].mean_n, t0 = a.pieces[p].tile_first, nt = (n + AS_TILE - 1) / AS_TILE;
    double s = 0.0, w = 0.0, c = 0.0;
    for (long long k = lane; k < nt; k += 64) {
      const double* q = a.part + 3 * (size_t)(t0 + k);
      s += q[0];
      w += q[1];
      c += q[2];
    }
    s = as_wave_sum(s);
    w = as_wave_sum(w);
    c = as_wave_sum(c);
    const double m = s / (double)n;
    if (lane == 0) a.piece_mean[p] = m;
    acc += w - c * m;
  }
  if (lane == 0) a.row_mean[r] = acc / (double)row.L;
}

// One tile of one row: the row's pieces that touch the tile in table order, each overwriting what an earlier one put there
// (in registers: the last one wins), 0 where there is none; minus the row mean; one rounding, one store per sample.
__global__ __launch_bounds__(AS_NTH) void assemble_write_kernel(const AsArgs a) {
  const int t = threadIdx.x;
  const int r = a.write_tile_row[blockIdx.x];
  const AsRow row = a.rows[r];
  const long long j0 = ((long long)blockIdx.x - row.tile_first) * AS_TILE;
  const double mr = a.row_mean[r];
  double v[AS_PER];
#pragma unroll
  for (int k = 0; k < AS_PER; ++k) v[k] = 0.0;
  for (int p = row.piece_first; p < row.piece_end; ++p) {
    const AsPiece pc = a.pieces[p];
    if (pc.dst >= j0 + AS_TILE || pc.dst + pc.keep_n <= j0) continue;  // (uniform) not in this tile
    const double m = a.piece_mean[p];
    double x[AS_PER];
    as_load(static_cast<const char*>(pc.src) + pc.keep_lo * (pc.kind == VP_SAMPLES_FLOAT64 ? 8 : 4), pc.kind, pc.keep_n,
            j0 - pc.dst, t, x);
#pragma unroll
    for (int k = 0; k < AS_PER; ++k) {
      const long long d = j0 + k * AS_NTH + t - pc.dst;
      if (d >= 0 && d < pc.keep_n) v[k] = x[k] - m;
    }
  }
  float* out = a.data + row.out;
#pragma unroll
  for (int k = 0; k < AS_PER; ++k) {
    const long long j = j0 + k * AS_NTH + t;
    if (j < row.L) out[j] = (float)(v[k] - mr);
  }
}

size_t as_align(size_t n) { return (n + 15) & ~(size_t)15; }

int as_launch_error(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return VP_OK;
  set_error("%s launch failed: %s", name, hipGetErrorString(e));
  return VP_ERR_HIP;
}

}  // namespace

}  // namespace vp

using namespace vp;

extern "C" int vp_bank_assemble(vp_bank* h, long long first_trace, long long n_traces, const vp_assemble_piece* pieces,
                                long long n_pieces, const int64_t* trace_lengths, const double* onsets, void* stream) {
  VP_REQUIRE(h && trace_lengths && onsets && n_traces >= 1, "vp_bank_assemble: bad argument");
  VP_REQUIRE(n_pieces >= 0 && n_pieces <= INT32_MAX && (pieces || n_pieces == 0), "vp_bank_assemble: %lld pieces at %p",
             n_pieces, (const void*)pieces);
  Bank& bk = *reinterpret_cast<Bank*>(h);
  VP_REQUIRE(first_trace == bk.n_written, "vp_bank_assemble: traces are written in order: next is %lld, got %lld",
             bk.n_written, first_trace);
  VP_REQUIRE(n_traces <= bk.n_traces - bk.n_written, "vp_bank_assemble: %lld traces past the bank's %lld", n_traces,
             bk.n_traces);
  const size_t nt = (size_t)n_traces, np = (size_t)n_pieces, nr = 3 * nt;
  std::vector<long long> off(nt), len(nt);
  long long floats = 0;
  for (size_t i = 0; i < nt; ++i) {
    VP_REQUIRE(trace_lengths[i] >= 1 && trace_lengths[i] <= AS_MAX_N, "vp_bank_assemble: trace %lld has length %lld",
               first_trace + (long long)i, (long long)trace_lengths[i]);
    off[i] = bk.floats_written + floats;
    len[i] = trace_lengths[i];
    floats += 3 * trace_lengths[i];
    VP_REQUIRE(floats <= bk.n_floats - bk.floats_written, "vp_bank_assemble: %lld floats past the bank's %lld", floats,
               bk.n_floats);
  }

  // rows and their write tiles
  std::vector<AsRow> rows(nr);
  long long write_tiles = 0;
  for (size_t r = 0; r < nr; ++r) {
    const long long L = len[r / 3];
    rows[r] = AsRow{off[r / 3] + (long long)(r % 3) * L, L, write_tiles, 0, 0};
    write_tiles += (L + AS_TILE - 1) / AS_TILE;
  }
  // pieces, checked, and their stats tiles
  std::vector<AsPiece> pcs(np);
  long long stat_tiles = 0, prev_row = -1;
  for (size_t p = 0; p < np; ++p) {
    const vp_assemble_piece& q = pieces[p];
    VP_REQUIRE(q.trace >= first_trace && q.trace < first_trace + n_traces, "vp_bank_assemble: piece %zu: trace %d outside [%lld, %lld)",
               p, (int)q.trace, first_trace, first_trace + n_traces);
    VP_REQUIRE(q.component >= 0 && q.component < 3, "vp_bank_assemble: piece %zu: component %d outside [0, 3)", p,
               (int)q.component);
    VP_REQUIRE(q.kind == VP_SAMPLES_INT32 || q.kind == VP_SAMPLES_FLOAT32 || q.kind == VP_SAMPLES_FLOAT64,
               "vp_bank_assemble: piece %zu: sample kind %d is none of VP_SAMPLES_INT32 / FLOAT32 / FLOAT64", p, (int)q.kind);
    VP_REQUIRE(q.src, "vp_bank_assemble: piece %zu: null source", p);
    VP_REQUIRE(q.mean_n >= 1 && q.mean_n <= AS_MAX_N && q.keep_n >= 1, "vp_bank_assemble: piece %zu: mean range of %lld, kept range of %lld samples",
               p, (long long)q.mean_n, (long long)q.keep_n);
    VP_REQUIRE(q.keep_lo >= 0 && q.keep_n <= q.mean_n - q.keep_lo, "vp_bank_assemble: piece %zu: kept [%lld, +%lld) outside its mean range [0, %lld)",
               p, (long long)q.keep_lo, (long long)q.keep_n, (long long)q.mean_n);
    const long long row = 3 * (q.trace - first_trace) + q.component, L = len[(size_t)(q.trace - first_trace)];
    VP_REQUIRE(q.dst >= 0 && q.keep_n <= L - q.dst, "vp_bank_assemble: piece %zu: row samples [%lld, +%lld) outside [0, %lld)", p,
               (long long)q.dst, (long long)q.keep_n, L);
    VP_REQUIRE(row >= prev_row, "vp_bank_assemble: piece %zu: rows (trace, component) must ascend", p);
    prev_row = row;
    pcs[p] = AsPiece{q.src, q.mean_n, q.keep_lo, q.keep_n, q.dst, stat_tiles, (int)row, (int)q.kind};
    stat_tiles += (q.mean_n + AS_TILE - 1) / AS_TILE;
  }
  for (size_t r = 0, p = 0; r < nr; ++r) {  // rows ascend: a row's pieces are one run of the table
    rows[r].piece_first = (int)p;
    while (p < np && pcs[p].row == (int)r) ++p;
    rows[r].piece_end = (int)p;
  }
  VP_REQUIRE(stat_tiles <= INT32_MAX && write_tiles <= INT32_MAX, "vp_bank_assemble: %lld + %lld tiles in one call", stat_tiles,
             write_tiles);
  std::vector<int> stat_tile_piece((size_t)stat_tiles), write_tile_row((size_t)write_tiles);
  for (size_t p = 0; p < np; ++p)
    std::fill_n(stat_tile_piece.begin() + pcs[p].tile_first, (pcs[p].mean_n + AS_TILE - 1) / AS_TILE, (int)p);
  for (size_t r = 0; r < nr; ++r)
    std::fill_n(write_tile_row.begin() + rows[r].tile_first, (rows[r].L + AS_TILE - 1) / AS_TILE, (int)r);

  // one staged block: the tables, the bank's per-trace arrays, then (device only) the sums
  const size_t b_pcs = np * sizeof(AsPiece), b_rows = nr * sizeof(AsRow), b_st = (size_t)stat_tiles * sizeof(int),
               b_wt = (size_t)write_tiles * sizeof(int), b_ll = nt * sizeof(long long), b_on = nt * 4 * sizeof(double);
  const size_t o_rows = as_align(b_pcs), o_st = o_rows + as_align(b_rows), o_wt = o_st + as_align(b_st),
               o_off = o_wt + as_align(b_wt), o_len = o_off + as_align(b_ll), o_on = o_len + as_align(b_ll),
               staged = o_on + as_align(b_on);
  const size_t o_part = staged, o_pm = o_part + as_align((size_t)stat_tiles * 3 * sizeof(double)),
               o_rm = o_pm + as_align(np * sizeof(double)), total = o_rm + as_align(nr * sizeof(double));
  std::vector<char> blob(staged, 0);
  if (b_pcs) memcpy(blob.data(), pcs.data(), b_pcs);
  memcpy(blob.data() + o_rows, rows.data(), b_rows);
  if (b_st) memcpy(blob.data() + o_st, stat_tile_piece.data(), b_st);
  memcpy(blob.data() + o_wt, write_tile_row.data(), b_wt);
  memcpy(blob.data() + o_off, off.data(), b_ll);
  memcpy(blob.data() + o_len, len.data(), b_ll);
  memcpy(blob.data() + o_on, onsets, b_on);

  VP_HIP(hipSetDevice(bk.device));
  int rc = bk.assemble_ring.acquire(total);
  if (rc != VP_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* dev = static_cast<char*>(bk.assemble_ring.stage({{blob.data(), staged}}, s));
  if (!dev) return VP_ERR_HIP;
  VP_HIP(hipMemcpyAsync(bk.off_dev + first_trace, dev + o_off, b_ll, hipMemcpyDeviceToDevice, s));
  VP_HIP(hipMemcpyAsync(bk.len_dev + first_trace, dev + o_len, b_ll, hipMemcpyDeviceToDevice, s));
  VP_HIP(hipMemcpyAsync(bk.onset_dev + 4 * first_trace, dev + o_on, b_on, hipMemcpyDeviceToDevice, s));
  AsArgs a{};
  a.pieces = reinterpret_cast<const AsPiece*>(dev);
  a.rows = reinterpret_cast<const AsRow*>(dev + o_rows);
  a.stat_tile_piece = reinterpret_cast<const int*>(dev + o_st);
  a.write_tile_row = reinterpret_cast<const int*>(dev + o_wt);
  a.part = reinterpret_cast<double*>(dev + o_part);
  a.piece_mean = reinterpret_cast<double*>(dev + o_pm);
  a.row_mean = reinterpret_cast<double*>(dev + o_rm);
  a.data = bk.data;
  if (stat_tiles) {
    hipLaunchKernelGGL(assemble_stats_kernel, dim3((unsigned)stat_tiles), dim3(AS_NTH), 0, s, a);
    if ((rc = as_launch_error("assemble_stats_kernel")) != VP_OK) return rc;
  }
  hipLaunchKernelGGL(assemble_means_kernel, dim3((unsigned)nr), dim3(64), 0, s, a);
  if ((rc = as_launch_error("assemble_means_kernel")) != VP_OK) return rc;
  hipLaunchKernelGGL(assemble_write_kernel, dim3((unsigned)write_tiles), dim3(AS_NTH), 0, s, a);
  if ((rc = as_launch_error("assemble_write_kernel")) != VP_OK) return rc;
  if ((rc = bk.assemble_ring.retire(s)) != VP_OK) return rc;
  bk.len.insert(bk.len.end(), len.begin(), len.end());
  bk.off.insert(bk.off.end(), off.begin(), off.end());
  bk.n_written += n_traces;
  bk.floats_written += floats;
  return VP_OK;
}
