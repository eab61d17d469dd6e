// Stand-alone check of volpick_amd/csrc/api_host.h (WindowPlan, ScanLayout, collect_rows) against the code they
// replaced in api.hip, which is kept below word for word, and against the oracle's window rule.  Host compiler only, no
// HIP; tests/test_api_host_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_host.h"

// ------------------------------------------------------------------------------------------------------------------
// The replaced code (api.hip before WindowPlan / ScanLayout / collect_rows).
namespace old {

int64_t count_windows(int64_t N, int T, int overlap, int64_t* n_regular, int* has_tail) {
  if (N < T) {
    *n_regular = 0;
    *has_tail = 0;
    return 0;
  }
  const int64_t step = T - overlap;
  *n_regular = (N - T) / step + 1;
  *has_tail = ((*n_regular - 1) * step + T < N) ? 1 : 0;
  return *n_regular + *has_tail;
}

struct ScanLayout {
  size_t header, per_spec, total;
  int cap;
};
static ScanLayout scan_layout(int n_specs, int cap) {
  ScanLayout L;
  L.cap = std::max(cap, 1);
  L.header = ((size_t)n_specs * 2 * sizeof(int) + 255) / 256 * 256;
  L.per_spec = (size_t)L.cap * (3 * sizeof(int64_t) + sizeof(float));
  L.per_spec = (L.per_spec + 255) / 256 * 256;
  L.total = L.header + L.per_spec * n_specs;
  return L;
}

struct Slot {
  char* d_pick;
  char* h_pick;
  int n_specs, cap;
};

// the pointer fill of scan_submit, row i
static void fill_pick_args(vp::PickArgs& a, const Slot& sl, const ScanLayout& L, int i, const float* const* rows,
                           const int64_t* lens, const float* thr_on, const float* thr_off, int cap) {
  char* base = sl.d_pick + L.header + L.per_spec * i;
  a.trace = rows[i];
  a.n = lens[i] > 0 ? lens[i] : 0;
  a.thr_on = thr_on[i];
  a.thr_off = thr_off[i];
  a.count = (int*)sl.d_pick + 2 * i;
  a.on = (int64_t*)base;
  a.off = a.on + L.cap;
  a.peak = a.off + L.cap;
  a.value = (float*)(a.peak + L.cap);
  a.cap = cap;
}

static int scan_collect(const Slot& sl, int64_t* on, int64_t* off, int64_t* peak, float* value, int32_t* spec_of, int cap,
                        int* n_found) {
  const ScanLayout L = scan_layout(sl.n_specs, sl.cap);
  int total = 0, written = 0;
  for (int i = 0; i < sl.n_specs; ++i) {
    const int found = ((const int*)sl.h_pick)[2 * i];
    total += found;
    const int m = std::min(found, sl.cap);
    const char* base = sl.h_pick + L.header + L.per_spec * i;
    const int64_t* t_on = (const int64_t*)base;
    const int64_t* t_off = t_on + L.cap;
    const int64_t* t_pk = t_off + L.cap;
    const float* t_v = (const float*)(t_pk + L.cap);
    std::vector<int> order(m);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return t_on[x] < t_on[y]; });
    for (int k = 0; k < m && written < cap; ++k, ++written) {
      on[written] = t_on[order[k]];
      off[written] = t_off[order[k]];
      peak[written] = t_pk[order[k]];
      value[written] = t_v[order[k]];
      if (spec_of) spec_of[written] = i;
    }
  }
  *n_found = total;
  return 0;
}

// the tail of vp_classify_multi
struct Handle {
  char* m_pick_h;
};
static void multi_collect(const Handle* h, const ScanLayout& L, int R, int n_specs, int cap_per_row, int64_t* on, int64_t* off,
                          int64_t* peak, float* value, int32_t* spec_of, int32_t* block_of, int cap, int* n_found) {
  int total_found = 0, written = 0;
  for (int r = 0; r < R; ++r) {
    const int found = ((const int*)h->m_pick_h)[2 * r];
    total_found += found;
    const int m = std::min(found, cap_per_row);
    const char* base = h->m_pick_h + L.header + L.per_spec * r;
    const int64_t* t_on = (const int64_t*)base;
    const int64_t* t_off = t_on + L.cap;
    const int64_t* t_pk = t_off + L.cap;
    const float* t_v = (const float*)(t_pk + L.cap);
    std::vector<int> order(m);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return t_on[x] < t_on[y]; });
    for (int k = 0; k < m && written < cap; ++k, ++written) {
      on[written] = t_on[order[k]];
      off[written] = t_off[order[k]];
      peak[written] = t_pk[order[k]];
      value[written] = t_v[order[k]];
      if (spec_of) spec_of[written] = r % n_specs;
      if (block_of) block_of[written] = r / n_specs;
    }
    if (found > cap_per_row) total_found = std::max(total_found, cap + 1);  // forces the retry path
  }
  *n_found = total_found;
}

}  // namespace old

// ------------------------------------------------------------------------------------------------------------------
static long n_checked = 0, n_bad = 0;
#define CHECK(cond, ...)               \
  do {                                 \
    ++n_checked;                       \
    if (!(cond)) {                     \
      if (++n_bad <= 10) {             \
        printf("  mismatch: ");        \
        printf(__VA_ARGS__);           \
        printf("\n");                  \
      }                                \
    }                                  \
  } while (0)

static int report(const char* what, long bad_before, long checked_before) {
  const bool ok = n_bad == bad_before;
  printf("%s: %s (%ld comparisons)\n", what, ok ? "identical" : "DIFFERENT", n_checked - checked_before);
  return ok ? 0 : 1;
}

static uint32_t rng_state = 12345;
static uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

// ---- WindowPlan ----------------------------------------------------------------------------------------------------
// oracle.pipeline.window_starts: arange(0, N - T + 1, step), plus N - T if the last of them ends before N
struct OracleWindows {
  int64_t n_arange, N, T, step;
  OracleWindows(int64_t N_, int64_t T_, int64_t overlap) : N(N_), T(T_), step(T_ - overlap) {
    n_arange = N - T + 1 > 0 ? (N - T + 1 + step - 1) / step : 0;
  }
  bool tail() const { return n_arange > 0 && (n_arange - 1) * step + T < N; }
  int64_t count() const { return n_arange + (tail() ? 1 : 0); }
  int64_t start(int64_t i) const { return i < n_arange ? i * step : N - T; }
};

static void check_plan(int64_t N, int T, int overlap) {
  const int64_t step = T - overlap;
  int64_t n_reg;
  int tail;
  const int64_t nw = old::count_windows(N, T, overlap, &n_reg, &tail);
  const OracleWindows ow(N, T, overlap);
  const int blinds[3][2] = {{0, 0}, {1, 2}, {T - 2, 1}};
  for (const auto& b : blinds) {
    const vp::WindowPlan wp(N, T, overlap, b[0], b[1]);
    CHECK(wp.n_windows() == nw && wp.n_regular == n_reg && wp.has_tail == tail && wp.step == step && nw == ow.count(),
          "counts N=%lld T=%d overlap=%d: %lld/%lld/%d, old %lld/%lld/%d, oracle %lld", (long long)N, T, overlap,
          (long long)wp.n_windows(), (long long)wp.n_regular, wp.has_tail, (long long)nw, (long long)n_reg, tail,
          (long long)ow.count());
    // annotate_device / vp_classify_multi before the change
    const int64_t fv = nw > 0 ? b[0] : -1;
    const int64_t lv = nw > 0 ? (tail ? N - T : (n_reg - 1) * step) + T - b[1] - 1 : -1;
    const int64_t lv_oracle = nw > 0 ? ow.start(nw - 1) + T - b[1] - 1 : -1;
    CHECK(wp.first_valid == fv && wp.last_valid == lv && lv == lv_oracle, "valid range N=%lld T=%d overlap=%d blind (%d, %d): %lld..%lld, old %lld..%lld",
          (long long)N, T, overlap, b[0], b[1], (long long)wp.first_valid, (long long)wp.last_valid, (long long)fv, (long long)lv);
  }
  const vp::WindowPlan wp(N, T, overlap, 0, 0);
  const int64_t dense = 20000;  // every start up to here; of longer plans both ends and the regular / tail border
  for (int64_t i = 0; i < nw; ++i) {
    if (i == dense && nw > 2 * dense) i = nw - dense;
    const int64_t was = (i < n_reg) ? i * step : N - T;  // vp_window_starts / the window table before the change
    CHECK(wp.start(i) == was && was == ow.start(i), "start %lld of N=%lld T=%d overlap=%d: %lld, old %lld, oracle %lld", (long long)i,
          (long long)N, T, overlap, (long long)wp.start(i), (long long)was, (long long)ow.start(i));
  }
}

static int check_window_plans() {
  const long b0 = n_bad, c0 = n_checked;
  for (int T : {8, 3001}) {
    std::vector<int> overlaps = {0, 1, T / 2, T - 1, T / 3, T - 2, (int)(T * 0.9)};
    std::sort(overlaps.begin(), overlaps.end());
    overlaps.erase(std::unique(overlaps.begin(), overlaps.end()), overlaps.end());
    for (int overlap : overlaps) {
      const int64_t step = T - overlap;
      for (int64_t N = 1; N <= 3 * (int64_t)T; ++N) check_plan(N, T, overlap);
      for (int64_t k : {0ll, 1ll, 2ll, 3ll, 7ll, 1000ll, 1ll << 20, 1ll << 31})  // (the last: N and the starts beyond 2^31)
        for (int d = -1; d <= 1; ++d) check_plan(k * step + T + d, T, overlap);
    }
  }
  return report("window plans", b0, c0);
}

// ---- ScanLayout ----------------------------------------------------------------------------------------------------
static int check_layouts() {
  const long b0 = n_bad, c0 = n_checked;
  for (int n_specs : {1, 4, 5, 16, 48})
    for (int cap : {0, 1, 255, 256, 257}) {
      const old::ScanLayout O = old::scan_layout(n_specs, cap);
      const vp::ScanLayout L(n_specs, cap);
      CHECK(L.header == O.header && L.per_spec == O.per_spec && L.total == O.total && L.cap == O.cap, "sizes n_specs=%d cap=%d", n_specs, cap);
      std::vector<char> dev(L.total), host(L.total, 0);
      std::vector<const float*> rows(n_specs);
      std::vector<int64_t> lens(n_specs);
      std::vector<float> thr_on(n_specs), thr_off(n_specs);
      static const float traces[64] = {};
      for (int i = 0; i < n_specs; ++i) {
        rows[i] = traces + i;
        lens[i] = (i % 3 == 1) ? -(int64_t)i : ((int64_t)i << 29) + 7;  // negative lengths are clamped to 0
        thr_on[i] = .5f + i;
        thr_off[i] = .25f + i;
      }
      const old::Slot sl{dev.data(), host.data(), n_specs, cap};
      std::vector<std::pair<size_t, size_t>> spans;  // [begin, end) byte ranges of every array of every row
      for (int r = 0; r < n_specs; ++r) {
        vp::PickArgs was{};
        old::fill_pick_args(was, sl, O, r, rows.data(), lens.data(), thr_on.data(), thr_off.data(), cap);
        const vp::PickArgs a = L.args(dev.data(), r, rows[r], lens[r], thr_on[r], thr_off[r], cap);
        CHECK(a.trace == was.trace && a.n == was.n && a.thr_on == was.thr_on && a.thr_off == was.thr_off && a.on == was.on &&
                  a.off == was.off && a.peak == was.peak && a.value == was.value && a.cap == was.cap && a.count == was.count,
              "PickArgs of row %d, n_specs=%d cap=%d", r, n_specs, cap);
        CHECK(a.cap == cap && a.n >= 0, "caller's cap / clamped length of row %d", r);
        const vp::ScanRow v = L.row(host.data(), r);
        CHECK((const char*)v.on - host.data() == (const char*)a.on - dev.data() && (const char*)v.off - host.data() == (const char*)a.off - dev.data() &&
                  (const char*)v.peak - host.data() == (const char*)a.peak - dev.data() && (const char*)v.value - host.data() == (const char*)a.value - dev.data() &&
                  (const char*)&((const int*)host.data())[2 * r] - host.data() == (const char*)a.count - dev.data(),
              "host view of row %d, n_specs=%d cap=%d", r, n_specs, cap);
        const size_t n = (size_t)L.cap;
        spans.push_back({(size_t)((char*)a.count - dev.data()), (size_t)((char*)a.count - dev.data()) + 2 * sizeof(int)});
        spans.push_back({(size_t)((char*)a.on - dev.data()), (size_t)((char*)(a.on + n) - dev.data())});
        spans.push_back({(size_t)((char*)a.off - dev.data()), (size_t)((char*)(a.off + n) - dev.data())});
        spans.push_back({(size_t)((char*)a.peak - dev.data()), (size_t)((char*)(a.peak + n) - dev.data())});
        spans.push_back({(size_t)((char*)a.value - dev.data()), (size_t)((char*)(a.value + n) - dev.data())});
      }
      std::sort(spans.begin(), spans.end());
      for (size_t i = 0; i < spans.size(); ++i) {
        CHECK(spans[i].first < spans[i].second && spans[i].second <= L.total, "array outside the block, n_specs=%d cap=%d", n_specs, cap);
        CHECK(i == 0 || spans[i - 1].second <= spans[i].first, "arrays overlap, n_specs=%d cap=%d", n_specs, cap);
        CHECK((spans[i].first < L.header) == (spans[i].second <= L.header), "array straddles the header, n_specs=%d cap=%d", n_specs, cap);
      }
    }
  return report("scan layouts", b0, c0);
}

// ---- collect_rows --------------------------------------------------------------------------------------------------
struct Out {
  std::vector<int64_t> on, off, peak;
  std::vector<float> value;
  std::vector<int32_t> spec_of, block_of;
  int n_found = -1;
  explicit Out(int n) : on(n + 4, -7), off(n + 4, -7), peak(n + 4, -7), value(n + 4, -7.f), spec_of(n + 4, -7), block_of(n + 4, -7) {}
  bool operator==(const Out& o) const {
    return on == o.on && off == o.off && peak == o.peak && value == o.value && spec_of == o.spec_of && block_of == o.block_of &&
           n_found == o.n_found;
  }
};

// a host block as the publish kernel leaves it: per row `found` and min(found, cap) entries in the order the scan
// appended them (any order), the rest of every array untouched (here: a pattern no result may contain)
static std::vector<char> make_block(const vp::ScanLayout& L, int n_rows, int row_cap, int variant, int* sum_kept) {
  std::vector<char> block(L.total, (char)0xA5);
  const int counts[5] = {0, 1, row_cap, row_cap + 1, 3 * row_cap};
  *sum_kept = 0;
  for (int r = 0; r < n_rows; ++r) {
    const int found = counts[(2 * r + variant) % 5];
    ((int*)block.data())[2 * r] = found;
    ((int*)block.data())[2 * r + 1] = 0;
    const vp::PickArgs a = L.args(block.data(), r, nullptr, 0, 0.f, 0.f, row_cap);
    const int m = std::min(found, row_cap);
    *sum_kept += m;
    std::vector<int64_t> onsets(m);
    for (int k = 0; k < m; ++k) onsets[k] = ((int64_t)1 << 32) * (r % 2) + 10 * k + r;  // distinct inside a row
    for (int k = m - 1; k > 0; --k) std::swap(onsets[k], onsets[rng() % (k + 1)]);
    for (int k = 0; k < m; ++k) {
      a.on[k] = onsets[k];
      a.off[k] = onsets[k] + 3;
      a.peak[k] = onsets[k] + 1;
      a.value[k] = .5f + (float)(onsets[k] % 1000) / 2048.f;
    }
  }
  return block;
}

static int check_collect() {
  const long b0 = n_bad, c0 = n_checked;
  for (int n_specs : {1, 3, 16})
    for (int K : {1, 5})
      for (int row_cap : {0, 1, 2, 7}) {
        const int R = n_specs * K;
        const vp::ScanLayout L(R, row_cap);
        const old::ScanLayout O = old::scan_layout(R, row_cap);
        for (int variant = 0; variant < 5; ++variant) {  // every row takes every count once
          int kept;
          std::vector<char> block = make_block(L, R, row_cap, variant, &kept);
          for (int cap : {0, 1, kept / 2, kept - 1, kept, kept + 1, kept + 9}) {
            if (cap < 0) continue;
            for (int with_ids = 0; with_ids < 2; ++with_ids) {
              // scan_collect: the rows are the specs of one slot
              Out was(cap), now(cap);
              const old::Slot sl{nullptr, block.data(), R, row_cap};
              old::scan_collect(sl, was.on.data(), was.off.data(), was.peak.data(), was.value.data(), with_ids ? was.spec_of.data() : nullptr, cap,
                                &was.n_found);
              int32_t* ids = with_ids ? now.spec_of.data() : nullptr;
              now.n_found = vp::collect_rows(L, block.data(), R, row_cap, now.on.data(), now.off.data(), now.peak.data(), now.value.data(), cap, 0,
                                             [&](int i, int r) {
                                               if (ids) ids[i] = r;
                                             });
              CHECK(was == now, "scan_collect n_specs=%d row_cap=%d cap=%d: n_found %d, old %d", R, row_cap, cap, now.n_found, was.n_found);
              if (row_cap == 0) continue;  // vp_classify_multi requires cap_per_row > 0
              // the tail of vp_classify_multi: row r is spec r % n_specs of block r / n_specs
              Out mwas(cap), mnow(cap);
              const old::Handle h{block.data()};
              old::multi_collect(&h, O, R, n_specs, row_cap, mwas.on.data(), mwas.off.data(), mwas.peak.data(), mwas.value.data(),
                                 with_ids ? mwas.spec_of.data() : nullptr, with_ids ? mwas.block_of.data() : nullptr, cap, &mwas.n_found);
              int32_t *spec_of = with_ids ? mnow.spec_of.data() : nullptr, *block_of = with_ids ? mnow.block_of.data() : nullptr;
              mnow.n_found = vp::collect_rows(L, block.data(), R, row_cap, mnow.on.data(), mnow.off.data(), mnow.peak.data(), mnow.value.data(), cap,
                                              cap + 1, [&](int i, int r) {
                                                if (spec_of) spec_of[i] = r % n_specs;
                                                if (block_of) block_of[i] = r / n_specs;
                                              });
              CHECK(mwas == mnow, "multi collect n_specs=%d K=%d row_cap=%d cap=%d: n_found %d, old %d", n_specs, K, row_cap, cap, mnow.n_found,
                    mwas.n_found);
              bool overflowed = false;
              for (int r = 0; r < R; ++r) overflowed |= L.row(block.data(), r).found > row_cap;
              CHECK(!overflowed || mnow.n_found >= cap + 1, "an overflowed row must force n_found > cap (n_found %d, cap %d)", mnow.n_found, cap);
              for (int i = 1; with_ids && i < std::min(cap, kept); ++i)  // sorted by onset inside a row
                CHECK(mnow.spec_of[i] != mnow.spec_of[i - 1] || mnow.block_of[i] != mnow.block_of[i - 1] || mnow.on[i] > mnow.on[i - 1],
                      "onsets out of order at %d", i);
            }
          }
        }
      }
  return report("collected results", b0, c0);
}

int main() {
  int rc = check_window_plans();
  rc |= check_layouts();
  rc |= check_collect();
  return rc;
}
