// Stand-alone check of volpick_amd/csrc/sos_host.h (check_sample_kind, load_sos, warmup_length) against the code it
// replaced: the validation bodies of make_plan in resample.hip and in sosfilt.hip and resample.hip's warmup_length, kept
// below word for word (what followed the checks -- the choice of kernels, the matrix table -- is cut).  Host compiler
// only, no HIP; tests/test_sos_host_cpu.py writes the coefficient tables, builds this with
// -fsanitize=address,undefined and runs it:   sos_host_check TABLES
// TABLES: per table a line "NAME N_SECTIONS DECIMATE_CODE" and 6 N_SECTIONS numbers (C99 hex floats) in scipy's row order;
// DECIMATE_CODE is what decimation answers to the table as it is (0, or -4 where its warm-up is beyond the halo), worked
// out by the wrapper from numpy's roots.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sos_host.h"

static char g_error[512];
void vp::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

constexpr int DHALO = 1024;  // resample.hip: room for the warm-up ahead of a tile

// ------------------------------------------------------------------------------------------------------------------
// The replaced code.
namespace old {
using namespace vp;

int warmup_length(const double* sos, int ns, double* r_out) {
  const double r = sos_pole_radius(sos, ns);
  *r_out = r;
  if (!(r < 1.0)) return -1;
  if (r < 1e-12) return 2 * ns;
  return (int)std::ceil(40.0 * std::log(2.0) / -std::log(r)) + 2 * ns;
}

struct DecimatePlan {
  SosArg arg;
  int warm;
};

int make_decimate_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                       int factor, const float* out_dev, int64_t out_len, DecimatePlan* plan) {
  VP_REQUIRE(in_dev && sos && out_dev, "%s: null argument", who);
  VP_REQUIRE(in_kind == VP_SAMPLES_INT32 || in_kind == VP_SAMPLES_FLOAT32 || in_kind == VP_SAMPLES_FLOAT64,
             "%s: in_kind %d is none of VP_SAMPLES_INT32 / FLOAT32 / FLOAT64", who, in_kind);
  VP_REQUIRE(n >= 1, "%s: n = %lld, need at least one sample", who, (long long)n);
  VP_REQUIRE(factor >= 2, "%s: factor = %d, need >= 2", who, factor);
  VP_REQUIRE(n_sections >= 1 && n_sections <= DMAXS, "%s: n_sections = %d, the kernel is built for 1..%d", who, n_sections,
             DMAXS);
  VP_REQUIRE(out_len == (n + factor - 1) / factor, "%s: out_len = %lld, ceil(n / factor) = %lld", who, (long long)out_len,
             (long long)((n + factor - 1) / factor));
  for (int s = 0; s < n_sections; ++s) {
    for (int i = 0; i < 6; ++i) VP_REQUIRE(std::isfinite(sos[6 * s + i]), "%s: section %d has a non-finite coefficient", who, s);
    VP_REQUIRE(sos[6 * s + 3] == 1.0, "%s: section %d has a0 = %g, need 1 (scipy's sos layout)", who, s, sos[6 * s + 3]);
    plan->arg.c[s][0] = sos[6 * s + 0];
    plan->arg.c[s][1] = sos[6 * s + 1];
    plan->arg.c[s][2] = sos[6 * s + 2];
    plan->arg.c[s][3] = sos[6 * s + 4];
    plan->arg.c[s][4] = sos[6 * s + 5];
  }
  for (int s = n_sections; s < DMAXS; ++s)
    for (int i = 0; i < 5; ++i) plan->arg.c[s][i] = 0.0;
  double r = 0.0;
  plan->warm = warmup_length(sos, n_sections, &r);
  VP_REQUIRE(plan->warm >= 0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  if (plan->warm > DHALO) {
    set_error("%s: largest pole radius %g needs a warm-up of %d samples, the tile has room for %d", who, r, plan->warm, DHALO);
    return VP_ERR_UNSUPPORTED;
  }
  return VP_OK;
}

size_t elem_bytes(int kind) { return kind == VP_SAMPLES_FLOAT64 ? 8 : 4; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

struct FilterPlan {
  SosArg arg;
  int ns;
};

int make_filter_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                     const float* out_dev, FilterPlan* plan, double* r_seen) {
  VP_REQUIRE(in_kind == VP_SAMPLES_INT32 || in_kind == VP_SAMPLES_FLOAT32 || in_kind == VP_SAMPLES_FLOAT64,
             "%s: in_kind %d is none of VP_SAMPLES_INT32 / FLOAT32 / FLOAT64", who, in_kind);
  VP_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
  VP_REQUIRE(sos, "%s: null argument", who);
  VP_REQUIRE(n == 0 || (in_dev && out_dev), "%s: null argument", who);
  VP_REQUIRE(n_sections >= 1 && n_sections <= DMAXS, "%s: n_sections = %d, the kernel is built for 1..%d", who, n_sections,
             DMAXS);
  for (int s = 0; s < n_sections; ++s) {
    for (int i = 0; i < 6; ++i) VP_REQUIRE(std::isfinite(sos[6 * s + i]), "%s: section %d has a non-finite coefficient", who, s);
    VP_REQUIRE(sos[6 * s + 3] == 1.0, "%s: section %d has a0 = %g, need 1 (scipy's sos layout)", who, s, sos[6 * s + 3]);
    plan->arg.c[s][0] = sos[6 * s + 0];
    plan->arg.c[s][1] = sos[6 * s + 1];
    plan->arg.c[s][2] = sos[6 * s + 2];
    plan->arg.c[s][3] = sos[6 * s + 4];
    plan->arg.c[s][4] = sos[6 * s + 5];
  }
  for (int s = n_sections; s < DMAXS; ++s)
    for (int i = 0; i < 5; ++i) plan->arg.c[s][i] = 0.0;
  const double r = sos_pole_radius(sos, n_sections);
  *r_seen = r;  // (the one line added: the radius the old body computed, for the comparison)
  VP_REQUIRE(r < 1.0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  VP_REQUIRE(n == 0 || !overlap(in_dev, (size_t)n * elem_bytes(in_kind), out_dev, (size_t)n * sizeof(float)),
             "%s: out_dev overlaps in_dev", who);
  plan->ns = n_sections;
  return VP_OK;
}

}  // namespace old

// ------------------------------------------------------------------------------------------------------------------
// The same two plans as resample.hip and sosfilt.hip make them now: sos_host.h for what they share, and each
// operation's own lines (n, factor and out_len, the warm-up refusal; n, the overlap) around it.  These two functions are
// a copy by hand of make_plan in the two .hip files (which need HIP to compile), not that code itself: what this program
// exercises for real is check_sample_kind, load_sos and warmup_length, and whoever changes a make_plan keeps the copy in step.
namespace now {
using namespace vp;

int make_decimate_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                       int factor, const float* out_dev, int64_t out_len, old::DecimatePlan* plan, double* r_seen) {
  VP_REQUIRE(in_dev && sos && out_dev, "%s: null argument", who);
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n >= 1, "%s: n = %lld, need at least one sample", who, (long long)n);
  VP_REQUIRE(factor >= 2, "%s: factor = %d, need >= 2", who, factor);
  VP_REQUIRE(out_len == (n + factor - 1) / factor, "%s: out_len = %lld, ceil(n / factor) = %lld", who, (long long)out_len,
             (long long)((n + factor - 1) / factor));
  double r = 0.0;
  if (const int rc = load_sos(who, sos, n_sections, &plan->arg, &r)) return rc;
  *r_seen = r;
  plan->warm = warmup_length(sos, n_sections, &r);
  VP_REQUIRE(plan->warm >= 0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  if (plan->warm > DHALO) {
    set_error("%s: largest pole radius %g needs a warm-up of %d samples, the tile has room for %d", who, r, plan->warm, DHALO);
    return VP_ERR_UNSUPPORTED;
  }
  return VP_OK;
}

int make_filter_plan(const char* who, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                     const float* out_dev, old::FilterPlan* plan, double* r_seen) {
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
  VP_REQUIRE(sos, "%s: null argument", who);
  VP_REQUIRE(n == 0 || (in_dev && out_dev), "%s: null argument", who);
  double r = 0.0;
  if (const int rc = load_sos(who, sos, n_sections, &plan->arg, &r)) return rc;
  *r_seen = r;
  VP_REQUIRE(r < 1.0, "%s: the filter is not stable (largest pole radius %g)", who, r);
  VP_REQUIRE(n == 0 || !old::overlap(in_dev, (size_t)n * elem_bytes(in_kind), out_dev, (size_t)n * sizeof(float)),
             "%s: out_dev overlaps in_dev", who);
  plan->ns = n_sections;
  return VP_OK;
}

}  // namespace now

// ------------------------------------------------------------------------------------------------------------------
static int g_cases = 0, g_bad = 0;

static bool same_double(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void fail(const std::string& label, const char* what) {
  ++g_bad;
  std::printf("DIFFERENT %s: %s\n", label.c_str(), what);
}

// One call of both plans, old and new, on one table and one sample kind.  `want`: the code reasoning expects, whatever
// the two sides say.
static void compare(const std::string& label, const double* sos, int ns, int in_kind, int want_decimate, int want_filter) {
  static int in_buf[64];
  static float out_buf[64];
  const int64_t n = 16;
  const int factor = 2;
  ++g_cases;
  for (const char* who : {"vp_decimate_lowpass", "vp_decimate_lowpass_bench"}) {
    old::DecimatePlan po, pn;
    std::memset(&po, 0xAA, sizeof po);
    std::memset(&pn, 0xAA, sizeof pn);
    double r_new = -7.0;
    g_error[0] = 0;
    const int rc_old = old::make_decimate_plan(who, in_buf, in_kind, n, sos, ns, factor, out_buf, n / factor, &po);
    const std::string text_old = g_error;
    g_error[0] = 0;
    const int rc_new = now::make_decimate_plan(who, in_buf, in_kind, n, sos, ns, factor, out_buf, n / factor, &pn, &r_new);
    if (rc_old != rc_new) fail(label, "decimation: return code");
    if (rc_old != want_decimate) fail(label, "decimation: not the expected code");
    if (text_old != g_error) fail(label, "decimation: error text");
    if (std::memcmp(&po.arg, &pn.arg, sizeof po.arg) != 0) fail(label, "decimation: SosArg bytes");
    if (std::memcmp(&po.warm, &pn.warm, sizeof po.warm) != 0) fail(label, "decimation: warm-up");
    if (rc_old == VP_OK && !(r_new < 1.0)) fail(label, "decimation: accepted with a radius of 1 or more");
    if (rc_old == VP_OK && text_old != "") fail(label, "decimation: text without an error");
  }
  for (const char* who : {"vp_sos_filter", "vp_sos_filter_bench"}) {
    old::FilterPlan po, pn;
    std::memset(&po, 0xAA, sizeof po);
    std::memset(&pn, 0xAA, sizeof pn);
    double r_old = -7.0, r_new = -7.0;
    g_error[0] = 0;
    const int rc_old = old::make_filter_plan(who, in_buf, in_kind, n, sos, ns, out_buf, &po, &r_old);
    const std::string text_old = g_error;
    g_error[0] = 0;
    const int rc_new = now::make_filter_plan(who, in_buf, in_kind, n, sos, ns, out_buf, &pn, &r_new);
    if (rc_old != rc_new) fail(label, "filter: return code");
    if (rc_old != want_filter) fail(label, "filter: not the expected code");
    if (text_old != g_error) fail(label, "filter: error text");
    if (std::memcmp(&po, &pn, sizeof po) != 0) fail(label, "filter: plan bytes");
    if (!same_double(r_old, r_new)) fail(label, "filter: radius");
  }
  // the moved warmup_length against the old one, whatever the plans said (only where the table can be read)
  if (ns >= 1 && ns <= vp::DMAXS) {
    double r_old = -7.0, r_new = -7.0;
    const int w_old = old::warmup_length(sos, ns, &r_old), w_new = vp::warmup_length(sos, ns, &r_new);
    if (w_old != w_new) fail(label, "warmup_length");
    if (!same_double(r_old, r_new)) fail(label, "warmup_length: radius");
  }
}

struct Table {
  std::string name;
  int ns, want_decimate;
  std::vector<double> c;
};

static std::vector<Table> read_tables(const char* path) {
  std::vector<Table> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  char name[128], num[128];
  int ns, want;
  while (std::fscanf(f, "%127s %d %d", name, &ns, &want) == 3) {
    Table t{name, ns, want, {}};
    for (int i = 0; i < 6 * ns; ++i) {
      if (std::fscanf(f, "%127s", num) != 1) {
        std::fclose(f);
        return {};
      }
      t.c.push_back(std::strtod(num, nullptr));
    }
    out.push_back(t);
  }
  std::fclose(f);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: sos_host_check TABLES\n");
    return 2;
  }
  const std::vector<Table> tables = read_tables(argv[1]);
  if (tables.empty()) {
    std::printf("DIFFERENT: no tables in %s\n", argv[1]);
    return 1;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int n_long_warmup = 0;

  for (const Table& t : tables) {
    if (t.ns < 1 || t.ns > vp::DMAXS) {
      fail(t.name, "a table of the file has no 1..4 sections");
      continue;
    }
    const double* sos = t.c.data();
    if (t.want_decimate != VP_OK && t.want_decimate != VP_ERR_UNSUPPORTED) fail(t.name, "the file's code for decimation");
    if (t.want_decimate == VP_ERR_UNSUPPORTED) {  // stable, and beyond the halo: decimation alone refuses it
      double r;
      if (vp::warmup_length(sos, t.ns, &r) <= DHALO) fail(t.name, "its warm-up fits the halo");
      ++n_long_warmup;
    }
    // the table as it is, every sample kind, -1 and 3 among them
    for (int kind = -1; kind <= 3; ++kind) {
      const int want = kind >= 0 && kind <= 2 ? VP_OK : VP_ERR_INVALID;
      compare(t.name + " in_kind " + std::to_string(kind), sos, t.ns, kind, want == VP_OK ? t.want_decimate : want, want);
    }
    // n_sections 0 and 5: refused before a coefficient is read
    compare(t.name + " n_sections 0", sos, 0, VP_SAMPLES_FLOAT32, VP_ERR_INVALID, VP_ERR_INVALID);
    compare(t.name + " n_sections 5", sos, 5, VP_SAMPLES_FLOAT32, VP_ERR_INVALID, VP_ERR_INVALID);
    // NaN and inf in every column of every section; a0 = 2
    for (int s = 0; s < t.ns; ++s) {
      for (int i = 0; i < 6; ++i)
        for (const double v : {nan, inf, -inf}) {
          std::vector<double> c = t.c;
          c[6 * s + i] = v;
          compare(t.name + " non-finite at " + std::to_string(s) + "," + std::to_string(i), c.data(), t.ns, VP_SAMPLES_INT32,
                  VP_ERR_INVALID, VP_ERR_INVALID);
        }
      std::vector<double> c = t.c;
      c[6 * s + 3] = 2.0;
      compare(t.name + " a0 = 2 in section " + std::to_string(s), c.data(), t.ns, VP_SAMPLES_FLOAT64, VP_ERR_INVALID,
              VP_ERR_INVALID);
    }
    // one section's poles moved onto the unit circle (a2 = 1, |a1| < 2) and outside it (a2 = 1.21; two real poles, one
    // at -1.5): not stable.  Every section's denominator tail zeroed: radius 0, the warm-up is 2 per section.
    for (int s = 0; s < t.ns; ++s) {
      std::vector<double> c = t.c;
      c[6 * s + 4] = -1.2, c[6 * s + 5] = 1.0;
      compare(t.name + " pole on the circle in section " + std::to_string(s), c.data(), t.ns, VP_SAMPLES_INT32, VP_ERR_INVALID,
              VP_ERR_INVALID);
      c[6 * s + 5] = 1.21;
      compare(t.name + " complex poles outside in section " + std::to_string(s), c.data(), t.ns, VP_SAMPLES_INT32,
              VP_ERR_INVALID, VP_ERR_INVALID);
      c[6 * s + 4] = 2.0, c[6 * s + 5] = 0.75;
      compare(t.name + " real pole outside in section " + std::to_string(s), c.data(), t.ns, VP_SAMPLES_INT32, VP_ERR_INVALID,
              VP_ERR_INVALID);
    }
    {
      std::vector<double> c = t.c;
      for (int s = 0; s < t.ns; ++s) c[6 * s + 4] = c[6 * s + 5] = 0.0;
      double r = -1.0;
      if (vp::warmup_length(c.data(), t.ns, &r) != 2 * t.ns || !(r < 1e-12)) fail(t.name, "zero denominator tail: warm-up is not 2 ns");
      compare(t.name + " zero denominator tail", c.data(), t.ns, VP_SAMPLES_FLOAT32, VP_OK, VP_OK);
    }
  }
  if (tables.size() < 17) fail("tables", "fewer than the 16 Butterworth tables and the long warm-up");
  if (n_long_warmup < 1) fail("tables", "no table with a warm-up beyond the halo");
  static_assert(vp::DMAXS == 4, "the cases are written for kernels of 1..4 sections");
  if (vp::elem_bytes(VP_SAMPLES_INT32) != 4 || vp::elem_bytes(VP_SAMPLES_FLOAT32) != 4 || vp::elem_bytes(VP_SAMPLES_FLOAT64) != 8)
    fail("elem_bytes", "sizes");
  std::printf("%d tables, %d cases: %s\n", (int)tables.size(), g_cases, g_bad ? "DIFFERENT" : "identical");
  return g_bad ? 1 : 0;
}
