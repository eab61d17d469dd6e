// Stand-alone run of volpick_amd/csrc/stalta_host.h (stalta_rec_table, check_sta_lta).  Host compiler only, no HIP;
// tests/test_stalta_f64_cpu.py builds this with -fsanitize=address,undefined and runs it:   stalta_host_check NSTA NLTA ...
// Per pair a line "table NSTA NLTA" and per state a line of c, a and the 16 powers as C99 hex floats; then one line
// "check NAME CODE" per argument case below.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stalta_host.h"

static char g_error[512];
void vp::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const long long nsta = atoll(argv[i]), nlta = atoll(argv[i + 1]);
    vp::StaLtaRec* r = new vp::StaLtaRec;  // on the heap: the sanitizer sees a write past either array
    vp::stalta_rec_table(nsta, nlta, r);
    printf("table %lld %lld\n", nsta, nlta);
    for (int s = 0; s < 2; ++s) {
      printf("%a %a", r->c[s], r->a[s]);
      for (int k = 0; k < vp::STALTA_LEVELS; ++k) printf(" %a", r->pw[s][k]);
      printf("\n");
    }
    delete r;
  }
  std::vector<float> in(64), out(64);
  const void* a = in.data();
  void* b = out.data();
  const int F32 = VP_SAMPLES_FLOAT32, REC = VP_STALTA_RECURSIVE;
  struct {
    const char* name;
    int rc;
  } cases[] = {
      {"valid", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 5, 20, b, F32)},
      {"valid_empty", vp::check_sta_lta("t", nullptr, F32, 1, 0, 0, REC, 5, 20, nullptr, F32)},
      {"valid_three_series", vp::check_sta_lta("t", a, F32, 3, 21, 20, VP_STALTA_CLASSIC, 1, 1, b, VP_SAMPLES_FLOAT64)},
      {"valid_nlta_at_limit", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 5, 65536, b, F32)},
      {"null_in", vp::check_sta_lta("t", nullptr, F32, 1, 64, 64, REC, 5, 20, b, F32)},
      {"null_out", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 5, 20, nullptr, F32)},
      {"in_kind", vp::check_sta_lta("t", a, 7, 1, 64, 64, REC, 5, 20, b, F32)},
      {"out_kind_int32", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 5, 20, b, VP_SAMPLES_INT32)},
      {"type", vp::check_sta_lta("t", a, F32, 1, 64, 64, 2, 5, 20, b, F32)},
      {"negative_n", vp::check_sta_lta("t", a, F32, 1, 64, -1, REC, 5, 20, b, F32)},
      {"no_series", vp::check_sta_lta("t", a, F32, 0, 64, 64, REC, 5, 20, b, F32)},
      {"stride_below_n", vp::check_sta_lta("t", a, F32, 2, 31, 32, REC, 5, 20, b, F32)},
      {"nsta_zero", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 0, 20, b, F32)},
      {"nsta_above_nlta", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 21, 20, b, F32)},
      {"overlap", vp::check_sta_lta("t", a, F32, 1, 32, 32, REC, 5, 20, in.data() + 16, F32)},
      {"overlap_second_series", vp::check_sta_lta("t", a, F32, 2, 32, 16, REC, 5, 20, in.data() + 40, F32)},
      {"nlta_beyond_limit", vp::check_sta_lta("t", a, F32, 1, 64, 64, REC, 5, 65537, b, F32)},
  };
  for (const auto& c : cases) printf("check %s %d\n", c.name, c.rc);
  return 0;
}
