// Stand-alone driver of volpick_amd/csrc/spectrogram_host.h (check_spectrogram: every argument check of vp_spectrogram, the
// kernel's limits, the frames per workgroup and the LDS layout).  Host compiler only, no HIP; tests/test_spectrogram_f64_cpu.py
// writes the cases, builds this with -fsanitize=address,undefined where the runtime links and runs it:
//     spectrogram_host_check CASES
// CASES: per line  IN_NULL OUT_NULL KIND N_SERIES STRIDE N SAMP_RATE NFFT PAD HOP DBSCALE FIRST COUNT  (SAMP_RATE a C99 hex float,
// nan and inf included).  Per case one line out:  RC NAMED JP TOTAL_FRAMES LDS_BYTES XS_CAP NRES SCALE  -- NAMED is 1 if a
// refusal's text starts with the entry point's name; the plan fields are 0 on a refusal.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "spectrogram_host.h"

static char g_error[512];
void vp::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: spectrogram_host_check CASES\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  static int in_buf[8];
  static float out_buf[8];
  const char* who = "vp_spectrogram";
  int in_null, out_null, kind, n_series, nfft, pad, hop, db;
  long long stride, n, first, count;
  char rate[64];
  int cases = 0;
  while (std::fscanf(f, "%d %d %d %d %lld %lld %63s %d %d %d %d %lld %lld", &in_null, &out_null, &kind, &n_series, &stride, &n,
                     rate, &nfft, &pad, &hop, &db, &first, &count) == 13) {
    vp::SpecPlan p;
    std::memset(&p, 0, sizeof p);
    g_error[0] = 0;
    const int rc = vp::check_spectrogram(who, in_null ? nullptr : in_buf, kind, n_series, stride, n, std::strtod(rate, nullptr),
                                         nfft, pad, hop, db, first, count, out_null ? nullptr : out_buf, &p);
    const int named = std::strncmp(g_error, "vp_spectrogram:", 15) == 0;
    if (rc != VP_OK) std::memset(&p, 0, sizeof p);
    std::printf("%d %d %d %lld %zu %d %d %a\n", rc, named, p.jp, p.total_frames, p.lds_bytes, p.xs_cap, p.nres, p.scale);
    ++cases;
  }
  std::fclose(f);
  std::printf("%d cases\n", cases);
  return 0;
}
