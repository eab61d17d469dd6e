// Stand-alone run of volpick_amd/csrc/mseed_write_host.h (mseed_rate_fields, mseed_time, mseed_trace_headers, the argument
// checks).  Host compiler only, no HIP; tests/test_mseed_write_cpu.py builds this with -fsanitize=address,undefined and
// runs it.  Arguments come in groups of nine:
//     START_US RATE FIRST COUNT SEQUENCE RECLEN ENCODING BIG_ENDIAN B1001_MODE
// and each prints "header " and the 64 bytes of that one record's header in hex (trace XX.VOLC.00.HHZ, quality D), or
// "refused CODE".  Then one line "check NAME CODE" per argument case below.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mseed_write_host.h"

static char g_error[512];
void vp::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

static vp_mseed_trace trace(long long start_us, double rate, const char* net, const char* sta, const char* loc, const char* cha) {
  vp_mseed_trace t;
  memset(&t, 0, sizeof t);
  t.start_us = start_us;
  t.sample_rate = rate;
  t.nsamples = 1;
  t.quality = 'D';
  strncpy(t.network, net, sizeof t.network);  // (a code that fills its array has no terminator: mseed_code_len stops at the end)
  strncpy(t.station, sta, sizeof t.station);
  strncpy(t.location, loc, sizeof t.location);
  strncpy(t.channel, cha, sizeof t.channel);
  return t;
}

int main(int argc, char** argv) {
  for (int i = 1; i + 8 < argc; i += 9) {
    const vp_mseed_trace t = trace(atoll(argv[i]), atof(argv[i + 1]), "XX", "VOLC", "00", "HHZ");
    const int64_t first = atoll(argv[i + 2]), count = atoll(argv[i + 3]);
    const int reclen = atoi(argv[i + 5]), enc = atoi(argv[i + 6]), be = atoi(argv[i + 7]), mode = atoi(argv[i + 8]);
    int32_t factor = 0, mult = 0;
    int rc = vp::check_mseed_trace("t", t, 0, &factor, &mult);
    uint8_t* h = new uint8_t[64];  // on the heap: the sanitizer sees a write past it
    if (rc == VP_OK)
      rc = vp::mseed_trace_headers("t", t, &first, &count, 1, atoll(argv[i + 4]), factor, mult, reclen, enc, be != 0, mode, h, 64);
    if (rc != VP_OK) {
      printf("refused %d\n", rc);
    } else {
      printf("header ");
      for (int k = 0; k < 64; ++k) printf("%02x", h[k]);
      printf("\n");
    }
    delete[] h;
  }
  int32_t f = 0, m = 0;
  const int I32 = VP_SAMPLES_INT32, F32 = VP_SAMPLES_FLOAT32, F64 = VP_SAMPLES_FLOAT64;
  struct {
    const char* name;
    int rc;
  } cases[] = {
      {"valid_steim2", vp::check_mseed_encode("t", I32, 512, 11, -1)},
      {"valid_steim1_65536", vp::check_mseed_encode("t", I32, 65536, 10, 0)},
      {"valid_int16", vp::check_mseed_encode("t", I32, 128, 1, 1)},
      {"valid_float32", vp::check_mseed_encode("t", F32, 4096, 4, 0)},
      {"valid_float64", vp::check_mseed_encode("t", F64, 4096, 5, 0)},
      {"valid_trace", vp::check_mseed_trace("t", trace(0, 62.5, "XX", "VOLCA", "00", "HHZ"), 0, &f, &m)},
      {"reclen_64", vp::check_mseed_encode("t", I32, 64, 11, 0)},
      {"reclen_not_power", vp::check_mseed_encode("t", I32, 1000, 11, 0)},
      {"reclen_beyond", vp::check_mseed_encode("t", I32, 131072, 11, 0)},
      {"encoding_2", vp::check_mseed_encode("t", I32, 512, 2, 0)},
      {"encoding_text", vp::check_mseed_encode("t", I32, 512, 0, 0)},
      {"float_as_steim", vp::check_mseed_encode("t", F32, 512, 11, 0)},
      {"int_as_float", vp::check_mseed_encode("t", I32, 512, 4, 0)},
      {"kind", vp::check_mseed_encode("t", 7, 512, 11, 0)},
      {"b1001_mode", vp::check_mseed_encode("t", I32, 512, 11, 2)},
      {"steim2_65536", vp::check_mseed_encode("t", I32, 65536, 11, 0)},
      {"station_6", vp::check_mseed_trace("t", trace(0, 100, "XX", "VOLCAN", "00", "HHZ"), 0, &f, &m)},
      {"network_3", vp::check_mseed_trace("t", trace(0, 100, "XXX", "VOLC", "00", "HHZ"), 0, &f, &m)},
      {"location_3", vp::check_mseed_trace("t", trace(0, 100, "XX", "VOLC", "000", "HHZ"), 0, &f, &m)},
      {"channel_4", vp::check_mseed_trace("t", trace(0, 100, "XX", "VOLC", "00", "HHZZ"), 0, &f, &m)},
      {"rate_zero", vp::check_mseed_trace("t", trace(0, 0.0, "XX", "VOLC", "00", "HHZ"), 0, &f, &m)},
      {"rate_negative", vp::check_mseed_trace("t", trace(0, -1.0, "XX", "VOLC", "00", "HHZ"), 0, &f, &m)},
      {"rate_no_pair", vp::check_mseed_trace("t", trace(0, 1e-5, "XX", "VOLC", "00", "HHZ"), 0, &f, &m)},
  };
  for (const auto& c : cases) printf("check %s %d\n", c.name, c.rc);
  return 0;
}
