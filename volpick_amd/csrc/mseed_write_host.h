// What the miniSEED writer does on the host: the argument checks of vp_mseed_encode, the SEED rate fields, the civil date
// of a record's start and the 64-byte header (fixed section, blockette 1000, blockette 1001).  No HIP:
// tests/mseed_write_host_check.cpp builds it with the host compiler.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "vp_error.h"

namespace vp {

constexpr int MSEED_DATA_OFFSET = 64;        // with or without blockette 1001
constexpr int64_t MSEED_MAX_RECORD_SAMPLES = 65535;  // the header's sample count is 16 bits

inline bool mseed_is_steim(int encoding) { return encoding == 10 || encoding == 11; }

// Data words of a Steim record: 15 per frame, less X0 and Xn.
inline int64_t mseed_steim_words(int reclen) { return 15LL * ((reclen - MSEED_DATA_OFFSET) / 64) - 2; }

// Bytes of one sample of a plain encoding; 0 for anything else.
inline int mseed_plain_width(int encoding) { return encoding == 1 ? 2 : encoding == 3 || encoding == 4 ? 4 : encoding == 5 ? 8 : 0; }

// The most samples one record can hold.
inline int64_t mseed_record_capacity(int reclen, int encoding) {
  if (encoding == 11) return 7 * mseed_steim_words(reclen);
  if (encoding == 10) return 4 * mseed_steim_words(reclen);
  return (reclen - MSEED_DATA_OFFSET) / mseed_plain_width(encoding);
}

// The SEED factor / multiplier of a rate (volpick_hip.h: vp_mseed_rate_fields).
inline bool mseed_rate_fields(double rate, int32_t* factor, int32_t* mult) {
  if (!(rate > 0.0) || !std::isfinite(rate)) return false;
  for (int m = 1; m <= 32767; ++m) {
    const double f = rate * m;
    if (f > 32767.0) break;
    if (f >= 1.0 && f == std::floor(f) && f / m == rate) {
      *factor = (int32_t)f;
      *mult = m == 1 ? 1 : -m;
      return true;
    }
  }
  const double p = 1.0 / rate;
  if (p >= 1.0 && p <= 32767.0 && p == std::floor(p) && 1.0 / p == rate) {
    *factor = -(int32_t)p;
    *mult = 1;
    return true;
  }
  return false;
}

// Microseconds since 1970-01-01 -> year, day of year, time of day, 0.0001 s ticks and the microseconds left over (0..99).
struct MseedTime {
  int year, doy, hour, minute, second, fract, usec;
};
inline MseedTime mseed_time(int64_t us) {
  int64_t days = us / 86400000000LL, rem = us % 86400000000LL;
  if (rem < 0) {
    rem += 86400000000LL;
    --days;
  }
  // civil year of a day count (proleptic Gregorian), by the 400-year cycle from 0000-03-01
  const int64_t z = days + 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const int64_t doe = z - era * 146097;
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int64_t doy_march = doe - (365 * yoe + yoe / 4 - yoe / 100);  // from March 1st
  const int64_t month = (5 * doy_march + 2) / 153;                    // 0 = March
  int64_t year = yoe + era * 400 + (month >= 10 ? 1 : 0);
  const bool leap = (year % 4 == 0 && year % 100 != 0) || year % 400 == 0;
  const int64_t doy = month >= 10 ? doy_march - 306 + 1 : doy_march + 59 + (leap ? 1 : 0) + 1;
  MseedTime t;
  t.year = (int)year;
  t.doy = (int)doy;
  const int64_t sec = rem / 1000000, sub = rem % 1000000;
  t.hour = (int)(sec / 3600);
  t.minute = (int)(sec / 60 % 60);
  t.second = (int)(sec % 60);
  t.fract = (int)(sub / 100);
  t.usec = (int)(sub % 100);
  return t;
}

// Start of the record whose first sample is the trace's sample `pos`.
inline int64_t mseed_record_start(const vp_mseed_trace& tr, int64_t pos) {
  return tr.start_us + (int64_t)std::nearbyint((double)pos * 1e6 / tr.sample_rate);  // halves to even
}

inline int mseed_code_len(const char* s, int cap) {
  int n = 0;
  while (n < cap && s[n]) ++n;
  return n;
}

// The per-call arguments of vp_mseed_encode that need no device.  `who` is the entry point the refusal names.
inline int check_mseed_encode(const char* who, int sample_kind, int reclen, int encoding, int b1001_mode) {
  VP_REQUIRE(reclen >= 128 && reclen <= 65536 && (reclen & (reclen - 1)) == 0,
             "%s: reclen %d is not a power of two in 128..65536", who, reclen);
  const bool ok = sample_kind == VP_SAMPLES_INT32   ? (encoding == 11 || encoding == 10 || encoding == 3 || encoding == 1)
                  : sample_kind == VP_SAMPLES_FLOAT32 ? encoding == 4
                  : sample_kind == VP_SAMPLES_FLOAT64 ? encoding == 5
                                                              : false;
  VP_REQUIRE(ok, "%s: encoding %d cannot hold samples of kind %d (int32: 11, 10, 3, 1; float32: 4; float64: 5)", who, encoding,
             sample_kind);
  VP_REQUIRE(b1001_mode >= -1 && b1001_mode <= 1, "%s: b1001_mode %d is none of -1, 0, 1", who, b1001_mode);
  if (mseed_record_capacity(reclen, encoding) > MSEED_MAX_RECORD_SAMPLES) {
    set_error("%s: a %d-byte record of encoding %d could hold more than %lld samples, beyond the header's 16-bit count", who,
              reclen, encoding, (long long)MSEED_MAX_RECORD_SAMPLES);
    return VP_ERR_UNSUPPORTED;
  }
  return VP_OK;
}

// One trace's header fields: codes that fit, a quality character, a rate the two 16-bit fields can carry.
inline int check_mseed_trace(const char* who, const vp_mseed_trace& tr, int64_t index, int32_t* factor, int32_t* mult) {
  VP_REQUIRE(mseed_code_len(tr.network, 4) <= 2 && mseed_code_len(tr.station, 8) <= 5 && mseed_code_len(tr.location, 4) <= 2 &&
                 mseed_code_len(tr.channel, 4) <= 3,
             "%s: trace %lld: network / station / location / channel longer than 2 / 5 / 2 / 3 characters", who,
             (long long)index);
  VP_REQUIRE(tr.quality == 'D' || tr.quality == 'R' || tr.quality == 'Q' || tr.quality == 'M',
             "%s: trace %lld: data quality %d is none of D, R, Q, M", who, (long long)index, tr.quality);
  VP_REQUIRE(mseed_rate_fields(tr.sample_rate, factor, mult),
             "%s: trace %lld: sampling rate %.17g has no exact SEED factor / multiplier pair", who, (long long)index,
             tr.sample_rate);
  return VP_OK;
}

inline void mseed_put16(uint8_t* p, unsigned v, bool be) {
  p[be ? 0 : 1] = (uint8_t)(v >> 8);
  p[be ? 1 : 0] = (uint8_t)v;
}
inline void mseed_put_code(uint8_t* p, const char* s, int field) {
  const int n = mseed_code_len(s, field);
  for (int i = 0; i < field; ++i) p[i] = i < n ? (uint8_t)s[i] : (uint8_t)' ';
}

// One 64-byte header.
inline void mseed_record_header(uint8_t* h, const vp_mseed_trace& tr, int64_t sequence, int64_t start_us, int count,
                                int32_t factor, int32_t mult, int reclen, int encoding, bool be, bool b1001) {
  std::memset(h, 0, MSEED_DATA_OFFSET);
  int64_t seq = sequence % 1000000;
  for (int i = 5; i >= 0; --i) {
    h[i] = (uint8_t)('0' + seq % 10);
    seq /= 10;
  }
  h[6] = (uint8_t)tr.quality;
  h[7] = ' ';
  mseed_put_code(h + 8, tr.station, 5);
  mseed_put_code(h + 13, tr.location, 2);
  mseed_put_code(h + 15, tr.channel, 3);
  mseed_put_code(h + 18, tr.network, 2);
  const MseedTime t = mseed_time(start_us);
  mseed_put16(h + 20, (unsigned)t.year, be);
  mseed_put16(h + 22, (unsigned)t.doy, be);
  h[24] = (uint8_t)t.hour;
  h[25] = (uint8_t)t.minute;
  h[26] = (uint8_t)t.second;
  mseed_put16(h + 28, (unsigned)t.fract, be);
  mseed_put16(h + 30, (unsigned)count, be);
  mseed_put16(h + 32, (unsigned)(uint16_t)(int16_t)factor, be);
  mseed_put16(h + 34, (unsigned)(uint16_t)(int16_t)mult, be);
  h[39] = b1001 ? 2 : 1;  // blockettes that follow
  mseed_put16(h + 44, MSEED_DATA_OFFSET, be);
  mseed_put16(h + 46, 48, be);
  mseed_put16(h + 48, 1000, be);
  mseed_put16(h + 50, b1001 ? 56 : 0, be);
  h[52] = (uint8_t)encoding;
  h[53] = be ? 1 : 0;
  int exp = 0;
  while ((1 << exp) < reclen) ++exp;
  h[54] = (uint8_t)exp;
  if (b1001) {
    mseed_put16(h + 56, 1001, be);
    h[60] = 100;  // timing quality, per cent
    h[61] = (uint8_t)t.usec;
    const int frames = (reclen - MSEED_DATA_OFFSET) / 64;
    h[63] = frames <= 255 ? (uint8_t)frames : 0;  // (the field is one byte)
  }
}

// Whether the records of one trace carry blockette 1001 under b1001_mode (-1: as soon as one start is off the 100 us grid).
inline bool mseed_wants_b1001(const vp_mseed_trace& tr, const int64_t* rec_first, int64_t n_records, int b1001_mode) {
  if (b1001_mode >= 0) return b1001_mode != 0;
  for (int64_t r = 0; r < n_records; ++r) {
    int64_t m = mseed_record_start(tr, rec_first[r]) % 100;
    if (m != 0) return true;
  }
  return false;
}

// The headers of one trace's records (volpick_hip.h: vp_mseed_record_headers); the trace has passed check_mseed_trace.
inline int mseed_trace_headers(const char* who, const vp_mseed_trace& tr, const int64_t* rec_first, const int64_t* rec_count,
                               int64_t n_records, int64_t first_sequence, int32_t factor, int32_t mult, int reclen, int encoding,
                               bool be, int b1001_mode, uint8_t* headers, int64_t stride) {
  const bool b1001 = mseed_wants_b1001(tr, rec_first, n_records, b1001_mode);
  for (int64_t r = 0; r < n_records; ++r) {
    VP_REQUIRE(rec_first[r] >= 0 && rec_count[r] >= 0 && rec_count[r] <= MSEED_MAX_RECORD_SAMPLES,
               "%s: record %lld: first sample %lld, count %lld", who, (long long)r, (long long)rec_first[r],
               (long long)rec_count[r]);
    mseed_record_header(headers + r * stride, tr, first_sequence + r, mseed_record_start(tr, rec_first[r]), (int)rec_count[r],
                        factor, mult, reclen, encoding, be, b1001);
  }
  return VP_OK;
}

}  // namespace vp
