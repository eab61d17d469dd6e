// What vp_spectrogram checks and plans on the host before it touches the device: every argument, the kernel's limits, the
// frames a workgroup owns and its LDS layout.  No HIP: tests/spectrogram_host_check.cpp builds it with the host compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sos_host.h"  // check_sample_kind, elem_bytes

namespace vp {

constexpr int SPEC_MIN_NFFT = 32, SPEC_MAX_NFFT = 512;  // window lengths the frame kernel takes
constexpr int SPEC_MAX_RATIO = 16;                      // pad / nfft
constexpr int SPEC_MAX_PAD = 4096;
constexpr int SPEC_IMAGE = 4096;                        // complex elements of a workgroup's FFT image
constexpr size_t SPEC_LDS_LIMIT = 160 * 1024;

struct SpecPlan {
  int nfft, lg, pad, ratio, nres, hop, jp, lgjp, xs_cap;
  long long total_frames;
  size_t table_elems;  // complex: nres * nfft twisted windows, then nfft / 2 unit roots
  size_t lds_bytes;
  double scale;        // 1 / (samp_rate * sum w^2)
};

inline bool spec_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// Every argument of vp_spectrogram but the device index; fills *p.  `who` is the entry point the refusal names.
inline int check_spectrogram(const char* who, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                             double samp_rate, int nfft, int pad, int hop, int dbscale, int64_t first_frame, int64_t n_frames,
                             const float* out_dev, SpecPlan* p) {
  VP_REQUIRE(in_dev && out_dev, "%s: null argument", who);
  if (const int rc = check_sample_kind(who, in_kind)) return rc;
  VP_REQUIRE(n_series >= 1, "%s: n_series = %d, need at least one series", who, n_series);
  VP_REQUIRE(std::isfinite(samp_rate) && samp_rate > 0.0, "%s: samp_rate = %g is not finite and positive", who, samp_rate);
  VP_REQUIRE(spec_pow2(nfft) && spec_pow2(pad) && pad >= nfft, "%s: nfft = %d, pad = %d: need powers of two with pad >= nfft", who,
             nfft, pad);
  VP_REQUIRE(hop >= 1 && hop <= nfft, "%s: hop = %d outside [1, nfft = %d]", who, hop, nfft);
  VP_REQUIRE(n >= nfft, "%s: n = %lld samples, shorter than one window of nfft = %d", who, (long long)n, nfft);
  VP_REQUIRE(series_stride >= n, "%s: series_stride = %lld below n = %lld", who, (long long)series_stride, (long long)n);
  VP_REQUIRE(dbscale == 0 || dbscale == 1, "%s: dbscale = %d, need 0 or 1", who, dbscale);
  const long long total = ((long long)n - (nfft - hop)) / hop;
  VP_REQUIRE(first_frame >= 0 && n_frames >= 0 && first_frame <= total && n_frames <= total - first_frame,
             "%s: first_frame = %lld, n_frames = %lld: a range outside [0, %lld]", who, (long long)first_frame, (long long)n_frames,
             total);
  if (nfft < SPEC_MIN_NFFT || nfft > SPEC_MAX_NFFT || pad / nfft > SPEC_MAX_RATIO || pad > SPEC_MAX_PAD || n_series > 65535 ||
      n > ((int64_t)1 << 40)) {
    set_error("%s: nfft = %d, pad = %d, n_series = %d, n = %lld: the kernel takes nfft %d..%d, pad / nfft up to %d, pad up to %d, "
              "65535 series of up to 2^40 samples", who, nfft, pad, n_series, (long long)n, SPEC_MIN_NFFT, SPEC_MAX_NFFT,
              SPEC_MAX_RATIO, SPEC_MAX_PAD);
    return VP_ERR_UNSUPPORTED;
  }
  p->nfft = nfft;
  p->pad = pad;
  p->hop = hop;
  p->ratio = pad / nfft;
  p->nres = p->ratio / 2 + 1;
  p->lg = 0;
  while ((1 << p->lg) < nfft) ++p->lg;
  p->jp = SPEC_IMAGE / nfft < VP_SPECTROGRAM_TILE_FRAMES ? SPEC_IMAGE / nfft : VP_SPECTROGRAM_TILE_FRAMES;
  p->lgjp = 0;
  while ((1 << p->lgjp) < p->jp) ++p->lgjp;
  if ((long long)n_frames / p->jp >= 0x7fffffffLL) {
    set_error("%s: %lld frames are beyond one launch (%d frames per workgroup, 2^31 - 1 workgroups): take them in ranges", who,
              (long long)n_frames, p->jp);
    return VP_ERR_UNSUPPORTED;
  }
  p->xs_cap = (p->jp - 1) * hop + nfft;
  p->xs_cap += p->xs_cap & 1;  // the complex tables behind the samples stay 16-byte aligned
  p->total_frames = total;
  p->table_elems = (size_t)p->nres * nfft + nfft / 2;
  p->lds_bytes = sizeof(double) * ((size_t)p->xs_cap + 2 * p->table_elems + 2 * (size_t)p->jp * (nfft + 1));
  if (p->lds_bytes > SPEC_LDS_LIMIT) {
    set_error("%s: nfft = %d, pad = %d, hop = %d need %zu bytes of LDS, a workgroup has %zu", who, nfft, pad, hop, p->lds_bytes,
              SPEC_LDS_LIMIT);
    return VP_ERR_UNSUPPORTED;
  }
  double sw2 = 0.0;  // np.hanning(nfft): 0.5 - 0.5 cos(2 pi i / (nfft - 1))
  for (int i = 0; i < nfft; ++i) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)(nfft - 1));
    sw2 += w * w;
  }
  p->scale = 1.0 / samp_rate / sw2;
  return VP_OK;
}

}  // namespace vp
