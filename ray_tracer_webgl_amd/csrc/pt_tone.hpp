// pt_tone.hpp — EXPOSURE METERING AND THE TONE CURVES (include/ptrace.h pt_meter / pt_resolve_toned have the statement lists;
// DESIGN.md §4.8k), written once for the device and the host: pt_kernels_display.hip runs it per thread over device memory,
// pt_exposure_solve (pt_api.hip) is kernel 2's solve on the host, tests/tone_shim.cpp and tests/tone_main.cpp run all of it over
// host arrays (the latter exactly sized, under the sanitizers).
// fp32, ONE IEEE operation per statement, nothing fused (-ffp-contract=off), `/` and sqrt correctly rounded; the counts are
// integers.  No HIP header needed.
#pragma once
#include <stdint.h>

#include "../../include/ptrace.h"

#if defined(__HIPCC__)
#define PT_TONE_HD __host__ __device__ __forceinline__
#else
#define PT_TONE_HD inline
#endif

namespace pttone {

struct alignas(16) F4 { float x, y, z, w; };

// the tallies of one metering: 256 bins, then the pixels below the first bin, then the pixels looked at (lit + below)
constexpr uint32_t kBins = 256u, kBelow = 256u, kMetered = 257u, kTallies = 258u;
constexpr uint32_t kBin0 = 888u;  // bits(2^-16) >> 20

PT_TONE_HD uint32_t f2u(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
PT_TONE_HD float u2f(uint32_t u) { union { float f; uint32_t u; } c; c.u = u; return c.f; }

// the read-outs' divisor (pt_kernels.hip pixel_scale): the pixel's own sample count
PT_TONE_HD float pixel_scale(float w) { return w > 0.0f ? 1.0f / w : 0.0f; }

// the linear colour of a source texel: an accumulation texel {sums, count} or an external linear texel (its .w is not read)
PT_TONE_HD void source_colour(const F4 v, bool from_accum, float x[3]) {
  x[0] = v.x; x[1] = v.y; x[2] = v.z;
  if (from_accum) {
    const float scale = pixel_scale(v.w);
    x[0] = v.x * scale; x[1] = v.y * scale; x[2] = v.z * scale;
  }
}

PT_TONE_HD float luminance(const float x[3]) {
  float Y = 0.2126f * x[0];
  float t = 0.7152f * x[1];
  Y = Y + t;
  t = 0.0722f * x[2];
  Y = Y + t;
  return Y;
}

// the tally a luminance is counted in: its bin, or kBelow (zero, negative, NaN, subnormal, too dark)
PT_TONE_HD uint32_t tally_of(float Y) {
  if (!(Y >= 0x1p-16f)) return kBelow;
  uint32_t k = (f2u(Y) >> 20) - kBin0;
  if (k > 255u) k = 255u;
  return k;
}

// the lower edge of bin k (k = 256: 2^16, the end of the last bin)
PT_TONE_HD float bin_edge(uint32_t k) { return u2f((k + kBin0) << 20); }

// pt_band_row (pt_host.cpp): the image row of a context's local row
PT_TONE_HD uint32_t band_row(uint32_t band_rows, uint32_t band_index, uint32_t band_count, uint32_t local_row) {
  if (band_count <= 1u || band_rows == 0u) return local_row;
  return (local_row / band_rows * band_count + band_index) * band_rows + local_row % band_rows;
}

// the metering window in image coordinates and the rows this context holds
struct Window {
  uint32_t x0, y0, w, h;  // w == 0 or h == 0: the whole frame
  uint32_t band_rows, band_index, band_count;
};

// is local pixel (px, ly) metered?  The differences cannot wrap, so a window that reaches past the frame ends at the frame.
PT_TONE_HD bool in_window(const Window& win, uint32_t px, uint32_t ly) {
  if (win.w == 0u || win.h == 0u) return true;
  if (px < win.x0 || px - win.x0 >= win.w) return false;
  const uint32_t y = band_row(win.band_rows, win.band_index, win.band_count, ly);
  return y >= win.y0 && y - win.y0 < win.h;
}

PT_TONE_HD bool finite_positive(float v) { return v > 0.0f && v < __builtin_inff(); }

// PT_ERR_INVALID's cases of PtMeterOptions (the window is never invalid)
PT_TONE_HD bool meter_options_valid(const PtMeterOptions& o) {
  if (!finite_positive(o.key) || !finite_positive(o.e_min) || !finite_positive(o.e_max) || !finite_positive(o.white_min)) return false;
  if (o.e_min > o.e_max) return false;
  if (o.key_permille > 1000u || o.high_permille > 1000u || o.key_permille > o.high_permille) return false;
  return o.rate == o.rate;  // (not NaN)
}

// the smallest bin whose cumulative count exceeds `rank` (rank < N = the sum of the bins)
template <class Hist>
PT_TONE_HD uint32_t bin_of_rank(const Hist& hist, uint64_t rank) {
  uint64_t cum = 0;
  for (uint32_t k = 0; k < kBins; k++) {
    cum += hist[k];
    if (cum > rank) return k;
  }
  return kBins - 1u;
}

// KERNEL 2: the record of a metering from its tallies and the record before it (`before` is read only when was_valid)
template <class Hist>
PT_TONE_HD PtExposure solve(const Hist& hist, uint32_t below, const PtMeterOptions& o, bool was_valid, const PtExposure& before) {
  PtExposure r;
  r.exposure = was_valid ? before.exposure : 1.0f;
  r.white = was_valid ? before.white : o.white_min;
  r.y_key = was_valid ? before.y_key : 0.0f;
  r.y_high = was_valid ? before.y_high : 0.0f;
  r.lit = 0;
  r.below = below;
  r.meterings = (was_valid ? before.meterings : 0u) + 1u;
  const float e_prev = r.exposure;
  uint64_t N = 0;
  for (uint32_t k = 0; k < kBins; k++) N += hist[k];
  if (N == 0) return r;
  uint64_t rank_key = (N * (uint64_t)o.key_permille) / 1000u;
  if (rank_key > N - 1u) rank_key = N - 1u;
  uint64_t rank_high = (N * (uint64_t)o.high_permille) / 1000u;
  if (rank_high > N - 1u) rank_high = N - 1u;
  const float y_key = bin_edge(bin_of_rank(hist, rank_key));
  const float y_high = bin_edge(bin_of_rank(hist, rank_high));
  float e_t = o.key / y_key;
  if (e_t < o.e_min) e_t = o.e_min;
  if (e_t > o.e_max) e_t = o.e_max;
  float e;
  if (was_valid && o.rate < 1.0f) {
    if (!(o.rate > 0.0f)) {
      e = e_prev;
    } else {
      float d = e_t - e_prev;
      d = d * o.rate;
      e = e_prev + d;
    }
  } else {
    e = e_t;
  }
  float white = y_high * e;
  if (!(white >= o.white_min)) white = o.white_min;
  r.exposure = e;
  r.white = white;
  r.y_key = y_key;
  r.y_high = y_high;
  r.lit = N;
  return r;
}

// the curve of one channel, x already exposed; w2 = white * white
PT_TONE_HD float curve(int32_t which, float x, float w2) {
  if (which == PT_TONE_REINHARD) {
    float a = x / w2;
    a = a + 1.0f;
    const float n = x * a;
    const float d = x + 1.0f;
    return n / d;
  }
  if (which == PT_TONE_FILMIC) {
    float a = 2.51f * x;
    a = a + 0.03f;
    const float n = x * a;
    float b = 2.43f * x;
    b = b + 0.59f;
    float d = x * b;
    d = d + 0.14f;
    return n / d;
  }
  return x;
}

// the toned colour of a linear colour: exposed, through the curve, then the square root when gamma != 0
PT_TONE_HD void tone(const float x[3], int32_t which, int gamma, float exposure, float white, float y[3]) {
  const float w2 = white * white;
  for (int c = 0; c < 3; c++) {
    const float xe = x[c] * exposure;
    float v = curve(which, xe, w2);
    if (gamma) v = __builtin_sqrtf(v);
    y[c] = v;
  }
}

// the read-outs' byte (pt_kernels.hip unorm8)
PT_TONE_HD uint32_t unorm8(float v) {
  if (!(v > 0.0f)) return 0u;
  if (v >= 1.0f) return 255u;
  float t = v * 255.0f;
  t = t + 0.5f;
  return (uint32_t)t;
}

PT_TONE_HD uint32_t pack_rgba8(const float y[3]) { return unorm8(y[0]) | (unorm8(y[1]) << 8) | (unorm8(y[2]) << 16) | (255u << 24); }

}  // namespace pttone
