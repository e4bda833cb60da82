// pt_error_plan.hpp — the host arithmetic of the error estimate (include/ptrace.h PT_OPT_ERROR_ESTIMATE, pt_render_adaptive;
// DESIGN.md §4.8b, §4.8c): the frame's figures from the tile records, THE SELECTION RULE, a tile's in-image pixels.  Host only:
// no HIP, no context, so tests/error_plan_shim.cpp can hold it against tests/error_ref.py and tests/adaptive_ref.py without a
// device.  The API side launches the tile kernel, copies and synchronises, then calls in here.
//
// `h`: what pt_error_tiles_kernel wrote, four floats per entry — the records {sum e, sum m2, counted lanes, min n over counted
// lanes} of tiles [0, n_tiles), then the tallies {short pixels, uncounted pixels with n >= 2, max n over counted lanes, -} of the
// same tiles at [n_tiles, 2 n_tiles).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ptrace.h"

namespace pterr {

// pt_error_stats: the records added in tile index order, in double.  Fills every field but passes_rendered and reached.
inline void sum_tiles(const float* h, size_t n_tiles, uint64_t pixels, PtErrorStats* out) {
  double E = 0.0, M = 0.0;
  uint64_t counted = 0, n_short = 0, n_bad = 0;
  float nmin = 0.f, nmax = 0.f;
  for (size_t t = 0; t < n_tiles; t++) {
    const float* r = h + 4 * t;
    const float* a = h + 4 * (n_tiles + t);
    E += (double)r[0];
    M += (double)r[1];
    if (r[2] > 0.0f) {
      nmin = counted ? std::fmin(nmin, r[3]) : r[3];
      nmax = std::fmax(nmax, a[2]);
    }
    counted += (uint64_t)r[2];
    n_short += (uint64_t)a[0];
    n_bad += (uint64_t)a[1];
  }
  out->sum_e2 = E;
  out->sum_m2 = M;
  out->rel_error = M > 0.0 ? std::sqrt(E / M) : 0.0;
  out->rms_error = counted ? std::sqrt(E / (3.0 * (double)counted)) : 0.0;
  out->pixels = pixels;
  out->pixels_counted = counted;
  out->pixels_short = n_short;
  out->pixels_nonfinite = n_bad;
  out->passes_min = nmin < 4294967040.0f ? (uint32_t)nmin : 0xffffffffu;  // (the largest float below 2^32)
  out->passes_max = nmax < 4294967040.0f ? (uint32_t)nmax : 0xffffffffu;
}

// pt_render_until's and pt_render_adaptive's stop
inline bool target_reached(const PtErrorStats& st, float target) { return st.rel_error <= (double)target && st.pixels_short == 0; }

// THE SELECTION RULE (include/ptrace.h), on the records and tallies sum_tiles has just added up; flags[t] = 1 for an active tile,
// returns the active count
inline uint32_t select_tiles(const PtErrorStats& st, float target, const float* h, size_t n_tiles, uint32_t* flags) {
  const double tau = (double)target;
  const double t2 = tau * tau;
  const double b = t2 * st.sum_m2;
  const double Cd = (double)st.pixels_counted;
  uint32_t n_active = 0;
  for (size_t t = 0; t < n_tiles; t++) {
    const double lhs = (double)h[4 * t] * Cd;
    const double rhs = b * (double)h[4 * t + 2];
    const bool active = h[4 * (n_tiles + t)] > 0.0f || lhs > rhs;
    flags[t] = active ? 1u : 0u;
    n_active += active ? 1u : 0u;
  }
  return n_active;
}

// in-image pixels of tile t of a width x rows image of tiles_x tiles per row
inline uint32_t tile_pixels(uint32_t width, uint32_t rows, uint32_t tiles_x, uint32_t t) {
  const uint32_t x0 = 8u * (t % tiles_x), y0 = 8u * (t / tiles_x);
  const uint32_t w = width > x0 ? (width - x0 < 8u ? width - x0 : 8u) : 0u;
  const uint32_t h = rows > y0 ? (rows - y0 < 8u ? rows - y0 : 8u) : 0u;
  return w * h;
}

// pt_resolve_filtered: the rows a pixel of local row ly may look at — its own chunk of band_rows consecutive
// image rows, as first and last LOCAL row (the last chunk of a band may be partial).  band_rows == 0: the context is no band,
// every local row.  ly < local_rows.  (constexpr: pt_filter_kernel computes its row range with this very function.)
struct ChunkRows { uint32_t first, last; };
constexpr ChunkRows chunk_rows(uint32_t ly, uint32_t band_rows, uint32_t local_rows) {
  if (band_rows == 0u) return ChunkRows{0u, local_rows - 1u};
  const uint32_t first = ly / band_rows * band_rows;
  const uint32_t left = local_rows - first;            // rows from `first` to the end: at least 1
  return ChunkRows{first, first + (left < band_rows ? left : band_rows) - 1u};
}

}  // namespace pterr
