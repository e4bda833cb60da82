// gather_sweep.hpp — the sweep tests/gather_shim.cpp hands to tests/test_gather_ref.py and tests/gather_main.cpp walks under the
// sanitizers: the direction counts, the normals (the axes both ways — (0, 0, -1) is the frame's pole —, unnormalised, tiny, huge
// and denormal ones) and, per D, an item's records with mixed signs and a zero (and, on request, a NaN).  Host only.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../include/ptrace.h"

namespace gathersweep {

inline const std::vector<uint32_t>& direction_counts() {
  static const std::vector<uint32_t> d = {64u, 128u, 4096u};
  return d;
}

struct Normal { float n[3]; };
inline const std::vector<Normal>& normals() {
  static const std::vector<Normal> v = {
      {{1.0f, 0.0f, 0.0f}},   {{-1.0f, 0.0f, 0.0f}},  {{0.0f, 1.0f, 0.0f}},     {{0.0f, -1.0f, 0.0f}},   {{0.0f, 0.0f, 1.0f}},
      {{0.0f, 0.0f, -1.0f}},  {{0.0f, -0.0f, -1.0f}}, {{1e-4f, 0.0f, -1.0f}},   {{3.0f, -4.0f, 12.0f}},  {{-0.3f, 0.2f, -0.1f}},
      {{1e-20f, 2e-20f, -1e-20f}}, {{0.0f, 3e-30f, 0.0f}}, {{1e-41f, 0.0f, 2e-41f}}, {{1e30f, -2e30f, 1e30f}}, {{3e38f, 3e38f, 3e38f}},
      {{0.57735f, 0.57735f, 0.57735f}}, {{-0.0f, 0.0f, 5.0f}},
  };
  return v;
}

// D records: sums of mixed sign, a zero, varying magnitudes; samples 4; with_nan puts one NaN at j = 70 % D's red
inline std::vector<PtRayRadiance> records(uint32_t D, bool with_nan) {
  std::vector<PtRayRadiance> r(D);
  uint32_t x = 0x9e3779b9u ^ D;
  for (uint32_t j = 0; j < D; j++) {
    for (int c = 0; c < 3; c++) {
      x = x * 1664525u + 1013904223u;
      const float mag = std::ldexp((float)(x >> 8) * (1.0f / 16777216.0f), (int)(x & 7u) - 3);
      r[j].sum[c] = (x & 8u) ? -mag : mag;
    }
    r[j].samples = 4.0f;
  }
  r[5].sum[1] = 0.0f;
  r[6].sum[0] = -0.0f;
  if (with_nan) r[70u % D].sum[0] = NAN;
  return r;
}

}  // namespace gathersweep
