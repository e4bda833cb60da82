// probe_sweep.hpp — THE SWEEP of the probe-lattice tests: one lattice, the record sets and the pixels that tests/probe_shim.cpp
// hands to tests/test_probe_ref.py and tests/probe_main.cpp walks under the sanitizers.  The lattice is 3 x 3 x 4 with a dyadic x
// axis (origin -1.25, step 0.5: g is exactly the node's index at a node), a y axis whose arithmetic rounds (origin 0.1, step 0.3)
// and a z axis of step 1.  The pixels: hit points ON nodes (the first, the last, the inner node (1, 1, 1) that the eight cells
// around it see as each of their corners) and one ulp either side of them per axis and on all axes, points whose g is one ulp
// either side of an index, points below 0 and beyond the last node on every axis, inner points; the six axis normals (the half-space test at dot == 0 and one ulp either side of it,
// with the on-node points) and two oblique ones; every type and an unknown one; a miss.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../include/ptrace.h"

namespace probesweep {

struct Pixel {
  float albedo[3], n[3], hp[3];
  int32_t index, type;
};

inline PtProbeLattice lattice() {
  PtProbeLattice L = {};
  L.origin[0] = -1.25f; L.origin[1] = 0.1f; L.origin[2] = -2.0f;
  L.step[0] = 0.5f; L.step[1] = 0.3f; L.step[2] = 1.0f;
  L.nx = 3; L.ny = 3; L.nz = 4;
  L.flags = 0;
  return L;
}
inline const float* camera() {
  static const float cam[3] = {0.4f, 1.7f, 5.5f};
  return cam;
}

enum { SET_MIXED = 0, SET_INNER_EMPTY, SET_ALL_EMPTY, SET_NEGATIVE, SET_COUNT };
// a set's records, 28 floats per node: coefficients of both signs from a small integer hash (SET_NEGATIVE: band 0 negative and
// dominant, so that every blend is negative and clamps); samples 64, but 0 at node (1, 1, 1) (SET_INNER_EMPTY) or everywhere
inline std::vector<float> records(int set) {
  const PtProbeLattice L = lattice();
  const uint32_t nodes = L.nx * L.ny * L.nz;
  std::vector<float> r((size_t)nodes * 28);
  uint32_t h = 0x9E3779B9u;
  for (uint32_t i = 0; i < nodes; i++) {
    for (int k = 0; k < 27; k++) {
      h = h * 1664525u + 1013904223u;
      float v = (float)((int32_t)(h >> 8) % 2001 - 700) * (1.0f / 512.0f);  // [-1.37, 2.54]
      if (set == SET_NEGATIVE) v = k < 3 ? -8.0f - std::fabs(v) : v * 0.125f;
      r[(size_t)i * 28 + k] = v;
    }
    const bool inner = i == (1u * L.ny + 1u) * L.nx + 1u;
    r[(size_t)i * 28 + 27] = (set == SET_ALL_EMPTY || (set == SET_INNER_EMPTY && inner)) ? 0.0f : 64.0f;
  }
  return r;
}

inline std::vector<Pixel> pixels() {
  const PtProbeLattice L = lattice();
  std::vector<Pixel> out;
  std::vector<std::vector<float>> points;
  auto node = [&](uint32_t ix, uint32_t iy, uint32_t iz) {
    return std::vector<float>{__builtin_fmaf((float)ix, L.step[0], L.origin[0]), __builtin_fmaf((float)iy, L.step[1], L.origin[1]),
                              __builtin_fmaf((float)iz, L.step[2], L.origin[2])};
  };
  const uint32_t on[][3] = {{0, 0, 0}, {2, 2, 3}, {1, 1, 1}, {1, 2, 2}};
  for (const auto& o : on) {
    const std::vector<float> p = node(o[0], o[1], o[2]);
    points.push_back(p);
    for (int axis = 0; axis < 4; axis++)
      for (int dir = -1; dir <= 1; dir += 2) {
        std::vector<float> q = p;
        for (int c = 0; c < 3; c++)
          if (axis == 3 || axis == c) q[c] = std::nextafterf(p[c], dir > 0 ? INFINITY : -INFINITY);
        points.push_back(q);
      }
  }
  // the eight cells around node (1, 1, 1): it is each corner in turn
  for (int k = 0; k < 8; k++) {
    const std::vector<float> p = node(1, 1, 1);
    points.push_back({p[0] + ((k & 1) ? 0.2f : -0.15f), p[1] + ((k & 2) ? 0.11f : -0.07f), p[2] + ((k & 4) ? 0.6f : -0.35f)});
  }
  // g itself one ulp either side of an index, on the dyadic axis: x = origin + step * nextafter(k), exact in fp32 (but below
  // index 1, where x would need a bit more than fp32 has: there g lands on the index or two ulp below it)
  for (int k = 1; k <= 2; k++)
    for (int dir = -1; dir <= 1; dir += 2)
      points.push_back({(float)((double)L.origin[0] + (double)L.step[0] * (double)std::nextafterf((float)k, dir > 0 ? INFINITY : -INFINITY)), 0.3f, -0.5f});
  // below 0 and beyond the last node, axis by axis and on all
  points.push_back({-3.0f, 0.3f, -0.5f});
  points.push_back({4.0f, 0.3f, -0.5f});
  points.push_back({-1.0f, -2.0f, -0.5f});
  points.push_back({-1.0f, 9.0f, -0.5f});
  points.push_back({-1.0f, 0.3f, -7.5f});
  points.push_back({-1.0f, 0.3f, 7.5f});
  points.push_back({-30.0f, -30.0f, -30.0f});
  points.push_back({1e6f, 1e6f, 1e6f});
  const float normals[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0.6f, 0.48f, -0.64f}, {-0.36f, 0.8f, 0.48f}};
  const int32_t types[] = {PT_DIFFUSE, PT_METAL, PT_GLASS, PT_EMISSIVE, 7, -3};
  int serial = 0;
  for (const auto& p : points)
    for (const auto& n : normals)
      for (int32_t type : types) {
        // (every type on the first two normals only: the flat pixels do not read the look-up)
        if (type != PT_DIFFUSE && type != PT_METAL && type != PT_GLASS && &n != &normals[0] && &n != &normals[6]) continue;
        Pixel px;
        px.albedo[0] = 0.25f + 0.125f * (float)(serial % 5); px.albedo[1] = 0.5f; px.albedo[2] = 0.9f - 0.1f * (float)(serial % 3);
        for (int c = 0; c < 3; c++) { px.n[c] = n[c]; px.hp[c] = p[c]; }
        px.index = serial % 7;
        px.type = type;
        out.push_back(px);
        serial++;
      }
  // misses: the background in the albedo plane, zeros elsewhere, ids {-1, -1, -1, 0}
  for (int k = 0; k < 3; k++) {
    Pixel px = {{0.5f + 0.1f * (float)k, 0.7f, 1.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, -1, -1};
    out.push_back(px);
  }
  return out;
}

}  // namespace probesweep
