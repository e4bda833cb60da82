// gather_main.cpp — a stand-alone program over csrc/pt_gather.hpp for -fsanitize=address,undefined: the sweep of
// tests/gather_sweep.hpp — every j of every direction count, every normal, the reduction over exactly sized heap arrays with
// mixed signs, a zero and a NaN — through the functions the kernels compile.  A direction that is not finite or not of unit
// length, a read past an item's records or an index past the accumulators is a report, not a wrong bit.  And the item span of a
// gather batch (item_span) against the enumeration ray by ray, with the bound that keeps a batch's items inside the workspace.
// tests/test_gather_ref.py builds it and runs it as a child; nothing sanitized is loaded into Python.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_gather.hpp"
#include "gather_sweep.hpp"

static bool unit(const float w[3]) {
  if (!(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]))) return false;
  const double l2 = (double)w[0] * w[0] + (double)w[1] * w[1] + (double)w[2] * w[2];
  return std::fabs(l2 - 1.0) < 1e-5;
}

// item_span against the enumeration ray by ray of the batch [first, first + m) of items of D rays
static bool span_ok(uint32_t first, uint32_t m, uint32_t D, uint32_t plane) {
  const ptgather::ItemSpan s = ptgather::item_span(first, m, D);
  uint32_t lo = 0, hi = 0, done_lo = 0, done_n = 0;
  for (uint64_t ray = first; ray < (uint64_t)first + m; ray++) {
    const uint32_t item = (uint32_t)(ray / D);
    if (ray == first) lo = item;
    hi = item;
    if (ray % D == D - 1u) {
      if (!done_n) done_lo = item;
      done_n++;
    }
  }
  if (!done_n) done_lo = lo;  // (an empty range starts at the first item touched)
  const bool same = s.item0 == lo && s.items == hi - lo + 1u && s.done0 == done_lo && s.done1 == done_lo + done_n;
  const bool fits = s.items <= ptgather::items_per_batch(plane) && s.items <= plane / ptgather::kMinDirections + 2u && s.done0 == s.item0 && s.done1 <= s.item0 + s.items;
  if (!same || !fits) std::printf("gather: item_span(%u, %u, %u) = {%u, %u, %u, %u}, plane %u\n", first, m, D, s.item0, s.items, s.done0, s.done1, plane);
  return same && fits;
}

int main() {
  // every batch of calls of 1 to 5 items, and the last batch (the 64-bit sum) of the largest call there is
  for (uint32_t plane : {64u, 72u, 100u, 4096u})
    for (uint32_t D : {64u, 128u, 256u, 4096u}) {
      for (uint32_t n = 1; n <= 5; n++)
        for (uint32_t first = 0; first < n * D; first += plane)
          if (!span_ok(first, n * D - first < plane ? n * D - first : plane, D, plane)) return 1;
      const uint32_t total = 0xffffffffu / D * D, last = (total - 1u) / plane * plane;
      if (!span_ok(last, total - last, D, plane)) return 1;
    }
  for (uint32_t D : {0u, 63u, 64u, 65u, 128u, 4096u, 4160u})
    if (ptgather::directions_valid(D) != (D == 64u || D == 128u || D == 4096u)) { std::printf("gather: directions_valid(%u)\n", D); return 1; }
  if (ptgather::total_rays(0x4000000u, 64u) != 0ull || ptgather::total_rays(0x3ffffffu, 64u) != 0xffffffc0ull) { std::printf("gather: total_rays\n"); return 1; }
  size_t poles = 0;
  for (uint32_t D : gathersweep::direction_counts()) {
    std::unique_ptr<float[]> sc(new float[2 * D]);
    for (uint32_t j = 0; j < D; j++) {
      const float u = ptgather::turn(j);
      if (!(u >= 0.0f && u < 1.0f)) { std::printf("gather: turn(%u) = %g\n", j, (double)u); return 1; }
      // (libm's sin and cos of a rounded 2 pi, NOT the contract's sincos2pi: this program looks for memory errors and undefined
      // behaviour; its unit-length checks are coarse sanity, and the contract's arithmetic is tests/test_gather_ref.py's to check)
      sc[2 * j] = std::sin(6.2831855f * u);
      sc[2 * j + 1] = std::cos(6.2831855f * u);
      const float a = ptgather::stratum(j, D);
      if (!(a > 0.0f && a < 2.0f)) { std::printf("gather: stratum(%u, %u) = %g\n", j, D, (double)a); return 1; }
      float w[3], Y[9];
      ptgather::sphere_direction(a, sc[2 * j], sc[2 * j + 1], w);
      if (!unit(w)) { std::printf("gather: sphere direction %u of %u\n", j, D); return 1; }
      ptgather::sh_basis(w, Y);
      for (const gathersweep::Normal& n : gathersweep::normals()) {
        PtGatherPoint p = {{0.5f, -1.0f, 2.0f}, 0.0f, {n.n[0], n.n[1], n.n[2]}, 0.0f};
        if (!ptgather::item_valid(p, ptgather::IRRADIANCE)) { std::printf("gather: a sweep normal is invalid\n"); return 1; }
        float z[3];
        ptgather::unit_normal(n.n, z);
        if (!unit(z)) { std::printf("gather: unit_normal(%g, %g, %g)\n", (double)n.n[0], (double)n.n[1], (double)n.n[2]); return 1; }
        poles += z[2] == -1.0f;
        const PtRay r = ptgather::ray_of(p, ptgather::IRRADIANCE, j, D, sc[2 * j], sc[2 * j + 1]);
        const double cosine = (double)r.direction[0] * z[0] + (double)r.direction[1] * z[1] + (double)r.direction[2] * z[2];
        if (!unit(r.direction) || !(cosine > 0.0)) { std::printf("gather: hemisphere direction %u of %u\n", j, D); return 1; }
      }
    }
    // invalid items give the null ray
    for (int kind : {ptgather::IRRADIANCE, ptgather::PROBE}) {
      PtGatherPoint bad = {{0.0f, NAN, 0.0f}, 0.0f, {0.0f, 1.0f, 0.0f}, 0.0f};
      const PtRay r = ptgather::ray_of(bad, kind, 1, D, 0.0f, 1.0f);
      if (ptgather::item_valid(bad, kind) || r.direction[0] != 0.0f || r.direction[1] != 0.0f || r.direction[2] != 0.0f) { std::printf("gather: invalid item\n"); return 1; }
    }
    PtGatherPoint flat = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, -0.0f, 0.0f}, 0.0f};
    if (ptgather::item_valid(flat, ptgather::IRRADIANCE) || !ptgather::item_valid(flat, ptgather::PROBE)) { std::printf("gather: a normal of zeros\n"); return 1; }
    // the reduction over exactly sized arrays
    for (int with_nan = 0; with_nan < 2; with_nan++) {
      const std::vector<PtRayRadiance> rec = gathersweep::records(D, with_nan != 0);
      std::unique_ptr<PtRayRadiance[]> exact(new PtRayRadiance[D]);
      for (uint32_t j = 0; j < D; j++) exact[j] = rec[j];
      std::unique_ptr<float[]> e(new float[4]), sh(new float[28]);
      ptgather::reduce_item(ptgather::IRRADIANCE, exact.get(), D, sc.get(), e.get());
      ptgather::reduce_item(ptgather::PROBE, exact.get(), D, sc.get(), sh.get());
      if (e[3] != 4.0f * (float)D || sh[27] != 4.0f * (float)D) { std::printf("gather: samples\n"); return 1; }
      if ((std::isnan(e[0]) != 0) != (with_nan != 0) || (std::isnan(sh[0]) != 0) != (with_nan != 0)) { std::printf("gather: the NaN\n"); return 1; }
      if (std::isnan(e[1]) || std::isnan(sh[1])) { std::printf("gather: a NaN in another channel\n"); return 1; }
    }
  }
  if (!poles) { std::printf("gather: the sweep misses the frame's pole\n"); return 1; }
  std::printf("gather: ok\n");
  return 0;
}
