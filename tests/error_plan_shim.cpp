// error_plan_shim.cpp — the host arithmetic of the error estimate (csrc/pt_error_plan.hpp) behind C entries, for
// tests/test_error_plan.py.  Compiled by the tests with g++: the header is host only.  `h`: n_tiles records of four floats, then
// n_tiles tallies of four floats, as pt_error_stats copies them from the device.
#include "../ray_tracer_webgl_amd/csrc/pt_error_plan.hpp"

#define SHIM extern "C" __attribute__((visibility("default")))

SHIM void error_plan_stats(const float* h, uint64_t n_tiles, uint64_t pixels, PtErrorStats* out) {
  pterr::sum_tiles(h, (size_t)n_tiles, pixels, out);
}

SHIM int error_plan_reached(const PtErrorStats* st, float target) { return pterr::target_reached(*st, target) ? 1 : 0; }

SHIM uint32_t error_plan_select(const PtErrorStats* st, float target, const float* h, uint64_t n_tiles, uint32_t* flags) {
  return pterr::select_tiles(*st, target, h, (size_t)n_tiles, flags);
}

SHIM uint32_t error_plan_tile_pixels(uint32_t width, uint32_t rows, uint32_t tiles_x, uint32_t t) {
  return pterr::tile_pixels(width, rows, tiles_x, t);
}
