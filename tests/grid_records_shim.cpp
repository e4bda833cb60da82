// grid_records_shim.cpp — C entry points over csrc/pt_grid_records.hpp (the device form of a grid cell record and the ring
// layout of a one-layer grid) for tests/test_grid_records.py; host only, no HIP runtime.  Built by the test with
// -DPT_DEV_KNOBS: ptgrid::build then reads its cell-edge scale from PT_GRID_EDGE, which is how the test gets the library's own
// builder to make grids of 1 x 1 x 1 and 2 x 1 x 3 cells.
#include "../ray_tracer_webgl_amd/csrc/pt_scene_image.hpp"
#include "../include/ptrace.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define SHIM extern "C" __attribute__((visibility("default")))

SHIM uint32_t rec_from_host(uint32_t host_rec) { return ptrec::from_host(host_rec); }
SHIM uint32_t rec_to_host(uint32_t rec) { return ptrec::to_host(rec); }
SHIM uint32_t rec_none() { return ptrec::kNone; }
SHIM int rec_fits(uint32_t n_entries) { return ptrec::fits(n_entries) ? 1 : 0; }

// The (base, mask) of every round a lane runs on the device record `rec`, all G candidates passing: `fast` != 0 the way the
// kernels' G = 4 path takes it (short_mask4 for everybody, the long branch for a set sign bit), otherwise through round_mask /
// next (any G).  Returns the number of rounds (at most cap are written).
SHIM uint32_t rec_rounds(uint32_t rec, uint32_t G, int fast, uint32_t* base, uint32_t* mask, uint32_t cap) {
  uint32_t n = 0;
  while (rec >= ptrec::kNone) {  // `has`: a cell under test
    const uint32_t cand = (1u << G) - 1u;
    uint32_t m, nx;
    if (fast) {
      m = ptrec::short_mask4(rec, cand);
      nx = 0u;
      if (ptrec::is_long(rec)) { m = cand; nx = ptrec::next_long4(rec); }
    } else {
      m = cand & ptrec::round_mask(rec, G);
      nx = ptrec::next(rec, G);
    }
    if (n < cap) { base[n] = ptrec::first_of(rec); mask[n] = m; }
    n++;
    rec = nx;
  }
  return n;
}

SHIM uint64_t ring_cells(uint32_t nx, uint32_t nz) { return ptrec::ring_cells(nx, nz); }
SHIM uint32_t ring_index(uint32_t nx, uint32_t cx, uint32_t cz) { return ptrec::ring_index(nx, cx, cz); }
SHIM uint32_t ring_outside() { return ptrec::kOutside; }
SHIM void ring_layout(const uint32_t* host_cells, uint32_t nx, uint32_t nz, uint32_t* out) { ptrec::ring_layout(host_cells, nx, nz, out); }

// ptgrid::build on a sphere list with the cell edge scaled by edge_scale (<= 0: as the library builds it): n3 = cells per
// axis, cells = the host records (cap of them at most)
SHIM int records_build_grid(const PtSphere* s, uint32_t n, double edge_scale, uint32_t* n3, uint32_t* cells, size_t cap) {
  const ptscene::Split sp = ptscene::split(s, n);
  if (edge_scale > 0.0) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", edge_scale);
    setenv("PT_GRID_EDGE", buf, 1);
  } else {
    unsetenv("PT_GRID_EDGE");
  }
  ptgrid::Grid g;
  const bool ok = ptgrid::build(sp.geom.data(), sp.radii.data(), n, &g);
  unsetenv("PT_GRID_EDGE");
  if (!ok) return PT_ERR_NOT_READY;
  for (int k = 0; k < 3; k++) n3[k] = g.n[k];
  if (g.cells.size() > cap) return PT_ERR_CAPACITY;
  for (size_t k = 0; k < g.cells.size(); k++) cells[k] = g.cells[k];
  return PT_OK;
}
