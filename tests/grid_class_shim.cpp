// grid_class_shim.cpp — the grid of PT_GEOM_GRID for any margin class, on the host, for tests/test_grid.py.
//
// pt_build_grid (include/ptrace.h) builds the grid pt_set_spheres uploads: margin class 3 (d_near = 3 s0).  pt_tune and
// pt_refit_grid rebuild it for the class the view needs (csrc/pt_api.hip kNearFactors) with the same ptgrid::build.  This
// shim calls that builder with a class of the caller's choice, in either layout, and returns what pt_build_grid and
// pt_grid_walk_constants return for it.  It is compiled by the tests (g++, -ffp-contract=off like the library); that it
// builds the library's grid is checked against pt_build_grid / pt_build_grid_runs / pt_grid_walk_constants at class 3.
#include "../ray_tracer_webgl_amd/csrc/pt_scene_image.hpp"
#include "../include/ptrace.h"

#include <algorithm>
#include <cmath>
#include <vector>

// layout 0: pt_build_grid's (x-fastest runs), 1: pt_build_grid_runs' (Morton runs); walk10 (may be NULL) = {r2_near, lo_n.xyz,
// hi_n.xyz, inv_h.xyz} of the same grid.  PT_ERR_INVALID for a class that is not finite or lies outside [2, 16], or another
// layout; otherwise pt_build_grid's counts and return codes.
extern "C" __attribute__((visibility("default"))) int grid_class_build(
    const PtSphere* s, uint32_t n, double near_factor, int layout, uint32_t* counts8, float* geom12, float* margin4,
    float* delta_g, float* walk10, uint32_t* cells, size_t n_cells, float* entries, size_t entry_floats, uint32_t* entry_index,
    size_t n_index) {
  if (!std::isfinite(near_factor) || near_factor < 2.0 || near_factor > 16.0 || (layout != 0 && layout != 1)) return PT_ERR_INVALID;
  if (!s && n) return PT_ERR_INVALID;
  const ptscene::Split sp = ptscene::split(s, n);
  ptgrid::Grid g;
  if (!sp.regular || !ptgrid::build(sp.geom.data(), sp.radii.data(), n, &g, near_factor)) return PT_ERR_NOT_READY;
  if (layout == 1 && !ptgrid::morton_runs(&g)) return PT_ERR_CAPACITY;
  if (counts8) {
    counts8[0] = g.n[0]; counts8[1] = g.n[1]; counts8[2] = g.n[2]; counts8[3] = g.n_cell_entries;
    counts8[4] = g.n_always; counts8[5] = g.n_entries; counts8[6] = g.max_cell_entries; counts8[7] = g.nonempty;
  }
  if (geom12)
    for (int k = 0; k < 3; k++) { geom12[k] = g.lo[k]; geom12[3 + k] = g.h[k]; geom12[6 + k] = g.hi[k]; geom12[9 + k] = g.c0[k]; }
  if (margin4) { margin4[0] = g.s0; margin4[1] = g.rmin; margin4[2] = g.rmax; margin4[3] = g.d_near; }
  if (delta_g) *delta_g = g.delta_g;
  if (walk10) {
    walk10[0] = g.r2_near;
    for (int k = 0; k < 3; k++) { walk10[1 + k] = g.lo_n[k]; walk10[4 + k] = g.hi_n[k]; walk10[7 + k] = g.inv_h[k]; }
  }
  if ((cells && n_cells < g.cells.size()) || (entries && entry_floats < g.entries.size()) ||
      (entry_index && n_index < g.entry_index.size()))
    return PT_ERR_CAPACITY;
  if (cells) std::copy(g.cells.begin(), g.cells.end(), cells);
  if (entries) std::copy(g.entries.begin(), g.entries.end(), entries);
  if (entry_index) std::copy(g.entry_index.begin(), g.entry_index.end(), entry_index);
  return PT_OK;
}
