// C entry points over pt_geom_plan.hpp's choice of the grid kernel's walk, for tests/test_grid_flat.py (host only: no HIP runtime).
#include "../ray_tracer_webgl_amd/csrc/pt_geom_plan.hpp"

extern "C" int shim_grid_walk_flat(int build_kind, uint32_t n_layers_y) { return grid_walk_flat(build_kind, n_layers_y) ? 1 : 0; }

// the build a launch gets (grid_staging, with the LDS room of a walk kernel) and whether it walks flat: kind * 16 + flat
extern "C" int shim_flat_after_staging(uint64_t n_cells, uint32_t n_entries, uint32_t n_layers_y, int cells_build, int fit_state) {
  const Staging st = grid_staging(n_cells, n_entries, walk_lds_room(), cells_build != 0, fit_state);
  return st.kind * 16 + (grid_walk_flat(st.kind, n_layers_y) ? 1 : 0);
}
