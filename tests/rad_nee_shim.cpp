// rad_nee_shim.cpp — the side table of csrc/pt_rad_nee_table.hpp (the radiance-query builds of the next-event estimator) in front
// of ctypes for tests/test_radiance_nee_ref.py, beside what it must leave alone: kNeeKernels and the 14 x 7 trace table.  CPU
// only, no HIP.
#include <cstdint>

#include "../ray_tracer_webgl_amd/csrc/pt_rad_nee_table.hpp"

extern "C" {
int rn_rows(void) { return ROW_COUNT; }
int rn_builds(void) { return BUILD_COUNT; }
int rn_obj_count(void) { return OBJ_COUNT; }
int rn_obj_nee(void) { return OBJ_NEE; }
int rn_obj_rad_nee(void) { return OBJ_RAD_NEE; }
int rn_variants(void) { return PT_VARIANT_COUNT; }
static int cell_out(const TraceCell& k, int* object, int* id, int* waves, const char** name) {
  *object = k.object; *id = k.id; *waves = k.waves; *name = k.name;
  return 0;
}
// a row's cell of the new side table, of kNeeKernels, and of the trace table's column `build`
int rn_cell(int row, int* object, int* id, int* waves, const char** name) {
  return row < 0 || row >= ROW_COUNT ? 1 : cell_out(kRadNeeKernels[row], object, id, waves, name);
}
int rn_nee_cell(int row, int* object, int* id, int* waves, const char** name) {
  return row < 0 || row >= ROW_COUNT ? 1 : cell_out(kNeeKernels[row], object, id, waves, name);
}
int rn_table_cell(int row, int build, int* object, int* id, int* waves, const char** name) {
  return row < 0 || row >= ROW_COUNT || build < 0 || build >= BUILD_COUNT ? 1 : cell_out(kTraceKernels[row][build], object, id, waves, name);
}
// the statement the kernels' attribute reads (csrc/pt_kernels_radiance_nee.hip), for a variant id and its namesake's figure
int rn_waves(int variant_id, int namesake_waves) { return pt_rad_nee_waves(variant_id, namesake_waves); }
int rn_takes_cell(int next_event, int build) { return takes_rad_nee_cell(next_event != 0, build) ? 1 : 0; }
int rn_takes_nee_cell(int next_event, int build) { return takes_nee_cell(next_event != 0, build) ? 1 : 0; }
int rn_reads_ring(int row, int build) { return reads_ring_layout(row, build) ? 1 : 0; }
int rn_build_rad(void) { return BUILD_RAD; }
int rn_row_grid(void) { return ROW_GRID; }
}
