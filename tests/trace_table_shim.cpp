// trace_table_shim.cpp — the trace kernels' table and the three decisions a launch takes of it (csrc/pt_trace_table.hpp) behind
// C entries, for tests/test_trace_builds.py.  Compiled by the tests with g++: the header is host-only.
#include "../ray_tracer_webgl_amd/csrc/pt_trace_table.hpp"

#define TT_API extern "C" __attribute__((visibility("default")))

// out2 = {rows, columns} of the table
TT_API void tt_shape(int* out2) {
  out2[0] = (int)(sizeof kTraceKernels / sizeof kTraceKernels[0]);
  out2[1] = (int)(sizeof kTraceKernels[0] / sizeof kTraceKernels[0][0]);
}

// the number of code objects; out[object] = the number of ids its accessor takes
TT_API int tt_objects(int* out) {
#define TT_IDS(object, accessor, n_ids) out[OBJ_##object] = n_ids;
  PT_TRACE_OBJECTS(TT_IDS)
  return OBJ_COUNT;
}

// the cell's kernel name; out3 = {object, id, waves}
TT_API const char* tt_cell(int row, int build, int* out3) {
  const TraceCell& k = kTraceKernels[row][build];
  out3[0] = k.object;
  out3[1] = k.id;
  out3[2] = k.waves;
  return k.name;
}

TT_API int tt_row(int path, uint32_t n_spheres, int staging_kind, uint32_t grid_layers_y) {
  return trace_row(path, n_spheres, staging_kind, grid_layers_y);
}

TT_API int tt_build(int features, int overlay, int roulette, int count_work) {
  return trace_build(features != 0, overlay != 0, roulette != 0, count_work != 0);
}

// the column of a door launch; door: 0 none / 1 pt_render_features / 2 pt_query_rays / 3 pt_query_radiance
TT_API int tt_door_build(int door) { return door_build((Door)door); }

TT_API int tt_reads_ring_layout(int row, int build) { return reads_ring_layout(row, build); }
