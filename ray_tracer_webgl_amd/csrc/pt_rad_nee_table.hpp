// pt_rad_nee_table.hpp — the radiance-query builds of the next-event estimator (pt_query_radiance_nee, pt_gather_irradiance_nee,
// pt_bake_probes_nee; pt_kernels_radiance_nee.hip) as the host knows them: a second SIDE TABLE, beside kNeeKernels of
// pt_nee_table.hpp and made the same way from the PT_VARIANT_ROWS text — a cell's id is its variant row, its name the row's
// symbol with the suffix _rad_nee, its wave count pt_rad_nee_waves' (pt_extra.h), by construction.  No column of kTraceKernels
// and none of PT_TRACE_OBJECTS: cell.object is OBJ_RAD_NEE, behind OBJ_NEE, and pt_api.hip reaches the kernel through
// pt_rad_nee_kernel.  Host only, plain C++: tests/rad_nee_shim.cpp pins it.
#pragma once
#include "pt_nee_table.hpp"

enum { OBJ_RAD_NEE = OBJ_NEE + 1 };

namespace rad_nee_cells {
#define PT_RAD_NEE_CELL(stem, waves, Row, ...) \
  constexpr TraceCell PT_CELL_OF(stem##_rad_nee) = {OBJ_RAD_NEE, PT_VARIANT_ID(stem), pt_rad_nee_waves(PT_VARIANT_ID(stem), waves), #stem "_rad_nee"};
PT_VARIANT_ROWS(PT_RAD_NEE_CELL, )
}  // namespace rad_nee_cells

// by row, as kNeeKernels: the variant row that serves it (a door's launch is steered away from the LDS list walk as a next-event
// render launch is; one build serves the rows `grid` and `grid_layers`, walking three axes over the plain cell array)
#define PT_RAD_NEE_K(stem) rad_nee_cells::cell_pt_trace_kernel##stem##_rad_nee
constexpr TraceCell kRadNeeKernels[ROW_COUNT] = {
    PT_RAD_NEE_K(_scalar),   PT_RAD_NEE_K(_scalar),     PT_RAD_NEE_K(_scalar_nolds), PT_RAD_NEE_K(_small_t0),  PT_RAD_NEE_K(_small_t1),
    PT_RAD_NEE_K(_small_t2), PT_RAD_NEE_K(_small_t3),   PT_RAD_NEE_K(_bvh),          PT_RAD_NEE_K(_bvh_nodes), PT_RAD_NEE_K(_bvh_gmem),
    PT_RAD_NEE_K(_grid),     PT_RAD_NEE_K(_grid_cells), PT_RAD_NEE_K(_grid_gmem),    PT_RAD_NEE_K(_grid),
};

// Does a door's launch take this table's cell?  Where the entry point asked for the estimator (LaunchUse::next_event, which only
// the three _nee calls set) and the column would have been the radiance build.
inline bool takes_rad_nee_cell(bool next_event, int build) { return next_event && build == BUILD_RAD; }
