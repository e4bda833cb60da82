// pt_nee_table.hpp — the next-event builds (PT_OPT_NEXT_EVENT; pt_kernels_nee.hip) as the host knows them: a SIDE TABLE beside
// the trace table of pt_trace_table.hpp, one cell per row, made from the same PT_VARIANT_ROWS text — a cell's id is its variant
// row, its name the row's symbol with the suffix _nee, its wave count pt_nee_waves' (pt_extra.h), by construction.  The builds
// are no column of kTraceKernels and their object is none of PT_TRACE_OBJECTS: cell.object is OBJ_NEE, outside that list, and
// pt_api.hip reaches the kernel through pt_nee_kernel.  Host only, plain C++: tests/nee_shim.cpp pins it.
#pragma once
#include "pt_trace_table.hpp"

enum { OBJ_NEE = OBJ_COUNT };
// what pt_last_trace_build reports for a next-event launch: outside the table's columns (abi.py BUILD_NEXT_EVENT)
enum { BUILD_NEXT_EVENT = 16 };
static_assert((int)BUILD_NEXT_EVENT >= (int)BUILD_COUNT, "the next-event builds are no column of the trace table");

namespace nee_cells {
#define PT_NEE_CELL(stem, waves, Row, ...) \
  constexpr TraceCell PT_CELL_OF(stem##_nee) = {OBJ_NEE, PT_VARIANT_ID(stem), pt_nee_waves(PT_VARIANT_ID(stem), waves), #stem "_nee"};
PT_VARIANT_ROWS(PT_NEE_CELL, )
}  // namespace nee_cells

// by row, as kTraceKernels: the variant row that serves it (the LDS list walk is steered to the scalar row before a launch gets here,
// as for roulette; one build serves the rows `grid` and `grid_layers`)
#define PT_NEE_K(stem) nee_cells::cell_pt_trace_kernel##stem##_nee
constexpr TraceCell kNeeKernels[ROW_COUNT] = {
    PT_NEE_K(_scalar),   PT_NEE_K(_scalar),    PT_NEE_K(_scalar_nolds), PT_NEE_K(_small_t0), PT_NEE_K(_small_t1),
    PT_NEE_K(_small_t2), PT_NEE_K(_small_t3),  PT_NEE_K(_bvh),          PT_NEE_K(_bvh_nodes), PT_NEE_K(_bvh_gmem),
    PT_NEE_K(_grid),     PT_NEE_K(_grid_cells), PT_NEE_K(_grid_gmem),   PT_NEE_K(_grid),
};

// Does a render launch take the side table's cell?  Where the option is on and the column would have been the plain build.
inline bool takes_nee_cell(bool next_event, int build) { return next_event && build == BUILD_PLAIN; }
