// pt_trace_table.hpp — every trace kernel by how it reads the list (row) and which build runs (column), and the three decisions
// a launch takes of it: its row, its column, and whether the kernel of that cell reads the grid's ring layout.  Host only: no
// runtime call, no context, plain C++, so tests/trace_table_shim.cpp can pin it.  The cells are made from the kernel lists of
// pt_extra.h: a cell's wave count is its kernel's PT_BUILT_FOR and its name is the symbol, by construction.
#pragma once
#include <cstdint>

#include "../../include/ptrace.h"
#include "pt_extra.h"
#include "pt_geom_plan.hpp"
#include "pt_kernel_args.h"

#define PT_TRACE_OBJECT_ENTRY(object, accessor, n_ids) OBJ_##object,
enum TraceObject { PT_TRACE_OBJECTS(PT_TRACE_OBJECT_ENTRY) OBJ_COUNT };

// A kernel as the host knows it: the code object that holds it and its id there (what the object's accessor takes), the waves
// per SIMD it is built for (resident_blocks caps the occupancy query with it), its symbol.
struct TraceCell {
  int object, id, waves;
  const char* name;
};

namespace trace_cells {
#define PT_CELL_OF(sym) cell_##sym
#define PT_MAIN_CELL(sym, waves, Build) constexpr TraceCell PT_CELL_OF(sym) = {OBJ_MAIN, PT_KERNEL_ID(sym), waves, #sym};
#define PT_SMALL_CELL(sym, waves, Build) constexpr TraceCell PT_CELL_OF(sym) = {OBJ_SMALL, PT_KERNEL_ID(sym), waves, #sym};
#define PT_TWIN_CELL(sym, waves, Build) constexpr TraceCell PT_CELL_OF(sym) = {OBJ_EXTRA, PT_KERNEL_ID(sym), waves, #sym};
#define PT_VARIANT_CELL(stem, waves, Row, suffix, object) \
  constexpr TraceCell PT_CELL_OF(stem##suffix) = {object, PT_VARIANT_ID(stem), waves, #stem #suffix};
PT_MAIN_KERNELS(PT_MAIN_CELL)
PT_SMALL_KERNELS(PT_SMALL_CELL)
PT_TWIN_KERNELS(PT_TWIN_CELL)
PT_VARIANT_ROWS(PT_VARIANT_CELL, _rr, OBJ_EXTRA)
PT_VARIANT_ROWS(PT_VARIANT_CELL, _dbg, OBJ_DEBUG)
PT_VARIANT_ROWS(PT_VARIANT_CELL, _feat, OBJ_FEATURE)
PT_VARIANT_ROWS(PT_VARIANT_CELL, _qry, OBJ_QUERY)
PT_VARIANT_ROWS(PT_VARIANT_CELL, _rad, OBJ_RADIANCE)
}  // namespace trace_cells

// ROW_SMALL + list length % 4; ROW_BVH + what the hierarchy stages in the LDS (hierarchy_staging's kind: 0 / 1 / 2); ROW_GRID +
// the grid's build - 1 (grid_staging's kind: 1 / 2 / 3), where ROW_GRID itself is the LDS-staged build on a grid of one layer
// along y and ROW_GRID_LAYERS the same build on any other grid (grid_walk_flat)
enum TraceRow { ROW_LIST_LDS, ROW_SCALAR, ROW_SCALAR_NOLDS, ROW_SMALL, ROW_BVH = ROW_SMALL + 4, ROW_GRID = ROW_BVH + 3, ROW_GRID_LAYERS = ROW_GRID + 3,
                ROW_COUNT };
// (the first five are the values pt_last_trace_build reports: abi.py BUILD_*; a query or radiance launch is no render launch and
// its column is never stored in c->last_build)
enum TraceBuild { BUILD_PLAIN, BUILD_RR, BUILD_TWIN, BUILD_DBG, BUILD_FEAT, BUILD_QRY, BUILD_RAD, BUILD_COUNT };

// A row: its plain kernel, its measuring twin, and the variant row (pt_extra.h) whose roulette, overlay, feature, query and
// radiance builds serve it.  Where a way to read the list has no twin, the column holds the plain build, which then runs; the
// LDS list walk has no variants either (pt_geom_plan.hpp steers roulette, overlay and door launches to the scalar row).
#define PT_K(stem) trace_cells::cell_pt_trace_kernel##stem
//                                    plain     roulette    measuring twin  debug overlay  first-hit features  ray queries  radiance queries
#define PT_TABLE_ROW(plain, twin, v) {PT_K(plain), PT_K(v##_rr), PT_K(twin), PT_K(v##_dbg), PT_K(v##_feat), PT_K(v##_qry), PT_K(v##_rad)}
constexpr TraceCell kTraceKernels[ROW_COUNT][BUILD_COUNT] = {
    {PT_K(), PT_K(), PT_K(), PT_K(), PT_K(), PT_K(), PT_K()},
    PT_TABLE_ROW(_scalar, _scalar, _scalar),
    PT_TABLE_ROW(_scalar_nolds, _scalar_nolds, _scalar_nolds),
    PT_TABLE_ROW(_small_t0, _small_count, _small_t0),
    PT_TABLE_ROW(_small_t1, _small_count, _small_t1),
    PT_TABLE_ROW(_small_t2, _small_count, _small_t2),
    PT_TABLE_ROW(_small_t3, _small_count, _small_t3),
    PT_TABLE_ROW(_bvh, _bvh_count, _bvh),
    PT_TABLE_ROW(_bvh_nodes, _bvh_nodes, _bvh_nodes),
    PT_TABLE_ROW(_bvh_gmem, _bvh_gmem, _bvh_gmem),
    PT_TABLE_ROW(_grid, _grid_count, _grid),
    PT_TABLE_ROW(_grid_cells, _grid_cells_count, _grid_cells),
    PT_TABLE_ROW(_grid_gmem, _grid_gmem, _grid_gmem),
    PT_TABLE_ROW(_grid_layers, _grid_layers_count, _grid),
};

// The row of a launch through geometry path `path` (settled: one of PT_GEOM_LDS / SCALAR / SMALL / BVH / GRID) over a list of
// n_spheres: a walk's by what it stages (Staging::kind of hierarchy_staging / grid_staging) and the grid's layers along y, a
// list kernel's by the list's length.
inline int trace_row(int path, uint32_t n_spheres, int staging_kind, uint32_t grid_layers_y) {
  if (path == PT_GEOM_BVH) return ROW_BVH + staging_kind;
  if (path == PT_GEOM_GRID) return staging_kind == 1 && !grid_walk_flat(staging_kind, grid_layers_y) ? ROW_GRID_LAYERS : ROW_GRID + staging_kind - 1;
  if (path == PT_GEOM_SMALL) return ROW_SMALL + (int)(n_spheres & 3u);
  if (path == PT_GEOM_LDS) return ROW_LIST_LDS;
  return n_spheres <= PT_MAX_SPHERES_LDS ? ROW_SCALAR : ROW_SCALAR_NOLDS;  // (the LDS copy exists whenever the list fits)
}

// The column of a render or feature launch: features before the overlay before roulette before the measuring twin.
inline int trace_build(bool features, bool overlay, bool roulette, bool count_work) {
  return features ? BUILD_FEAT : (overlay ? BUILD_DBG : (roulette ? BUILD_RR : (count_work ? BUILD_TWIN : BUILD_PLAIN)));
}

// The entry points that are no render launch, each a door to a column of its own: pt_render_features, pt_query_rays,
// pt_query_radiance.  A door launch takes a variant row's build through the path forced or settled; the overlay, roulette and
// the measuring twins do not act on it.
enum Door { DOOR_NONE, DOOR_FEATURES, DOOR_QUERY, DOOR_RADIANCE };
inline int door_build(Door door) {
  return door == DOOR_FEATURES ? BUILD_FEAT : (door == DOOR_QUERY ? BUILD_QRY : (door == DOOR_RADIANCE ? BUILD_RAD : BUILD_PLAIN));
}

// Does the kernel of this cell read the grid's ring layout?  The two-axis walk does: pt_trace_kernel_grid and its twin (the
// roulette, overlay, feature, query and radiance builds of that row walk three axes).
inline bool reads_ring_layout(int row, int build) { return row == ROW_GRID && (build == BUILD_PLAIN || build == BUILD_TWIN); }
