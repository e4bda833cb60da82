// pt_extra.h — THE LIST of the trace kernel's builds, and how pt_api.hip reaches the kernels of every code object.
//
// Each of the 79 trace kernels is stated once, below: its symbol, the waves per SIMD it is built for (PT_BUILT_FOR,
// pt_kernel_args.h) and its build type (pt_trace_body.hpp).  From an entry come the kernel's definition and the `case` of its
// object's accessor (pt_trace_body.hpp PT_TRACE_KERNEL...), its id, and its cell of the host's table with the same wave count
// and the symbol as a string (pt_trace_table.hpp).  Plain preprocessor and enums: the seven device units that trace and the
// host-only table header read the same text.  A list's order is the order of the definitions in its translation unit.
//
// HOW TO ADD A COLUMN of builds (one more flag on every variant row): the flag and its adaptor in pt_trace_body.hpp; a new
// pt_kernels_<name>.hip that is its header comment, PT_VARIANT_ROWS(PT_TRACE_VARIANT, _<suffix>, <Adaptor>) and
// PT_VARIANT_ACCESSOR(pt_<name>_kernel, _<suffix>, <Adaptor>), added to the Makefile's SRCS; one entry in PT_TRACE_OBJECTS
// here; and in pt_trace_table.hpp one value of TraceBuild, one cell expansion, one suffix in PT_TABLE_ROW and who names the
// column: the option's place in trace_build() for a render launch's, a Door and its line in door_build() for an entry point's.
//
// HOW TO ADD A SMALL KERNEL (any kernel that is no trace kernel and lives outside pt_kernels.hip): its accessor or its id below,
// beside its unit's; its parameter list, once, in pt_sigs.h; in its unit the handle through ptcall::handle(ptsig::Name{}, kernel),
// which compiles only while the two agree; in pt_api.hip the launch through call(ptsig::Name{}, handle, ...), which checks the
// arguments against the same list (pt_call.hpp has the rule).
#pragma once

// pt_kernels.hip (compiled into pt_api.hip's object): the list and walk kernels
#define PT_MAIN_KERNELS(X)                                          \
  X(pt_trace_kernel,              PT_WAVES_LIST_LDS, ListLds)       \
  X(pt_trace_kernel_scalar,       PT_WAVES_LIST,     Scalar)        \
  X(pt_trace_kernel_scalar_nolds, PT_WAVES_LIST,     ScalarNolds)   \
  X(pt_trace_kernel_bvh,          PT_WAVES_WALK,     Bvh)           \
  X(pt_trace_kernel_bvh_nodes,    PT_WAVES_WALK,     BvhNodes)      \
  X(pt_trace_kernel_bvh_gmem,     PT_WAVES_WALK,     BvhGmem)       \
  X(pt_trace_kernel_grid,         PT_WAVES_WALK,     Grid)          \
  X(pt_trace_kernel_grid_layers,  PT_WAVES_WALK,     GridLayers)    \
  X(pt_trace_kernel_grid_cells,   PT_WAVES_WALK,     GridCells)     \
  X(pt_trace_kernel_grid_gmem,    PT_WAVES_WALK,     GridGmem)

// pt_kernels_small.hip: the small-list kernels, one per list length modulo four
#define PT_SMALL_KERNELS(X)                                  \
  X(pt_trace_kernel_small_t0, PT_WAVES_SMALL, Small<0>)      \
  X(pt_trace_kernel_small_t1, PT_WAVES_SMALL, Small<1>)      \
  X(pt_trace_kernel_small_t2, PT_WAVES_SMALL, Small<2>)      \
  X(pt_trace_kernel_small_t3, PT_WAVES_SMALL, Small<3>)

// pt_kernels_extra.hip: the measuring twins (PT_OPT_COUNT_WORK); the small-list twin tests the padding (no TAIL)
#define PT_TWIN_KERNELS(X)                                                          \
  X(pt_trace_kernel_bvh_count,         PT_WAVES_WALK,       Count<Bvh>)             \
  X(pt_trace_kernel_grid_count,        PT_WAVES_WALK,       Count<Grid>)            \
  X(pt_trace_kernel_grid_layers_count, PT_WAVES_WALK,       Count<GridLayers>)      \
  X(pt_trace_kernel_grid_cells_count,  PT_WAVES_TWIN_CELLS, Count<GridCells>)       \
  X(pt_trace_kernel_small_count,       PT_WAVES_SMALL,      Count<Small<-1>>)

// The VARIANT ROWS: the twelve ways to read the list that have a Russian-roulette build (pt_kernels_extra.hip, suffix _rr), a
// debug-overlay build (pt_kernels_debug.hip, _dbg), a first-hit feature build (pt_kernels_features.hip, _feat), a ray-query
// build (pt_kernels_query.hip, _qry) and a radiance-query build (pt_kernels_radiance.hip, _rad), each the row's build under one
// adaptor with the same launch shape as its namesake.  The LDS list walk has none (pt_geom_plan.hpp steers those launches to the
// scalar row), and a one-layer grid is walked along three axes by the ..._grid_<suffix> build — right on any grid, and not
// measured: one build each serves the rows `grid` and `grid_layers`.
// X(stem, waves, row type, what the expansion passes on: suffix, adaptor)
#define PT_VARIANT_ROWS(X, ...)                                                \
  X(pt_trace_kernel_small_t0,     PT_WAVES_SMALL, Small<0>,    __VA_ARGS__)    \
  X(pt_trace_kernel_small_t1,     PT_WAVES_SMALL, Small<1>,    __VA_ARGS__)    \
  X(pt_trace_kernel_small_t2,     PT_WAVES_SMALL, Small<2>,    __VA_ARGS__)    \
  X(pt_trace_kernel_small_t3,     PT_WAVES_SMALL, Small<3>,    __VA_ARGS__)    \
  X(pt_trace_kernel_scalar,       PT_WAVES_LIST,  Scalar,      __VA_ARGS__)    \
  X(pt_trace_kernel_scalar_nolds, PT_WAVES_LIST,  ScalarNolds, __VA_ARGS__)    \
  X(pt_trace_kernel_bvh,          PT_WAVES_WALK,  Bvh,         __VA_ARGS__)    \
  X(pt_trace_kernel_bvh_nodes,    PT_WAVES_WALK,  BvhNodes,    __VA_ARGS__)    \
  X(pt_trace_kernel_bvh_gmem,     PT_WAVES_WALK,  BvhGmem,     __VA_ARGS__)    \
  X(pt_trace_kernel_grid,         PT_WAVES_WALK,  GridLayers,  __VA_ARGS__)    \
  X(pt_trace_kernel_grid_cells,   PT_WAVES_WALK,  GridCells,   __VA_ARGS__)    \
  X(pt_trace_kernel_grid_gmem,    PT_WAVES_WALK,  GridGmem,    __VA_ARGS__)

// The ids an accessor takes.  A variant's id is its row, in each of the five objects that hold variants; the twins of
// pt_kernels_extra.hip follow its roulette builds.
#define PT_KERNEL_ID(sym) PT_ID_##sym
#define PT_VARIANT_ID(stem) PT_VARIANT_##stem
#define PT_KERNEL_ID_ENTRY(sym, waves, Build) PT_KERNEL_ID(sym),
#define PT_VARIANT_ID_ENTRY(stem, waves, Row, ...) PT_VARIANT_ID(stem),
enum { PT_MAIN_KERNELS(PT_KERNEL_ID_ENTRY) PT_MAIN_COUNT };
enum { PT_SMALL_KERNELS(PT_KERNEL_ID_ENTRY) PT_SMALL_COUNT };
enum { PT_VARIANT_ROWS(PT_VARIANT_ID_ENTRY, ) PT_VARIANT_COUNT };
enum { PT_ROULETTE_LAST = PT_VARIANT_COUNT - 1, PT_TWIN_KERNELS(PT_KERNEL_ID_ENTRY) PT_EXTRA_COUNT };

// The seven code objects that hold the trace kernels (of the library's nine) and the accessor of each: the kernel's host-side
// handle (what hipLaunchKernel takes) by id, NULL for an id the object does not have.  Asking for a handle loads nothing yet; the
// HIP runtime loads a code object when one of its kernels is first used.  X(object, accessor, number of ids)
#define PT_TRACE_OBJECTS(X)                             \
  X(MAIN,     pt_main_kernel,     PT_MAIN_COUNT)        \
  X(SMALL,    pt_small_kernel,    PT_SMALL_COUNT)       \
  X(EXTRA,    pt_extra_kernel,    PT_EXTRA_COUNT)       \
  X(DEBUG,    pt_debug_kernel,    PT_VARIANT_COUNT)     \
  X(FEATURE,  pt_feature_kernel,  PT_VARIANT_COUNT)     \
  X(QUERY,    pt_query_kernel,    PT_VARIANT_COUNT)     \
  X(RADIANCE, pt_radiance_kernel, PT_VARIANT_COUNT)
#define PT_TRACE_ACCESSOR_DECL(object, accessor, n_ids) extern "C" const void* accessor(int id);
PT_TRACE_OBJECTS(PT_TRACE_ACCESSOR_DECL)

// pt_kernels_error.hip (a code object of its own): the error estimate's fold, read-out and tile kernels (PT_OPT_ERROR_ESTIMATE), and
// a partial round's fold and tile table (pt_render_adaptive), and the filtered read-outs (pt_resolve_filtered,
// pt_resolve_filtered_patch)
enum { PT_E_FOLD = 0, PT_E_RESOLVE, PT_E_TILES, PT_E_FOLD_TILES, PT_E_PARTITION, PT_E_FILTER, PT_E_FILTER_PATCH, PT_E_COUNT };
extern "C" const void* pt_error_kernel(int id);
// pt_kernels_reproject.hip (a code object of its own): temporal reprojection's kernels (PT_OPT_REPROJECT): pt_reproject's, and
// pt_reproject_estimate's, which gathers the error estimate's state in the same pass
extern "C" const void* pt_reproject_kernel_handle(void);
extern "C" const void* pt_reproject_estimate_kernel_handle(void);
// pt_kernels_display.hip (a code object of its own): exposure metering's two kernels and the toned read-out's (PT_OPT_TONEMAP)
enum { PT_D_METER = 0, PT_D_EXPOSURE, PT_D_TONE, PT_D_COUNT };
extern "C" const void* pt_display_kernel(int id);
// pt_kernels_glare.hip (a code object of its own): the glare pyramid's down, gather and composite kernels (PT_OPT_GLARE)
enum { PT_G_DOWN = 0, PT_G_GATHER, PT_G_COMPOSITE, PT_G_COUNT };
extern "C" const void* pt_glare_kernel(int id);
// pt_kernels_gather.hip (a code object of its own): the gather queries' ray generator and reduce (pt_gather_irradiance,
// pt_bake_probes)
enum { PT_GATHER_RAYS = 0, PT_GATHER_REDUCE, PT_GATHER_COUNT };
extern "C" const void* pt_gather_kernel(int id);
// pt_kernels_probe.hip (a code object of its own): the probe lattices' point generator and shading kernel (pt_bake_lattice,
// pt_shade_probes)
enum { PT_PROBE_POINTS = 0, PT_PROBE_SHADE, PT_PROBE_SHADE_SHARED, PT_PROBE_COUNT };
extern "C" const void* pt_lattice_kernel(int id);
// pt_kernels_nee.hip (a code object of its own): the next-event builds (PT_OPT_NEXT_EVENT), the twelve variant rows under the
// adaptor Nee with the suffix _nee, by variant id.  No column of the trace table: the host keeps them in the side table
// kNeeKernels (pt_nee_table.hpp) and takes a cell of it where a render launch's column would have been the plain build.
// Waves per SIMD a row's _nee build is built for: its namesake's figure, except where the four registers of shadow state that cross
// a walk (pt_scene.hpp NeeState) do not fit beside it — the nodes-only hierarchy walk and the cells-only grid walk spill at 80
// VGPRs (8 and 12 bytes of scratch per lane in the cross-compile's resource report) and are built for PT_WAVES_NEE_TIGHT, 96 VGPRs.
// One statement for the kernels' attribute and the host's side table.
#define PT_WAVES_NEE_TIGHT 5
constexpr int pt_nee_waves(int variant_id, int waves) {
  return variant_id == PT_VARIANT_ID(pt_trace_kernel_bvh_nodes) || variant_id == PT_VARIANT_ID(pt_trace_kernel_grid_cells) ? PT_WAVES_NEE_TIGHT : waves;
}
extern "C" const void* pt_nee_kernel(int id);
// pt_kernels_radiance_nee.hip (a code object of its own): the radiance-query builds of the next-event estimator
// (pt_query_radiance_nee and the two gather calls that walk through it), the twelve variant rows under the adaptor RadNee =
// Nee<Rad<Row>> with the suffix _rad_nee, by variant id.  No column of the trace table either: the side table kRadNeeKernels
// (pt_rad_nee_table.hpp), behind kNeeKernels.  Waves per SIMD a row's _rad_nee build is built for: its _nee build's figure — the
// staged ray's place rides in st_s, which is parked with the path, and the ray count is read where the item is decoded, so RAD
// adds no register that crosses a walk (the cross-compile's resource report: no scratch, no vector spill in any of the twelve;
// DESIGN.md §4.8o has the registers).  A row that stops fitting gets its own lower figure HERE: one statement for the kernels'
// attribute and the host's side table.
constexpr int pt_rad_nee_waves(int variant_id, int waves) { return pt_nee_waves(variant_id, waves); }
extern "C" const void* pt_rad_nee_kernel(int id);
// pt_kernels_query.hip, beside its ray-query builds (PT_OPT_RAY_QUERIES, pt_query_rays): the two kernels that move a batch of
// rays and records between the caller's device arrays and the query planes
extern "C" const void* pt_query_pack_kernel_handle(void);
extern "C" const void* pt_query_unpack_kernel_handle(void);
// pt_kernels_radiance.hip, beside its radiance-query builds (pt_query_radiance): the kernel that folds a batch's pass slabs into
// its records
extern "C" const void* pt_radiance_fold_kernel_handle(void);
