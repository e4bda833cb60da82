// pt_extra.h — the kernels of pt_kernels_extra.hip and pt_kernels_small.hip (code objects of their own): how pt_api.hip reaches them.
#pragma once
enum {
  PT_X_BVH_COUNT = 0, PT_X_GRID_COUNT, PT_X_GRID_CELLS_COUNT, PT_X_SMALL_COUNT,
  PT_X_SMALL_RR /* + list length % 4: four builds */, PT_X_SCALAR_RR = PT_X_SMALL_RR + 4, PT_X_SCALAR_NOLDS_RR, PT_X_BVH_RR, PT_X_BVH_NODES_RR, PT_X_BVH_GMEM_RR,
  PT_X_GRID_RR, PT_X_GRID_CELLS_RR, PT_X_GRID_GMEM_RR, PT_X_GRID_LAYERS_COUNT, PT_X_COUNT
};
// the kernel's host-side handle (what hipLaunchKernel takes); asking for it loads nothing yet
extern "C" const void* pt_extra_kernel(int id);
// pt_kernels_small.hip (a code object of its own): the small-list kernel built for this list length's remainder modulo four
extern "C" const void* pt_small_kernel(unsigned n_spheres);
// pt_kernels_debug.hip (a code object of its own): the debug-overlay builds (pt_set_debug_overlay), one per launch that has a
// roulette build
enum {
  PT_D_SMALL = 0 /* + list length % 4: four builds */, PT_D_SCALAR = PT_D_SMALL + 4, PT_D_SCALAR_NOLDS, PT_D_BVH, PT_D_BVH_NODES, PT_D_BVH_GMEM,
  PT_D_GRID, PT_D_GRID_CELLS, PT_D_GRID_GMEM, PT_D_COUNT
};
extern "C" const void* pt_debug_kernel(int id);
// pt_kernels_features.hip (a code object of its own): the first-hit feature builds (pt_render_features), one per launch that has a
// roulette build
enum {
  PT_F_SMALL = 0 /* + list length % 4: four builds */, PT_F_SCALAR = PT_F_SMALL + 4, PT_F_SCALAR_NOLDS, PT_F_BVH, PT_F_BVH_NODES, PT_F_BVH_GMEM,
  PT_F_GRID, PT_F_GRID_CELLS, PT_F_GRID_GMEM, PT_F_COUNT
};
extern "C" const void* pt_feature_kernel(int id);
// pt_kernels_error.hip (a code object of its own): the error estimate's fold, read-out and tile kernels (PT_OPT_ERROR_ESTIMATE), and
// a partial round's fold and tile table (pt_render_adaptive), and the filtered read-outs (pt_resolve_filtered,
// pt_resolve_filtered_patch)
enum { PT_E_FOLD = 0, PT_E_RESOLVE, PT_E_TILES, PT_E_FOLD_TILES, PT_E_PARTITION, PT_E_FILTER, PT_E_FILTER_PATCH, PT_E_COUNT };
extern "C" const void* pt_error_kernel(int id);
// pt_kernels_reproject.hip (a code object of its own): temporal reprojection's one kernel (PT_OPT_REPROJECT, pt_reproject)
extern "C" const void* pt_reproject_kernel_handle(void);
