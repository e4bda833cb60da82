// pt_kernels_features.hip — the FIRST-HIT FEATURE builds of the trace kernel (PT_OPT_FEATURES, pt_render_features: one pinhole
// ray through every pixel centre, its hit record written to four planes — albedo and distance, normal, hit point, ids;
// pt_refill.hpp and pt_shade.hpp FEAT), a translation unit and gfx950 code object of their own: the HIP runtime loads it when
// one of these kernels is first asked for, so a context that never renders features pays nothing for the twelve kernels in
// here.  One build per launch that has a Russian-roulette build, with the same launch shapes as their namesakes; a one-layer
// grid is walked along three axes by pt_trace_kernel_grid_feat, as the roulette build walks it.  pt_api.hip reaches them
// through pt_feature_kernel() only.
#include "pt_trace_body.hpp"
#include "pt_extra.h"

// (the small-list kernel: one build per list length modulo four, like pt_kernels_small.hip)
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t0_feat(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 0, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t1_feat(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t2_feat(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 2, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t3_feat(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 3, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_LIST) void pt_trace_kernel_scalar_feat(const PtKernelArgs A) {
  pt_trace_body<false, true, 0, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_LIST) void pt_trace_kernel_scalar_nolds_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 0, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 1, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_nodes_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 2, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_gmem_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 3, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 4, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_cells_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 5, false, false, -1, false, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_gmem_feat(const PtKernelArgs A) {
  pt_trace_body<false, false, 6, false, false, -1, false, false, true>(A);
}

extern "C" const void* pt_feature_kernel(int id) {
  switch (id) {
    case PT_F_SMALL + 0: return reinterpret_cast<const void*>(pt_trace_kernel_small_t0_feat);
    case PT_F_SMALL + 1: return reinterpret_cast<const void*>(pt_trace_kernel_small_t1_feat);
    case PT_F_SMALL + 2: return reinterpret_cast<const void*>(pt_trace_kernel_small_t2_feat);
    case PT_F_SMALL + 3: return reinterpret_cast<const void*>(pt_trace_kernel_small_t3_feat);
    case PT_F_SCALAR: return reinterpret_cast<const void*>(pt_trace_kernel_scalar_feat);
    case PT_F_SCALAR_NOLDS: return reinterpret_cast<const void*>(pt_trace_kernel_scalar_nolds_feat);
    case PT_F_BVH: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_feat);
    case PT_F_BVH_NODES: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_nodes_feat);
    case PT_F_BVH_GMEM: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_gmem_feat);
    case PT_F_GRID: return reinterpret_cast<const void*>(pt_trace_kernel_grid_feat);
    case PT_F_GRID_CELLS: return reinterpret_cast<const void*>(pt_trace_kernel_grid_cells_feat);
    case PT_F_GRID_GMEM: return reinterpret_cast<const void*>(pt_trace_kernel_grid_gmem_feat);
    default: return nullptr;
  }
}
