// pt_kernels_debug.hip — the DEBUG-OVERLAY builds of the trace kernel (pt_set_debug_overlay: the shader's cursor dot and
// selected-object outline, static/shader.frag:307-318; pt_shade.hpp DBG), a translation unit and gfx950 code object of
// their own: the HIP runtime loads it when one of these kernels is first asked for, so a context that never turns the
// overlay on pays nothing for the twelve kernels in here, and pt_kernels_extra.hip loads as fast as before.  One build
// per launch that has a Russian-roulette build, with the same launch shapes as their namesakes; a one-layer grid is
// walked along three axes by pt_trace_kernel_grid_dbg, as the roulette build walks it.  pt_api.hip reaches them through
// pt_debug_kernel() only.
#include "pt_trace_body.hpp"
#include "pt_extra.h"

// (the small-list kernel: one build per list length modulo four, like pt_kernels_small.hip)
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t0_dbg(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 0, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t1_dbg(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t2_dbg(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 2, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_SMALL) void pt_trace_kernel_small_t3_dbg(const PtKernelArgs A) {
  pt_trace_body<false, true, 7, false, false, 3, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_LIST) void pt_trace_kernel_scalar_dbg(const PtKernelArgs A) {
  pt_trace_body<false, true, 0, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_LIST) void pt_trace_kernel_scalar_nolds_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 0, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 1, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_nodes_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 2, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_bvh_gmem_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 3, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 4, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_cells_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 5, false, false, -1, false, true>(A);
}
extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(PT_WAVES_WALK) void pt_trace_kernel_grid_gmem_dbg(const PtKernelArgs A) {
  pt_trace_body<false, false, 6, false, false, -1, false, true>(A);
}

extern "C" const void* pt_debug_kernel(int id) {
  switch (id) {
    case PT_D_SMALL + 0: return reinterpret_cast<const void*>(pt_trace_kernel_small_t0_dbg);
    case PT_D_SMALL + 1: return reinterpret_cast<const void*>(pt_trace_kernel_small_t1_dbg);
    case PT_D_SMALL + 2: return reinterpret_cast<const void*>(pt_trace_kernel_small_t2_dbg);
    case PT_D_SMALL + 3: return reinterpret_cast<const void*>(pt_trace_kernel_small_t3_dbg);
    case PT_D_SCALAR: return reinterpret_cast<const void*>(pt_trace_kernel_scalar_dbg);
    case PT_D_SCALAR_NOLDS: return reinterpret_cast<const void*>(pt_trace_kernel_scalar_nolds_dbg);
    case PT_D_BVH: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_dbg);
    case PT_D_BVH_NODES: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_nodes_dbg);
    case PT_D_BVH_GMEM: return reinterpret_cast<const void*>(pt_trace_kernel_bvh_gmem_dbg);
    case PT_D_GRID: return reinterpret_cast<const void*>(pt_trace_kernel_grid_dbg);
    case PT_D_GRID_CELLS: return reinterpret_cast<const void*>(pt_trace_kernel_grid_cells_dbg);
    case PT_D_GRID_GMEM: return reinterpret_cast<const void*>(pt_trace_kernel_grid_gmem_dbg);
    default: return nullptr;
  }
}
