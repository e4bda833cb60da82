// pt_kernels_radiance.hip — the RADIANCE-QUERY builds of the trace kernel (pt_query_radiance: the path-traced radiance along the
// CALLER's rays — pt_refill.hpp RAD), a translation unit and gfx950 code object of their own: the HIP runtime loads it at the
// first pt_query_radiance of a process, so a context that never asks for a ray's radiance pays nothing for the thirteen kernels
// in here.  The twelve trace kernels are the variant rows of pt_extra.h (PT_VARIANT_ROWS, the same launch shapes as their
// namesakes) under the adaptor Rad and the suffix _rad: the plain build of the row with every sample's ray read from the query
// planes (behind PtKernelArgs::uuid) at the item's place; the seed, the shade, the sample loop and the item's slab store are the
// plain build's.  pt_api.hip reaches them through pt_radiance_kernel() only, the accessor PT_VARIANT_ACCESSOR makes of the same
// rows: the column BUILD_RAD of the host's trace table (pt_trace_table.hpp).
// The thirteenth folds a batch, one thread per ray, by the statements of pt_radiance.hpp:
//   pt_radiance_fold_kernel   n_passes slab texels of place i -> PtRayRadiance out[i]; the zero record where the staged ray is invalid
#include "pt_trace_body.hpp"
#include "pt_sigs.h"
#include "pt_radiance.hpp"

PT_VARIANT_ROWS(PT_TRACE_VARIANT, _rad, Rad)
PT_VARIANT_ACCESSOR(pt_radiance_kernel, _rad, Rad)

// grid = ceil(m / 256) workgroups of 256 threads; m <= plane, the texels of one plane; out holds m records
extern "C" __global__ __launch_bounds__(256) void pt_radiance_fold_kernel(const ptq::F4* slab, uint32_t plane, uint32_t n_passes, const ptq::F4* rays,
                                                                         uint32_t m, PtRayRadiance* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m) ptr::fold_at(slab, plane, n_passes, rays, i, out);
}

extern "C" const void* pt_radiance_fold_kernel_handle(void) { return ptcall::handle(ptsig::RadianceFold{}, pt_radiance_fold_kernel); }
