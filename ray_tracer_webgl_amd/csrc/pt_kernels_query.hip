// pt_kernels_query.hip — the RAY-QUERY builds of the trace kernel (PT_OPT_RAY_QUERIES, pt_query_rays: the closest hit of the
// CALLER's rays, their records written to the four query planes — pt_refill.hpp QRY, pt_shade.hpp FEAT), a translation unit and
// gfx950 code object of their own: the HIP runtime loads it when the option is turned on, so a context that never asks about a
// ray pays nothing for the fourteen kernels in here.  The twelve trace kernels are the variant rows of pt_extra.h
// (PT_VARIANT_ROWS, the same launch shapes as their namesakes) under the adaptor Qry and the suffix _qry; pt_api.hip reaches
// them through pt_query_kernel() only, the accessor PT_VARIANT_ACCESSOR makes of the same rows: the column BUILD_QRY of the
// host's trace table (pt_trace_table.hpp).
// The other two move a batch between the caller's DEVICE arrays and the planes, one thread per ray, the statements of
// pt_query.hpp (for host arrays pt_api.hip runs the same statements on the host and copies plane by plane):
//   pt_query_pack_kernel     PtRay[m] -> origins into PT_FEAT_POINT's plane, directions into PT_FEAT_NORMAL's
//   pt_query_unpack_kernel   the four planes -> PtRayHit[m]
#include "pt_trace_body.hpp"
#include "pt_sigs.h"

PT_VARIANT_ROWS(PT_TRACE_VARIANT, _qry, Qry)
PT_VARIANT_ACCESSOR(pt_query_kernel, _qry, Qry)

// grid = ceil(m / 256) workgroups of 256 threads; m <= plane, the texels of one plane
extern "C" __global__ __launch_bounds__(256) void pt_query_pack_kernel(const PtRay* rays, uint32_t m, ptq::F4* planes, uint32_t plane) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m) ptq::pack_at(rays, i, planes, plane);
}

extern "C" __global__ __launch_bounds__(256) void pt_query_unpack_kernel(const ptq::F4* planes, uint32_t plane, uint32_t m, PtRayHit* hits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m) ptq::unpack_at(planes, plane, i, hits);
}

extern "C" const void* pt_query_pack_kernel_handle(void) { return ptcall::handle(ptsig::QueryPack{}, pt_query_pack_kernel); }
extern "C" const void* pt_query_unpack_kernel_handle(void) { return ptcall::handle(ptsig::QueryUnpack{}, pt_query_unpack_kernel); }
