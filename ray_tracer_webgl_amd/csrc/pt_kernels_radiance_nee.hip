// pt_kernels_radiance_nee.hip — the RADIANCE-QUERY builds of the NEXT-EVENT estimator (pt_query_radiance_nee, and through it
// pt_gather_irradiance_nee and pt_bake_probes_nee), a translation unit and gfx950 code object of their own: the HIP runtime
// loads it when one of those calls first needs it, so a context that never asks pays nothing for the twelve kernels in here.
// They are the variant rows of pt_extra.h (PT_VARIANT_ROWS, the same launch shapes as their namesakes) under the adaptor RadNee
// = Nee<Rad<Row>> and the suffix _rad_nee: the row's radiance build — every sample's ray read from the query planes at the item's
// place, behind PtKernelArgs::uuid, the ray count in dbg_selected (pt_refill.hpp RAD) — shading as the row's next-event build
// does (pt_shade.hpp NEE), with the light table behind PtKernelArgs::slot_uuid and its length as the bits of dbg_cursor[0]
// (pt_scene.hpp nee_light_table; pt_kernel_args.h says why there).  The caller's ray is a path's first segment: a lane starts
// an item with NeeState::sampled() false, and every path's end leaves it false.  pt_api.hip reaches the kernels through
// pt_rad_nee_kernel() only: the side table kRadNeeKernels of the host (pt_rad_nee_table.hpp).  The fold of a batch is
// pt_kernels_radiance.hip's, as it is.
#include "pt_trace_body.hpp"

// (a row's waves per SIMD: pt_extra.h pt_rad_nee_waves)
#define PT_RAD_NEE_VARIANT(stem, waves, Row, suffix, Adaptor) PT_TRACE_KERNEL(stem##suffix, pt_rad_nee_waves(PT_VARIANT_ID(stem), waves), Adaptor<Row>)
PT_VARIANT_ROWS(PT_RAD_NEE_VARIANT, _rad_nee, RadNee)
PT_VARIANT_ACCESSOR(pt_rad_nee_kernel, _rad_nee, RadNee)
