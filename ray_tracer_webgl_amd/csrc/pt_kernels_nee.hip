// pt_kernels_nee.hip — the NEXT-EVENT builds of the trace kernel (PT_OPT_NEXT_EVENT: one light sample at every DIFFUSE hit whose
// path goes on — pt_shade.hpp NEE, pt_nee.hpp), a translation unit and gfx950 code object of their own: the HIP runtime loads it
// when the option is first turned on, so a context that never asks for it pays nothing for the twelve kernels in here.  They are
// the variant rows of pt_extra.h (PT_VARIANT_ROWS, the same launch shapes as their namesakes) under the adaptor Nee and the
// suffix _nee: the plain build of the row with the shadow state of pt_scene.hpp NeeState per lane; the light table travels in
// PtKernelArgs::uuid and its length in dbg_selected (pt_kernel_args.h).  pt_api.hip reaches them through pt_nee_kernel() only,
// the accessor PT_VARIANT_ACCESSOR makes of the same rows: the side table kNeeKernels of the host (pt_nee_table.hpp), beside the
// trace table and outside its columns.
#include "pt_trace_body.hpp"

// (a row's waves per SIMD: pt_extra.h pt_nee_waves)
#define PT_NEE_VARIANT(stem, waves, Row, suffix, Adaptor) PT_TRACE_KERNEL(stem##suffix, pt_nee_waves(PT_VARIANT_ID(stem), waves), Adaptor<Row>)
PT_VARIANT_ROWS(PT_NEE_VARIANT, _nee, Nee)
PT_VARIANT_ACCESSOR(pt_nee_kernel, _nee, Nee)
