// pt_kernels_features.hip — the FIRST-HIT FEATURE builds of the trace kernel (PT_OPT_FEATURES, pt_render_features: one pinhole
// ray through every pixel centre, its hit record written to four planes — albedo and distance, normal, hit point, ids;
// pt_refill.hpp and pt_shade.hpp FEAT), a translation unit and gfx950 code object of their own: the HIP runtime loads it when
// one of these kernels is first asked for, so a context that never renders features pays nothing for the twelve kernels in
// here.  They are the variant rows of pt_extra.h (PT_VARIANT_ROWS: one per launch that has a Russian-roulette build, with the
// same launch shapes as their namesakes) under the adaptor Feat and the suffix _feat; pt_api.hip reaches them through
// pt_feature_kernel() only, the accessor PT_VARIANT_ACCESSOR makes of the same rows.  (How to add such a column: pt_extra.h.)
#include "pt_trace_body.hpp"

PT_VARIANT_ROWS(PT_TRACE_VARIANT, _feat, Feat)
PT_VARIANT_ACCESSOR(pt_feature_kernel, _feat, Feat)
