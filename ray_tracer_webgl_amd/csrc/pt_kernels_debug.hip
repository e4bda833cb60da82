// pt_kernels_debug.hip — the DEBUG-OVERLAY builds of the trace kernel (pt_set_debug_overlay: the shader's cursor dot and
// selected-object outline, static/shader.frag:307-318; pt_shade.hpp DBG), a translation unit and gfx950 code object of
// their own: the HIP runtime loads it when one of these kernels is first asked for, so a context that never turns the
// overlay on pays nothing for the twelve kernels in here, and pt_kernels_extra.hip loads as fast as before.  They are
// the variant rows of pt_extra.h (PT_VARIANT_ROWS: one per launch that has a Russian-roulette build, with the same launch
// shapes as their namesakes) under the adaptor Dbg and the suffix _dbg; pt_api.hip reaches them through pt_debug_kernel() only,
// the accessor PT_VARIANT_ACCESSOR makes of the same rows.  (How to add such a column: pt_extra.h.)
#include "pt_trace_body.hpp"

PT_VARIANT_ROWS(PT_TRACE_VARIANT, _dbg, Dbg)
PT_VARIANT_ACCESSOR(pt_debug_kernel, _dbg, Dbg)
