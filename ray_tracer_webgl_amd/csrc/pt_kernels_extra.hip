// pt_kernels_extra.hip — the OPT-IN builds of the trace kernel, a translation unit (and therefore a gfx950
// code object) of their own: the Russian-roulette kernels (PT_OPT_RUSSIAN_ROULETTE, pt_shade.hpp) and the
// measuring twins (PT_OPT_COUNT_WORK: the same bodies with the executed-work tallies and the phase clock
// live).  The HIP runtime loads a code object when one of its kernels is first asked for, so a context that
// never turns these options on never pays for the seventeen kernels in here (round 3: one 557 KB code object
// with 22 instantiations of the body, loaded by every context's first launch).  Both are lists of pt_extra.h
// (PT_TWIN_KERNELS, PT_VARIANT_ROWS), expanded here; pt_api.hip reaches them through pt_extra_kernel() only.
#include "pt_trace_body.hpp"

// measuring twins (PT_OPT_COUNT_WORK): the same walks with the executed-work tallies, each the walk of the kernel it
// measures; the small-list kernel's twin is the phase clock of config 4 and State::default
PT_TWIN_KERNELS(PT_TRACE_KERNEL)

// Russian-roulette builds (PT_OPT_RUSSIAN_ROULETTE, opt-in): the variant rows under the adaptor Rr
PT_VARIANT_ROWS(PT_TRACE_VARIANT, _rr, Rr)

extern "C" const void* pt_extra_kernel(int id) {
  switch (id) {
    PT_VARIANT_ROWS(PT_TRACE_VARIANT_CASE, _rr, Rr)
    PT_TWIN_KERNELS(PT_TRACE_KERNEL_CASE)
    default: return nullptr;
  }
}
