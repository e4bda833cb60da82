// pt_kernels_small.hip — the small-list kernels (PT_GEOM_SMALL: lists of at most 16 spheres, the reference's own
// scene size: `uniform Sphere[15] u_sphere_list`, static/shader.frag:103), a translation unit and gfx950 code object
// of their own: a context whose scene has more than 16 spheres never loads it, one whose scene is the reference's
// never loads the walk kernels' share of a cold start twice over.
//
// No LDS in the scan, no candidate queue: the list reaches the VALU group by group from SGPRs (pt_list.hpp
// small_scan).  FOUR builds, one per list length modulo four: the last group of a list of 4 q + r spheres tests
// exactly r of them, so the padding entries are never looked at and nothing is masked — the reference's nine
// spheres (State::default; BASELINE config 4 has nine too) pay one test in their last group instead of four:
// config 4 -6.2 %, State::default 16 x 25 spp -5.6 %, its 1-spp frame -2.7 % against the build that tests the
// padding (A/B on one device, profiles/r04_ab_runs.txt).
// The four are the list PT_SMALL_KERNELS of pt_extra.h (symbol, waves per SIMD, build type), expanded here into their
// definitions and into the accessor pt_api.hip reaches them through.
#include "pt_trace_body.hpp"

PT_SMALL_KERNELS(PT_TRACE_KERNEL)

extern "C" const void* pt_small_kernel(int id) {
  switch (id) {
    PT_SMALL_KERNELS(PT_TRACE_KERNEL_CASE)
    default: return nullptr;
  }
}
