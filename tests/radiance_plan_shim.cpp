// radiance_plan_shim.cpp — csrc/pt_radiance.hpp (the arithmetic of pt_query_radiance) as plain C functions for
// tests/test_radiance_plan.py: g++, host only, no HIP header.
#include "../ray_tracer_webgl_amd/csrc/pt_radiance.hpp"

extern "C" {

uint32_t radiance_batch_first_pass(uint32_t first_pass, uint32_t batch, uint32_t n_passes) { return ptr::batch_first_pass(first_pass, batch, n_passes); }

void radiance_zero_record(PtRayRadiance* out) { *out = ptr::zero_record(); }

// one pass texel into a record
void radiance_fold_pass(PtRayRadiance* r, const float texel[4]) {
  const ptq::F4 t = {texel[0], texel[1], texel[2], texel[3]};
  ptr::fold_pass(*r, t);
}

// m records out of n_passes slab planes and the query planes the rays were staged in, as the fold kernel does it
void radiance_fold(const float* slab, uint32_t plane, uint32_t n_passes, const float* rays, uint32_t m, PtRayRadiance* out) {
  for (uint32_t i = 0; i < m; i++)
    ptr::fold_at(reinterpret_cast<const ptq::F4*>(slab), plane, n_passes, reinterpret_cast<const ptq::F4*>(rays), i, out);
}

uint32_t radiance_sizeof_record(void) { return (uint32_t)sizeof(PtRayRadiance); }

}  // extern "C"
