// pt_radiance.hpp — the ARITHMETIC of radiance queries (include/ptrace.h pt_query_radiance), written once for
// the device and the host, beside pt_query.hpp whose batches, tile rows, validity predicate and ray staging a radiance query
// shares unchanged: which passes a batch takes, the zero record, and the fold of a place's pass texels into its record.  The
// fold kernel of pt_kernels_radiance.hip runs it per thread, pt_api.hip takes the pass offset from it,
// tests/radiance_plan_shim.cpp pins it and tests/radiance_main.cpp drives it over bounds-checked buffers under the sanitizers.
// No HIP header needed.  The only floating-point operation in here is the fold's add.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_query.hpp"

namespace ptr {

// THE PASSES OF A BATCH: batch b of a call renders the passes first_pass + b * n_passes + p, p < n_passes — passes of its own, so
// that rays at the same place of different batches share no random numbers.  32-bit, wrapping as the render calls' pass number does.
PT_QRY_HD uint32_t batch_first_pass(uint32_t first_pass, uint32_t batch, uint32_t n_passes) { return first_pass + batch * n_passes; }

// the record of an invalid ray, and of any ray before its first pass: four +0; samples == 0 is the mark
PT_QRY_HD PtRayRadiance zero_record() {
  PtRayRadiance r;
  r.sum[0] = 0.0f; r.sum[1] = 0.0f; r.sum[2] = 0.0f; r.samples = 0.0f;
  return r;
}

// THE FOLD STATEMENT: one pass texel {sum r, g, b, samples of the pass} added into the record, one IEEE add per component
PT_QRY_HD void fold_pass(PtRayRadiance& r, const ptq::F4 pass) {
  r.sum[0] = r.sum[0] + pass.x;
  r.sum[1] = r.sum[1] + pass.y;
  r.sum[2] = r.sum[2] + pass.z;
  r.samples = r.samples + pass.w;
}

// The record of place i of a batch: `slab` holds n_passes planes of `plane` texels (pass p's texel of place i at p * plane + i),
// `rays` the query planes the batch's rays were staged in (ptq::pack_at).  An item without a valid ray stored nothing and its
// slab texels are stale: validity is decided here again, from the staged ray, by the one predicate.  i < m <= plane; writes
// out[i] and nothing else.
PT_QRY_HD void fold_at(const ptq::F4* slab, uint32_t plane, uint32_t n_passes, const ptq::F4* rays, uint32_t i, PtRayRadiance* out) {
  const ptq::F4 o = rays[(size_t)PT_FEAT_POINT * plane + i], d = rays[(size_t)PT_FEAT_NORMAL * plane + i];
  PtRayRadiance r = zero_record();
  if (ptq::ray_valid(o.x, o.y, o.z, d.x, d.y, d.z))
    for (uint32_t p = 0; p < n_passes; p++) fold_pass(r, slab[(size_t)p * plane + i]);
  out[i] = r;
}

}  // namespace ptr
