// pt_sigs.h — THE PARAMETER LISTS of the small kernels, stated once each: every kernel pt_api.hip launches through call()
// (pt_call.hpp has the rule), unit by unit.  The unit that defines the kernel makes its handle with
// ptcall::handle(ptsig::Name{}, kernel), which compiles only while the kernel's type is the one stated here; pt_api.hip passes
// the same ptsig::Name{} with its arguments.  The trace kernels are not here: they take one PtKernelArgs (launch_trace).
// The types a unit's own pure header defines are only declared, so that no unit reads another's header for this list; a type
// private to a unit (the probe kernels' Vec4) is named again — a second typedef of one ext_vector_type is the same type.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptrace.h"
#include "pt_call.hpp"

struct PtMatRec;
namespace ptrep { struct F4; struct I4; struct Consts; struct EstConsts; struct Frame; }
namespace pttone { struct F4; struct Window; }
namespace ptq { struct F4; }

namespace ptsig {
using ptcall::Sig;
using u32 = uint32_t;
typedef float Vec4 __attribute__((ext_vector_type(4)));

// pt_kernels_error.hip
// (accum, est, slab, n_pix, n_passes)
using FoldError = Sig<float4*, float4*, const float4*, u32, u32>;
// (accum, est, slab, order, n_active, width, rows, tiles_x, n_passes)
using FoldErrorTiles = Sig<float4*, float4*, const float4*, const u32*, u32, u32, u32, u32, u32>;
// (order, flags, part, base, n_tiles)
using PartitionOrder = Sig<const u32*, const u32*, u32*, u32*, u32>;
// (est, out, n_pix)
using ResolveError = Sig<const float4*, float4*, u32>;
// (est, tiles, aux, width, rows, tiles_x, n_tiles)
using ErrorTiles = Sig<const float4*, float4*, float4*, u32, u32, u32, u32>;
// (est, out, width, rows, band_rows, radius, kappa, gamma); the patch-wise one: patch after radius
using Filter = Sig<const float4*, float4*, u32, u32, u32, u32, float, int>;
using FilterPatch = Sig<const float4*, float4*, u32, u32, u32, u32, u32, float, int>;

// pt_kernels_reproject.hip
// (cur_ids, cur_pnt, hist_ids, hist_pnt, accum, out, K, f, tally)
using Reproject = Sig<const ptrep::I4*, const ptrep::F4*, const ptrep::I4*, const ptrep::F4*, const ptrep::F4*, ptrep::F4*, ptrep::Consts, ptrep::Frame,
                      unsigned long long*>;
// (cur_ids, cur_pnt, hist_ids, hist_pnt, accum, err, out, out_err, K, E, f, tally)
using ReprojectEstimate = Sig<const ptrep::I4*, const ptrep::F4*, const ptrep::I4*, const ptrep::F4*, const ptrep::F4*, const ptrep::F4*, ptrep::F4*,
                              ptrep::F4*, ptrep::Consts, ptrep::EstConsts, ptrep::Frame, unsigned long long*>;

// pt_kernels_display.hip
// (texels, from_accum, n_pix, width, win, tallies)
using Meter = Sig<const pttone::F4*, int, u32, u32, pttone::Window, u32*>;
// (state, options, was_valid)
using Exposure = Sig<u32*, PtMeterOptions, int>;
// (texels, from_accum, out, bytes, n_pix, curve, gamma, exposure, white, record)
using Tone = Sig<const pttone::F4*, int, void*, int, u32, int32_t, int, float, float, const PtExposure*>;

// pt_kernels_glare.hip
// (src, mode, threshold, sw, sh, dst, dw, dh)
using GlareDown = Sig<const pttone::F4*, int, float, u32, u32, pttone::F4*, u32, u32>;
// (level, w, h, weight, above, W, H)
using GlareGather = Sig<pttone::F4*, u32, u32, float, const pttone::F4*, u32, u32>;
// (src, from_accum, threshold, strength, u1, W, H, out, w, h)
using GlareComposite = Sig<const pttone::F4*, int, float, float, const pttone::F4*, u32, u32, pttone::F4*, u32, u32>;

// pt_kernels_gather.hip
// (points, item0, first, m, D, kind, planes, plane)
using GatherRays = Sig<const PtGatherPoint*, u32, u32, u32, u32, int, ptq::F4*, u32>;
// (rec, points, item0, items, first, m, D, kind, carry_in, carry_out, out, out0)
using GatherReduce = Sig<const PtRayRadiance*, const PtGatherPoint*, u32, u32, u32, u32, u32, int, const float*, float*, void*, u32>;

// pt_kernels_probe.hip
// (L, first, count, geom, mat, n_spheres, points)
using ProbePoints = Sig<PtProbeLattice, u32, u32, const float*, const PtMatRec*, u32, PtGatherPoint*>;
// (planes, plane, width, rows, L, flags, bias, cam_x, cam_y, cam_z, probes, out); the shared-cell form: paths after out
using ProbeShade = Sig<const Vec4*, u32, u32, u32, PtProbeLattice, u32, float, float, float, float, const float*, float*>;
using ProbeShadeShared = Sig<const Vec4*, u32, u32, u32, PtProbeLattice, u32, float, float, float, float, const float*, float*, u32*>;

// pt_kernels_query.hip
// (rays, m, planes, plane)
using QueryPack = Sig<const PtRay*, u32, ptq::F4*, u32>;
// (planes, plane, m, hits)
using QueryUnpack = Sig<const ptq::F4*, u32, u32, PtRayHit*>;

// pt_kernels_radiance.hip
// (slab, plane, n_passes, rays, m, out)
using RadianceFold = Sig<const ptq::F4*, u32, u32, const ptq::F4*, u32, PtRayRadiance*>;
}  // namespace ptsig
