// pt_kernels_display.hip — EXPOSURE METERING AND THE TONED READ-OUT (pt_set_option PT_OPT_TONEMAP, pt_meter, pt_resolve_toned;
// include/ptrace.h), a translation unit and gfx950 code object of its own: the HIP runtime loads it when the
// option is first turned on (or at the first toned read-out with an explicit exposure), so a context that never asks for it pays
// nothing.  Three pixel kernels, none a trace kernel:
//   pt_meter_kernel      kernel 1: the luminance histogram of the local pixels inside the window.  256-thread workgroups stride the
//                        capped pixel grid; every workgroup counts into 258 words of the LDS (ds_add_u32) and adds its non-zero
//                        words to the context's tallies with one integer atomic each: exact, whatever the order.  A wave whose
//                        metered lanes all fall in one tally — a flat wall, a black frame: the atomics' worst case — adds their
//                        count with ONE LDS atomic instead of 64 to one address.
//   pt_exposure_kernel   kernel 2: one workgroup stages the 256 bins in the LDS, thread 0 runs pttone::solve over them and writes the
//                        record.  256 values: no scan tree.
//   pt_tone_kernel       exposure, curve, optional sqrt; float texels or packed bytes.  One 16-byte load per pixel, one 16-byte or
//                        4-byte store.  The curve is a launch argument, so its branch is uniform.  With `record` set the exposure
//                        and the white point are read from the device record: no host round trip after a pt_meter.
// The per-pixel statements are pt_tone.hpp's, shared with the host.  pt_api.hip reaches the kernels through pt_display_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_tone.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"

namespace {

typedef float Vec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ pttone::F4 load_texel(const pttone::F4* p) {
  const Vec4 v = *reinterpret_cast<const Vec4*>(p);
  const pttone::F4 t = {v.x, v.y, v.z, v.w};
  return t;
}

}  // namespace

// grid = pixel_grid(n_pix), 256 threads.  texels: the accumulation (from_accum != 0) or linear texels, n_pix = rows * width of them;
// tallies: pttone::kTallies words, zeroed by the host before the launch.
extern "C" __global__ __launch_bounds__(256) void pt_meter_kernel(const pttone::F4* texels, int from_accum, uint32_t n_pix, uint32_t width,
                                                                  pttone::Window win, uint32_t* tallies) {
  __shared__ uint32_t s_tally[pttone::kTallies];
  for (uint32_t t = threadIdx.x; t < pttone::kTallies; t += 256u) s_tally[t] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  // (the trip count is the workgroup's: every lane of a wave reaches the ballots below)
  for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n_pix; base += stride) {
    const uint64_t i = base + threadIdx.x;
    bool metered = false;
    uint32_t slot = 0u;
    if (i < n_pix) {
      const uint32_t px = (uint32_t)(i % width), ly = (uint32_t)(i / width);
      if (pttone::in_window(win, px, ly)) {
        float x[3];
        pttone::source_colour(load_texel(texels + i), from_accum != 0, x);
        slot = pttone::tally_of(pttone::luminance(x));
        metered = true;
      }
    }
    const unsigned long long act = __ballot(metered);
    if (act == 0ull) continue;  // (wave-uniform)
    const uint32_t first = (uint32_t)__ffsll(act) - 1u;
    const uint32_t slot0 = (uint32_t)__shfl((int)slot, (int)first, 64);
    const unsigned long long same = __ballot(metered && slot == slot0);
    const uint32_t n_act = (uint32_t)__popcll(act);
    if (same == act) {
      if (lane == first) atomicAdd(&s_tally[slot0], n_act);
    } else if (metered) {
      atomicAdd(&s_tally[slot], 1u);
    }
    if (lane == first) atomicAdd(&s_tally[pttone::kMetered], n_act);
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < pttone::kTallies; t += 256u) {
    const uint32_t v = s_tally[t];
    if (v) atomicAdd(&tallies[t], v);
  }
}

// one workgroup of 256.  state: the tallies, then the record; was_valid: the record holds an earlier metering or set
extern "C" __global__ __launch_bounds__(256) void pt_exposure_kernel(uint32_t* state, PtMeterOptions options, int was_valid) {
  __shared__ uint32_t s_hist[pttone::kBins];
  s_hist[threadIdx.x] = state[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0u) {
    PtExposure* record = reinterpret_cast<PtExposure*>(state + pttone::kTallies);
    const PtExposure prev = *record;
    const uint32_t* hist = s_hist;
    *record = pttone::solve(hist, state[pttone::kBelow], options, was_valid != 0, prev);
  }
}

// grid = pixel_grid(n_pix), 256 threads.  out: n_pix float4 (bytes == 0) or n_pix packed RGBA8 words, never `texels` itself;
// record: NULL (exposure and white are the arguments) or the device record
extern "C" __global__ __launch_bounds__(256) void pt_tone_kernel(const pttone::F4* texels, int from_accum, void* out, int bytes, uint32_t n_pix,
                                                                 int32_t curve, int gamma, float exposure, float white,
                                                                 const PtExposure* record) {
  if (record) {
    exposure = record->exposure;
    white = record->white;
  }
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    float x[3], y[3];
    pttone::source_colour(load_texel(texels + i), from_accum != 0, x);
    pttone::tone(x, curve, gamma, exposure, white, y);
    if (bytes) {
      static_cast<uint32_t*>(out)[i] = pttone::pack_rgba8(y);
    } else {
      const Vec4 o = {y[0], y[1], y[2], 1.0f};
      static_cast<Vec4*>(out)[i] = o;
    }
  }
}

extern "C" const void* pt_display_kernel(int id) {
  switch (id) {
    case PT_D_METER: return ptcall::handle(ptsig::Meter{}, pt_meter_kernel);
    case PT_D_EXPOSURE: return ptcall::handle(ptsig::Exposure{}, pt_exposure_kernel);
    case PT_D_TONE: return ptcall::handle(ptsig::Tone{}, pt_tone_kernel);
  }
  return nullptr;
}
