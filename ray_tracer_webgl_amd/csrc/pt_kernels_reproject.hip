// pt_kernels_reproject.hip — TEMPORAL REPROJECTION (pt_set_option PT_OPT_REPROJECT, pt_reproject; include/ptrace.h, DESIGN.md
// §4.8g), a translation unit and gfx950 code object of its own: the HIP runtime loads it when the option is first turned on,
// so a context that never asks for it pays nothing.  Two kernels, neither a trace kernel:
//   pt_reproject_kernel   for every local pixel of the NEW view: project the hit point of its feature planes into the history
//                         camera, gather the accumulation at the four texels around that place where the history planes show
//                         the same surface, and write {colour * count, count} into the staging buffer
//   pt_reproject_estimate_kernel   the same, and in the same pass the error estimate's state A = {mean, n}, B = {M2, k} gathered
//                         from the same four texels (pt_reproject_estimate): the tap tests are evaluated once,
//                         an accepted tap costs two more 16-byte loads, a pixel two more 16-byte stores
// One thread per pixel in 32x8 workgroups, so a wave's gathers fall into a compact patch of the history (two rows of 32
// neighbouring pixels project to neighbouring places while the surface is the same).  Every access is one 16-byte load or store;
// there is no LDS tile: where a pixel gathers is data-dependent.  The per-pixel statements are pt_reproject.hpp's, shared with the
// host-side checks.  The three tallies are integers: counted per wave (ballot / shuffle), summed per workgroup in the LDS, then
// one atomic add per tally and workgroup — exact and independent of order.  pt_api.hip reaches the kernel through
// pt_reproject_kernel_handle() only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_reproject.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"

namespace {

struct DeviceMem {
  const ptrep::I4* h_ids;
  const ptrep::F4* h_pnt;
  const ptrep::F4* accum;
  __device__ __forceinline__ ptrep::I4 hids(size_t i) const { return h_ids[i]; }
  __device__ __forceinline__ ptrep::F4 hpnt(size_t i) const { return h_pnt[i]; }
  __device__ __forceinline__ ptrep::F4 acc(size_t i) const { return accum[i]; }
};

// A texel whose .w decides whether its .xyz are read at all: fetched as ONE vector, so that the compiler issues one
// global_load_dwordx4 and not a dword for the test and a dwordx3 behind it (two trips to memory for the same 16 bytes).
typedef float Vec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ptrep::F4 load_texel(const ptrep::F4* p) {
  const Vec4 v = *reinterpret_cast<const Vec4*>(p);
  const ptrep::F4 t = {v.x, v.y, v.z, v.w};
  return t;
}

struct DeviceMemEstimate {
  const ptrep::I4* h_ids;
  const ptrep::F4* h_pnt;
  const ptrep::F4* accum;
  const ptrep::F4* err;  // A, B interleaved: texel i at 2 i and 2 i + 1
  __device__ __forceinline__ ptrep::I4 hids(size_t i) const { return h_ids[i]; }
  __device__ __forceinline__ ptrep::F4 hpnt(size_t i) const { return h_pnt[i]; }
  __device__ __forceinline__ ptrep::F4 acc(size_t i) const { return load_texel(accum + i); }
  __device__ __forceinline__ ptrep::F4 errA(size_t i) const { return load_texel(err + 2 * i); }
  __device__ __forceinline__ ptrep::F4 errB(size_t i) const { return load_texel(err + 2 * i + 1); }
};

}  // namespace

// grid = (ceil(width / 32), ceil(rows / 8)), 256 threads.  cur_ids / cur_pnt: the current planes; hist_ids / hist_pnt: the
// history planes; accum: the accumulation as the call finds it (read only); out: rows * width texels (never accum itself);
// tally: {pixels_hit, pixels_kept, samples_kept}, zeroed by the host before the launch.
extern "C" __global__ __launch_bounds__(256) void pt_reproject_kernel(const ptrep::I4* cur_ids, const ptrep::F4* cur_pnt,
                                                                      const ptrep::I4* hist_ids, const ptrep::F4* hist_pnt,
                                                                      const ptrep::F4* accum, ptrep::F4* out, ptrep::Consts K,
                                                                      ptrep::Frame f, unsigned long long* tally) {
  __shared__ uint32_t s_tally[4][3];
  const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u), y = blockIdx.y * 8u + (threadIdx.x >> 5);
  const bool inside = x < f.width && y < f.rows;
  uint32_t hit = 0u, kept = 0u, nq = 0u;
  if (inside) {
    const size_t i = (size_t)y * f.width + (size_t)x;
    const ptrep::I4 ids = cur_ids[i];
    const ptrep::F4 Pn = cur_pnt[i];
    const DeviceMem mem = {hist_ids, hist_pnt, accum};
    const ptrep::F4 o = ptrep::reproject_pixel(ids, Pn, K, f, mem);
    out[i] = o;
    hit = ids.x >= 0 ? 1u : 0u;
    kept = o.w > 0.0f ? 1u : 0u;
    nq = kept ? (uint32_t)o.w : 0u;   // a whole number in [1, 2^24)
  }
  // per wave: the two counts from ballots, the samples through a shuffle tree (64 x 2^24 fits 32 bits)
  const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit != 0u)), n_kept = (uint32_t)__popcll(__ballot(kept != 0u));
  for (int off = 32; off >= 1; off >>= 1) nq += __shfl_down(nq, off, 64);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (lane == 0u) {
    s_tally[wave][0] = n_hit;
    s_tally[wave][1] = n_kept;
    s_tally[wave][2] = nq;
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    const unsigned long long v = (unsigned long long)s_tally[0][threadIdx.x] + s_tally[1][threadIdx.x] + s_tally[2][threadIdx.x] +
                                 s_tally[3][threadIdx.x];
    if (v) atomicAdd(&tally[threadIdx.x], v);
  }
}

// The same launch shape.  err: the estimate's state as the call finds it (read only, 2 * rows * width texels); out_err: as many
// texels of staging (never err itself: the gather reads the state at other pixels' places).  The tallies are pt_reproject's.
extern "C" __global__ __launch_bounds__(256) void pt_reproject_estimate_kernel(const ptrep::I4* cur_ids, const ptrep::F4* cur_pnt,
                                                                               const ptrep::I4* hist_ids, const ptrep::F4* hist_pnt,
                                                                               const ptrep::F4* accum, const ptrep::F4* err,
                                                                               ptrep::F4* out, ptrep::F4* out_err, ptrep::Consts K,
                                                                               ptrep::EstConsts E, ptrep::Frame f,
                                                                               unsigned long long* tally) {
  __shared__ uint32_t s_tally[4][3];
  const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u), y = blockIdx.y * 8u + (threadIdx.x >> 5);
  const bool inside = x < f.width && y < f.rows;
  uint32_t hit = 0u, kept = 0u, nq = 0u;
  if (inside) {
    const size_t i = (size_t)y * f.width + (size_t)x;
    const ptrep::I4 ids = cur_ids[i];
    const ptrep::F4 Pn = cur_pnt[i];
    const DeviceMemEstimate mem = {hist_ids, hist_pnt, accum, err};
    const ptrep::Carried o = ptrep::reproject_pixel_estimate(ids, Pn, K, E, f, mem);
    out[i] = o.acc;
    out_err[2 * i] = o.A;
    out_err[2 * i + 1] = o.B;
    hit = ids.x >= 0 ? 1u : 0u;
    kept = o.acc.w > 0.0f ? 1u : 0u;
    nq = kept ? (uint32_t)o.acc.w : 0u;
  }
  const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit != 0u)), n_kept = (uint32_t)__popcll(__ballot(kept != 0u));
  for (int off = 32; off >= 1; off >>= 1) nq += __shfl_down(nq, off, 64);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (lane == 0u) {
    s_tally[wave][0] = n_hit;
    s_tally[wave][1] = n_kept;
    s_tally[wave][2] = nq;
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    const unsigned long long v = (unsigned long long)s_tally[0][threadIdx.x] + s_tally[1][threadIdx.x] + s_tally[2][threadIdx.x] +
                                 s_tally[3][threadIdx.x];
    if (v) atomicAdd(&tally[threadIdx.x], v);
  }
}

extern "C" const void* pt_reproject_kernel_handle(void) { return ptcall::handle(ptsig::Reproject{}, pt_reproject_kernel); }
extern "C" const void* pt_reproject_estimate_kernel_handle(void) { return ptcall::handle(ptsig::ReprojectEstimate{}, pt_reproject_estimate_kernel); }
