// pt_kernels_glare.hip — THE GLARE PYRAMID (pt_set_option PT_OPT_GLARE, pt_glare; include/ptrace.h), a
// translation unit and gfx950 code object of its own: the HIP runtime loads it when the option is turned on, so a context that
// never asks for it pays nothing.  Three pixel kernels, none a trace kernel:
//   pt_glare_down_kernel       D_k from D_{k-1} (or, for level 1, from the source through `bright`: D_0 is never stored).  A
//                              256-thread workgroup owns a 16x16 output tile: it stages the tile's 34x34 source footprint in the
//                              LDS (indices clamped at the load, so the passes have no edge cases), runs the x pass from the LDS
//                              into the LDS (16 columns of 34 rows) and the y pass out of it.  The x pass's result is an fp32 in
//                              the LDS as it is in pt_glare.hpp's host loop: the bits do not depend on the tiling.  Workgroups
//                              stride over the tiles of the level: the grid may be capped.
//                              LDS layout: three planes of floats (r, g, b), not float4 texels.  The x pass reads four taps at
//                              columns 2j .. 2j+3 of a row: a stride of two texels from lane to lane.  As float4 that is a 32-byte
//                              stride under ds_read_b128 — a 16-lane group spans two 256-byte bank rows: two-way conflicts that no
//                              row padding removes.  As planes it is ds_read_b32 with a two-dword stride (32 banks, 32-lane groups):
//                              lanes 0-15 (one row) take the even banks from the row's base, and with a row stride of 35 dwords
//                              (odd) lanes 16-31 (the next row) take the odd ones: conflict-free.  The y pass reads column X of rows
//                              2Y .. 2Y+3: lanes 0-15 one row, lanes 16-31 two rows further; a row stride of 24 dwords puts those
//                              48 dwords = 16 banks apart: conflict-free as well.  24 072 bytes per workgroup.
//   pt_glare_gather_kernel     U_k over D_k: the level's own texel times its weight, plus up(U_{k+1}) below the top level.
//   pt_glare_composite_kernel  per pixel of the frame: bright again (two loads fewer than storing b), up(U_1), the output texel.
// The per-texel statements are pt_glare.hpp's, shared with the host.  pt_api.hip reaches the kernels through pt_glare_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_glare.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"

namespace {

using ptglare::F4;

typedef float Vec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ F4 load_texel(const F4* p) {
  const Vec4 v = *reinterpret_cast<const Vec4*>(p);
  const F4 t = {v.x, v.y, v.z, v.w};
  return t;
}
__device__ __forceinline__ void store_texel(F4* p, const F4 t) {
  const Vec4 v = {t.x, t.y, t.z, t.w};
  *reinterpret_cast<Vec4*>(p) = v;
}

constexpr uint32_t kTile = 16u;               // output texels per tile edge
constexpr uint32_t kFoot = 2u * kTile + 2u;   // source texels per footprint edge: 34
constexpr uint32_t kStageStride = 35u;        // dwords per staged row (odd: see above)
constexpr uint32_t kMidStride = 24u;          // dwords per row of the x pass's result (2 * 24 = 16 mod 32)

}  // namespace

// grid = min(tiles of the (dw, dh) level, cap), 256 threads.  src: the (sw, sh) image below — mode 0: level k-1 of the pyramid;
// 1: linear source texels; 2: accumulation texels (1 and 2 go through `bright`) —, dst: the (dw, dh) level, never src.
extern "C" __global__ __launch_bounds__(256) void pt_glare_down_kernel(const F4* src, int mode, float threshold, uint32_t sw, uint32_t sh,
                                                                       F4* dst, uint32_t dw, uint32_t dh) {
  __shared__ float s_stage[3][kFoot * kStageStride];
  __shared__ float s_mid[3][kFoot * kMidStride];
  const uint32_t tiles_x = (dw + kTile - 1u) / kTile, tiles_y = (dh + kTile - 1u) / kTile;
  const uint32_t n_tiles = tiles_x * tiles_y;
  // (the trip count is the workgroup's: every thread reaches the barriers)
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t X0 = (tile % tiles_x) * kTile, Y0 = (tile / tiles_x) * kTile;
    // the footprint: staged column c is source column 2*X0 - 1 + c, clamped; rows alike
    for (uint32_t i = threadIdx.x; i < kFoot * kFoot; i += 256u) {
      const uint32_t r = i / kFoot, col = i % kFoot;
      const uint32_t sx = ptglare::clamp_index(2 * (int64_t)X0 - 1 + col, sw);
      const uint32_t sy = ptglare::clamp_index(2 * (int64_t)Y0 - 1 + r, sh);
      const F4 v = load_texel(src + (size_t)sy * sw + sx);
      float t[3] = {v.x, v.y, v.z};
      if (mode != 0) {  // (launch-uniform)
        float x[3];
        ptglare::bright(v, mode == 2, threshold, x, t);
      }
      for (int c = 0; c < 3; c++) s_stage[c][r * kStageStride + col] = t[c];
    }
    __syncthreads();
    // the x pass: output column j of a row reads staged columns 2j .. 2j+3
    for (uint32_t i = threadIdx.x; i < kFoot * kTile; i += 256u) {
      const uint32_t r = i / kTile, j = i % kTile;
      for (int c = 0; c < 3; c++) {
        const float* row = &s_stage[c][r * kStageStride + 2u * j];
        s_mid[c][r * kMidStride + j] = ptglare::down_tap(row[0], row[1], row[2], row[3]);
      }
    }
    __syncthreads();
    // the y pass: output row Y of a column reads rows 2Y .. 2Y+3
    const uint32_t X = threadIdx.x % kTile, Y = threadIdx.x / kTile;
    F4 out;
    {
      const float* c0 = &s_mid[0][2u * Y * kMidStride + X];
      const float* c1 = &s_mid[1][2u * Y * kMidStride + X];
      const float* c2 = &s_mid[2][2u * Y * kMidStride + X];
      out.x = ptglare::down_tap(c0[0], c0[kMidStride], c0[2u * kMidStride], c0[3u * kMidStride]);
      out.y = ptglare::down_tap(c1[0], c1[kMidStride], c1[2u * kMidStride], c1[3u * kMidStride]);
      out.z = ptglare::down_tap(c2[0], c2[kMidStride], c2[2u * kMidStride], c2[3u * kMidStride]);
      out.w = 0.0f;
    }
    if (X0 + X < dw && Y0 + Y < dh) store_texel(dst + (size_t)(Y0 + Y) * dw + (X0 + X), out);
    // (the next trip's staging writes s_stage, last read before the second barrier; its x pass writes s_mid after the trip's first
    // barrier, which every thread reaches only after this y pass)
  }
}

// grid = pixel_grid(w * h), 256 threads.  level: D_k in, U_k out, a (w, h) level; above: U_{k+1}, a (W, H) level, or NULL at the top
extern "C" __global__ __launch_bounds__(256) void pt_glare_gather_kernel(F4* level, uint32_t w, uint32_t h, float weight, const F4* above,
                                                                         uint32_t W, uint32_t H) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t X = (uint32_t)(i % w), Y = (uint32_t)(i / w);
    store_texel(level + i, ptglare::gather_at(load_texel(level + i), weight, above, W, H, X, Y));
  }
}

// grid = pixel_grid(w * h), 256 threads.  src: the (w, h) source, accumulation texels when from_accum; u1: U_1, a (W, H) level;
// out: w * h texels, never src itself (pt_api.hip writes the read-outs' staging)
extern "C" __global__ __launch_bounds__(256) void pt_glare_composite_kernel(const F4* src, int from_accum, float threshold, float strength,
                                                                            const F4* u1, uint32_t W, uint32_t H, F4* out, uint32_t w,
                                                                            uint32_t h) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t X = (uint32_t)(i % w), Y = (uint32_t)(i / w);
    store_texel(out + i, ptglare::composite_at(load_texel(src + i), from_accum != 0, threshold, strength, u1, W, H, X, Y));
  }
}

extern "C" const void* pt_glare_kernel(int id) {
  switch (id) {
    case PT_G_DOWN: return ptcall::handle(ptsig::GlareDown{}, pt_glare_down_kernel);
    case PT_G_GATHER: return ptcall::handle(ptsig::GlareGather{}, pt_glare_gather_kernel);
    case PT_G_COMPOSITE: return ptcall::handle(ptsig::GlareComposite{}, pt_glare_composite_kernel);
  }
  return nullptr;
}
