// reproject_plan_shim.cpp — csrc/pt_reproject_plan.hpp (the host constants) and csrc/pt_reproject.hpp (one pixel of temporal
// reprojection, the header the kernel runs per thread) in front of ctypes, for tests/test_reproject_plan.py and
// tests/test_reproject_ref.py: CPU only, no HIP.  tests/reproject_main.cpp includes this file for its sanitizer build.
#include <cstddef>
#include <cstdint>

#include "../ray_tracer_webgl_amd/csrc/pt_reproject_plan.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_reproject.hpp"

// cam12 = {origin, horizontal, vertical, lower_left_corner}; 1 = constants written, 0 = refused
extern "C" int reproject_plan_constants(const float* cam12, uint32_t width, float tolerance_px, float* out16) {
  return ptrep::constants(cam12, cam12 + 3, cam12 + 6, cam12 + 9, width, tolerance_px, out16) ? 1 : 0;
}

inline ptrep::Consts consts_of(const float* k16, float cap_diffuse, float cap_other) {
  ptrep::Consts K;
  for (int c = 0; c < 3; c++) {
    K.O[c] = k16[ptrep::K_O + c];
    K.N[c] = k16[ptrep::K_N + c];
    K.A[c] = k16[ptrep::K_A + c];
    K.B[c] = k16[ptrep::K_B + c];
  }
  K.ea = k16[ptrep::K_EA];
  K.eb = k16[ptrep::K_EB];
  K.k = k16[ptrep::K_K];
  K.cap_diffuse = cap_diffuse;
  K.cap_other = cap_other;
  return K;
}

// every local pixel of a frame through reproject_pixel; `Mem` as pt_reproject.hpp asks
template <class Mem, class Cur, class Out>
inline void run_frame(const ptrep::Consts& K, const ptrep::Frame& f, const Cur& cur, const Mem& mem, Out& out) {
  for (uint32_t y = 0; y < f.rows; y++)
    for (uint32_t x = 0; x < f.width; x++) {
      const size_t i = (size_t)y * f.width + x;
      out.put(i, ptrep::reproject_pixel(cur.ids(i), cur.pnt(i), K, f, mem));
    }
}

namespace {
struct RawMem {
  const ptrep::I4* h_ids; const ptrep::F4* h_pnt; const ptrep::F4* accum;
  ptrep::I4 hids(size_t i) const { return h_ids[i]; }
  ptrep::F4 hpnt(size_t i) const { return h_pnt[i]; }
  ptrep::F4 acc(size_t i) const { return accum[i]; }
};
struct RawCur {
  const ptrep::I4* c_ids; const ptrep::F4* c_pnt;
  ptrep::I4 ids(size_t i) const { return c_ids[i]; }
  ptrep::F4 pnt(size_t i) const { return c_pnt[i]; }
};
struct RawOut {
  ptrep::F4* o;
  void put(size_t i, ptrep::F4 v) { o[i] = v; }
};
}  // namespace

// frame6 = {width, height, local rows, band_rows, band_index, band_count}; planes, accumulation and out: 16-byte aligned arrays of
// rows * width texels
extern "C" void reproject_plan_frame(const uint32_t* frame6, const float* k16, float cap_diffuse, float cap_other, const void* cur_ids,
                                     const void* cur_pnt, const void* hist_ids, const void* hist_pnt, const void* accum, void* out) {
  const ptrep::Frame f = {frame6[0], frame6[1], frame6[2], frame6[3], frame6[4], frame6[5]};
  const RawCur cur = {static_cast<const ptrep::I4*>(cur_ids), static_cast<const ptrep::F4*>(cur_pnt)};
  const RawMem mem = {static_cast<const ptrep::I4*>(hist_ids), static_cast<const ptrep::F4*>(hist_pnt), static_cast<const ptrep::F4*>(accum)};
  RawOut o = {static_cast<ptrep::F4*>(out)};
  run_frame(consts_of(k16, cap_diffuse, cap_other), f, cur, mem, o);
}
