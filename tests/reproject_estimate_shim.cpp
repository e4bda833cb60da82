// reproject_estimate_shim.cpp — csrc/pt_reproject.hpp's reproject_pixel_estimate (one pixel of temporal reprojection with the error
// estimate's state, the function pt_reproject_estimate_kernel runs per thread) and est_consts (what the entry point computes once)
// in front of ctypes, for tests/test_reproject_estimate_ref.py: CPU only, no HIP.  tests/reproject_estimate_main.cpp includes this
// file for its sanitizer build.  The constants of the history view, consts_of and the Raw* accessors are reproject_plan_shim.cpp's.
#include "reproject_plan_shim.cpp"

// every local pixel of a frame through reproject_pixel_estimate; `Mem` as pt_reproject.hpp asks, `Out`: put(i, acc), put_state(i, A, B)
template <class Mem, class Cur, class Out>
inline void run_frame_estimate(const ptrep::Consts& K, const ptrep::EstConsts& E, const ptrep::Frame& f, const Cur& cur, const Mem& mem,
                               Out& out) {
  for (uint32_t y = 0; y < f.rows; y++)
    for (uint32_t x = 0; x < f.width; x++) {
      const size_t i = (size_t)y * f.width + x;
      const ptrep::Carried r = ptrep::reproject_pixel_estimate(cur.ids(i), cur.pnt(i), K, E, f, mem);
      out.put(i, r.acc);
      out.put_state(i, r.A, r.B);
    }
}

namespace {
struct RawMemEstimate {
  const ptrep::I4* h_ids; const ptrep::F4* h_pnt; const ptrep::F4* accum; const ptrep::F4* err;
  ptrep::I4 hids(size_t i) const { return h_ids[i]; }
  ptrep::F4 hpnt(size_t i) const { return h_pnt[i]; }
  ptrep::F4 acc(size_t i) const { return accum[i]; }
  ptrep::F4 errA(size_t i) const { return err[2 * i]; }
  ptrep::F4 errB(size_t i) const { return err[2 * i + 1]; }
};
struct RawOutEstimate {
  ptrep::F4* o; ptrep::F4* e;
  void put(size_t i, ptrep::F4 v) { o[i] = v; }
  void put_state(size_t i, ptrep::F4 a, ptrep::F4 b) { e[2 * i] = a; e[2 * i + 1] = b; }
};
}  // namespace

// out4 = {Sf, S2, capP_diffuse, capP_other}
extern "C" void reproject_estimate_constants(int S, float cap_diffuse, float cap_other, float* out4) {
  const ptrep::EstConsts E = ptrep::est_consts(S, cap_diffuse, cap_other);
  out4[0] = E.Sf; out4[1] = E.S2; out4[2] = E.capP_diffuse; out4[3] = E.capP_other;
}

// as reproject_plan_frame, with S = the samples per pixel of the folded passes (> 0), state = 2 texels per pixel {A, B}, and two
// outputs: the accumulation's texels and the state's
extern "C" void reproject_estimate_frame(const uint32_t* frame6, const float* k16, float cap_diffuse, float cap_other, int S,
                                         const void* cur_ids, const void* cur_pnt, const void* hist_ids, const void* hist_pnt,
                                         const void* accum, const void* state, void* out, void* out_state) {
  const ptrep::Frame f = {frame6[0], frame6[1], frame6[2], frame6[3], frame6[4], frame6[5]};
  const RawCur cur = {static_cast<const ptrep::I4*>(cur_ids), static_cast<const ptrep::F4*>(cur_pnt)};
  const RawMemEstimate mem = {static_cast<const ptrep::I4*>(hist_ids), static_cast<const ptrep::F4*>(hist_pnt),
                              static_cast<const ptrep::F4*>(accum), static_cast<const ptrep::F4*>(state)};
  RawOutEstimate o = {static_cast<ptrep::F4*>(out), static_cast<ptrep::F4*>(out_state)};
  run_frame_estimate(consts_of(k16, cap_diffuse, cap_other), ptrep::est_consts(S, cap_diffuse, cap_other), f, cur, mem, o);
}
