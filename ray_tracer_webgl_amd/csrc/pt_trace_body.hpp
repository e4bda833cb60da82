// pt_trace_body.hpp — the path-tracing kernel body shared by the nine device translation units that trace (each a gfx950
// code object of its own, loaded when one of its kernels is first asked for): pt_kernels.hip (list and walk
// kernels), pt_kernels_small.hip (the small-list kernels, one per list length modulo four),
// pt_kernels_extra.hip (the opt-in builds: the Russian-roulette kernels and the measuring twins),
// pt_kernels_debug.hip (the opt-in debug-overlay builds), pt_kernels_features.hip (the opt-in first-hit feature builds),
// pt_kernels_query.hip (the opt-in ray-query builds), pt_kernels_radiance.hip (the radiance-query builds), pt_kernels_nee.hip
// (the opt-in next-event builds) and pt_kernels_radiance_nee.hip (the radiance-query builds of the next-event estimator).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernel_args.h"
#include "pt_extra.h"
#include "pt_arith.hpp"
#include "pt_scene.hpp"
#include "pt_refill.hpp"
#include "pt_list.hpp"
#include "pt_bvh_walk.hpp"
#include "pt_grid_walk.hpp"
#include "pt_shade.hpp"

using namespace ptd;

// --------------------------------------------------------------------------------------------
// What a trace kernel is built as: a TYPE whose constants the body reads by name.  ptb::Defaults holds the defaults; a ROW type
// says how the kernel reads the sphere list (pt_scene.hpp `Scene`) and an adaptor switches one flag on top of a row:
//   SCAN_LDS, HAVE_LDS, WALK   pt_scene.hpp `Scene`
//   COUNT    the measuring twin (tallies live)
//   RR       the opt-in Russian-roulette build (pt_shade.hpp)
//   TAIL     the small-list builds' list remainder (pt_scene.hpp SMALL_TAIL)
//   FLAT_Y   the grid walk of a one-layer grid (pt_scene.hpp, pt_grid_walk.hpp)
//   DBG      the opt-in debug-overlay build (pt_shade.hpp)
//   FEAT     the opt-in first-hit feature build (pt_render_features: one pinhole ray per pixel, its hit record written to four
//            planes, no scatter; pt_refill.hpp start_sample, pt_shade.hpp)
//   QRY      the opt-in ray-query build (pt_query_rays): the feature build with the CALLER's ray, read from the query planes at the
//            lane's work item, in the pixel-centre ray's place (pt_refill.hpp start_sample); set together with FEAT (adaptor Qry)
//   RAD      the radiance-query build (pt_query_radiance): the plain build with the CALLER's ray in the camera ray's place — QRY
//            without FEAT: every sample of an item starts from the ray staged at the item's place, the seed is the item's own,
//            and the shade, the sample loop and the slab store are the plain build's (pt_refill.hpp start_sample, radiance_admit)
//   NEE      the opt-in next-event build (PT_OPT_NEXT_EVENT): the plain build with one light sample at every DIFFUSE hit whose path
//            goes on, its shadow ray walked as the lane's next segment (pt_shade.hpp, pt_nee.hpp, pt_scene.hpp NeeState)
//   RAD and NEE together (adaptor RadNee; pt_query_radiance_nee): RAD acts in the refill and the sample's start, NEE in the shade
//            and the parking, and neither reads what the other writes — but both borrow the overlay's kernel arguments, so the
//            light table moves (pt_scene.hpp nee_light_table)
// Which kernel is which row under which adaptor is stated once, in the lists of pt_extra.h.
// --------------------------------------------------------------------------------------------
namespace ptb {
struct Defaults {
  static constexpr bool SCAN_LDS = false, HAVE_LDS = false, COUNT = false, RR = false, FLAT_Y = false, DBG = false, FEAT = false, QRY = false, RAD = false, NEE = false;
  static constexpr int WALK = 0, TAIL = -1;
};
struct ListLds : Defaults { static constexpr bool SCAN_LDS = true, HAVE_LDS = true; };
struct Scalar : Defaults { static constexpr bool HAVE_LDS = true; };
struct ScalarNolds : Defaults {};
template <int T> struct Small : Defaults { static constexpr bool HAVE_LDS = true; static constexpr int WALK = 7, TAIL = T; };
struct Bvh : Defaults { static constexpr int WALK = 1; };
struct BvhNodes : Defaults { static constexpr int WALK = 2; };
struct BvhGmem : Defaults { static constexpr int WALK = 3; };
struct GridLayers : Defaults { static constexpr int WALK = 4; };
struct Grid : GridLayers { static constexpr bool FLAT_Y = true; };
struct GridCells : Defaults { static constexpr int WALK = 5; };
struct GridGmem : Defaults { static constexpr int WALK = 6; };
template <class Row> struct Count : Row { static constexpr bool COUNT = true; };
template <class Row> struct Rr : Row { static constexpr bool RR = true; };
template <class Row> struct Dbg : Row { static constexpr bool DBG = true; };
template <class Row> struct Feat : Row { static constexpr bool FEAT = true; };
template <class Row> struct Qry : Row { static constexpr bool FEAT = true, QRY = true; };
template <class Row> struct Rad : Row { static constexpr bool RAD = true; };
template <class Row> struct Nee : Row { static constexpr bool NEE = true; };
template <class Row> using RadNee = Nee<Rad<Row>>;  // both: the next-event estimator along the caller's rays (pt_kernels_radiance_nee.hip)
}  // namespace ptb

// One entry of a kernel list (pt_extra.h) as the kernel's definition and as the `case` of its object's accessor; a row of
// the variant list is built under the column's adaptor and named with its suffix.
#define PT_TRACE_KERNEL(sym, waves, Build) \
  extern "C" __global__ __launch_bounds__(1024) PT_BUILT_FOR(waves) void sym(const PtKernelArgs A) { using namespace ptb; pt_trace_body<Build>(A); }
#define PT_TRACE_KERNEL_CASE(sym, waves, Build) case PT_KERNEL_ID(sym): return reinterpret_cast<const void*>(sym);
#define PT_TRACE_VARIANT(stem, waves, Row, suffix, Adaptor) PT_TRACE_KERNEL(stem##suffix, waves, Adaptor<Row>)
#define PT_TRACE_VARIANT_CASE(stem, waves, Row, suffix, Adaptor) case PT_VARIANT_ID(stem): return reinterpret_cast<const void*>(stem##suffix);
// The accessor of an object whose ids are the variant rows: the row's build of this column by its variant id.
#define PT_VARIANT_ACCESSOR(name, suffix, Adaptor)             \
  extern "C" const void* name(int id) {                        \
    switch (id) {                                              \
      PT_VARIANT_ROWS(PT_TRACE_VARIANT_CASE, suffix, Adaptor)  \
      default: return nullptr;                                 \
    }                                                          \
  }

// The path-tracing kernel body: one persistent wave working through (pixel, pass) items.
template <class B>
__device__ __forceinline__ void pt_trace_body(const PtKernelArgs& A) {
  using namespace ptk;
  constexpr bool SCAN_LDS = B::SCAN_LDS, HAVE_LDS = B::HAVE_LDS, COUNT = B::COUNT, RR = B::RR, FLAT_Y = B::FLAT_Y, DBG = B::DBG, FEAT = B::FEAT, QRY = B::QRY, RAD = B::RAD, NEE = B::NEE;
  constexpr int WALK = B::WALK, TAIL = B::TAIL;
  using S = Scene<SCAN_LDS, HAVE_LDS, WALK, TAIL, FLAT_Y>;
  S::stage(A);

  Path p;           // per lane
  Queue q;          // wave-uniform
  Carry cw;         // walk kernels: what survives a wave step
  BvhWalk bw;
  GridWalk gw;
  Tally<COUNT> tally;
  const PixelDiv pd = pixel_div();
  uint32_t seg_count = 0; // wave-uniform tally (samples are derived on the host: pixels * spp * passes)
  tally.start();
  NeeState<NEE> ne;  // the next-event builds' shadow state (empty unless NEE)

  for (;;) {
    refill<COUNT, QRY, RAD>(A, p, q, pd, tally);
    promote<COUNT>(p, tally);
    tally.phase(0);
    // one copy of the camera-ray code per step serves both kinds of lanes: those that just
    // pulled an item and those whose previous path ended in the last step
    if (p.alive && p.new_path) {
      tally.flag(PT_REG_CAMERA_RAY);
      start_sample<FEAT, QRY, RAD>(p, pd);
      p.new_path = false;
    }
    tally.phase(1);
    const unsigned long long live = pt_ballot(p.alive);
    if (live == 0ull) break; // every lane is dead after promote(), so every next slot is empty too: the queue is dry
    tally.step();

    // ---- hit_world: static/shader.frag:175-196 -------------------------------------------------
    Hit h;
    if constexpr (S::TREE) h.closest = cw.carried ? cw.closest_w : PT_MAX_T;
    if (!cw.carried) cw.hit_pos = 0xffffffffu;
    const bool fast = regular_ray(A, p);
    const int n_live = (int)__popcll(live);
    if constexpr (S::TREE) park_store(A, p);
    if constexpr (S::TREE && NEE) park_store(A, ne);  // (the shadow ray's weight: the parking area's spare dword)
    // TAIL MODE (pt_list.hpp) is the list kernels' way out of a launch's drain: the last few rays of a wave are looked at
    // by all 64 lanes.  The walk kernels do not have it: a walk costs a wave ~1 500 issue slots whatever its lane count
    // and a turn-around n / 64 x 45 + 70 per ray, so it only ever served waves of <= 3 live rays there (config 2), while
    // its test (three ballots per step) and its code cost every step: without it config 2 -1.3 %, the hierarchy -1 %, one
    // rank's band of eight -0.9 ... -1.4 % (profiles/r04_ab_runs.txt).  Nor do the small-list kernels: a turn-around per ray
    // costs what a whole step over nine spheres costs — without it config 4 -2 %, the reference's 1-spp frame 0.132 -> 0.114 ms.
    constexpr bool kTail = !S::TREE && !S::SMALL;
    const bool coop = kTail && (n_live <= (int)A.coop_max_live) && (pt_ballot(p.alive && !fast) == 0ull) &&
                      (pt_ballot(cw.carried) == 0ull);
    if (coop) {
      tail_mode<S>(A, p, live, h);
    } else {
      h.lit_from = fast ? 0xffffffffu : 0u;
      const bool scan_lane = p.alive && fast;
      if constexpr (S::BVH) bvh_walk<S, COUNT>(A, p, scan_lane, n_live, cw, bw, h, tally);
      else if constexpr (S::GRID) grid_walk<S, COUNT>(A, p, scan_lane, n_live, cw, gw, h, tally);
      else if constexpr (S::SMALL) small_scan<S>(A, p, scan_lane, h);
      else list_scan<S>(A, p, scan_lane, h);
      tally.literal(A, p.alive && !fast, scan_lane && h.lit_from < A.n_spheres, p.slab_index);
      // a REGULAR ray the grid walk hands over whole (it starts far outside the scene and reaches the
      // grid: pt_grid_walk.hpp) is looked at by the whole wave, 64 spheres at a time, like the rays of
      // tail mode, where the list is long (the kernels whose entries do not fit the LDS: thousands of
      // spheres, 0.3 ms per ray through the literal loop; config 5: 2.3e-5 of the rays, 1.5 % of the time)
      // (not in the build whose entries are staged in the LDS — scenes of hundreds of spheres: measured in round 6, the hand-over
      // there takes a far ray of a 1 500-sphere scene from ~18 000 to ~1 500 issue slots, but its code costs config 2, which has
      // no such ray, +0.5 ... +0.8 %; those scenes are served by a grid class that keeps far rays rare instead — pt_tune measures
      // the classes, pt_refit_grid follows the camera: profiles/r06_ab_runs.txt)
      if constexpr (S::GRID && S::WALK != 4) {
        const bool handed_over = scan_lane && h.lit_from == 0u;
        const unsigned long long m_h = pt_ballot(handed_over);
        if (m_h != 0ull) {
          tail_mode<S>(A, p, m_h, h);
          if (handed_over) h.lit_from = 0xffffffffu;
        }
      }
      literal_loop<S>(A, p, h); // (irregular rays; list kernels: candidates that did not fit the queue)
    }
    if constexpr (S::TREE) {
      if (coop) cw.carried = false;
      cw.closest_w = h.closest;
      park_load(A, p);
      if constexpr (NEE) park_load(A, ne);
    }
    tally.phase(6);

    // ---- shade: static/shader.frag:304-335 (carried lanes are not there yet) --------------------
    const bool shade = p.alive && !cw.carried;
    seg_count += (uint32_t)__popcll(pt_ballot(shade));
    tally.timebin(A, shade);
    if (shade) shade_segment<S, RR, COUNT, DBG, FEAT, QRY, NEE, RAD>(A, p, h, cw, tally, ne);
    tally.collect();
    tally.phase(7);
  }

  if (lane_id() == 0) atomicAdd(&A.counters[PT_CTR_SEGMENTS], (unsigned long long)seg_count);
  tally.flush(A);
}
