// pt_launch_plan.hpp — how a trace launch is dealt to its waves, once its kernel, workgroup size and residency are
// known: the queue's reservation size, static / grouped / shared dealing, the grid, the cost feedback and the list
// kernels' tail-mode limit.  Pure integer arithmetic on numbers known before the launch (host only: no HIP, no
// context), so tests/launch_plan_shim.cpp can pin it.  Scheduling only: the images are the same bits whatever it decides.
#pragma once
#include <cstdint>
#include <optional>

#include "pt_kernel_args.h"

// The launch path's dev knobs (PT_DEV_KNOBS builds only, read by pt_api.hip's read_launch_knobs): each, when set,
// overrides one decision at the point of the arithmetic where it was always applied.
struct LaunchKnobs {
  std::optional<uint32_t> carry_lanes;    // PT_CARRY_LANES (prepare_launch)
  std::optional<uint32_t> bvh_block;      // PT_BVH_BLOCK: the walk kernels' workgroup size (walk_block_threads)
  std::optional<uint32_t> coop_max;       // PT_COOP_MAX
  std::optional<int> per_cu;              // PT_PER_CU
  std::optional<uint32_t> queue_chunk;    // PT_QUEUE_CHUNK
  std::optional<uint32_t> grid_percent;   // PT_GRID_PERCENT
  std::optional<bool> queue_static;       // PT_QUEUE_STATIC
  std::optional<bool> cost_feedback;      // PT_COST_FEEDBACK
  std::optional<int> fewer_x10_1, fewer_x10_2;  // PT_FEWER_X10_1 / _2
  std::optional<bool> queue_grouped;      // PT_QUEUE_GROUPED
};

struct LaunchPlanIn {
  uint64_t items = 0;      // work items: tiles x 64 x passes
  int spp = 1;             // samples per pixel of an item
  uint32_t passes = 1;
  uint32_t block = 256;    // workgroup size
  int per_cu = 1;          // workgroups resident on a CU (occupancy, capped by what the kernel is built for)
  uint32_t num_cus = 256;
  bool walk = false;       // a hierarchy or grid walk (no tail mode), else a list kernel
  uint32_t n_spheres = 0;  // (list kernels: the tail-mode limit)
  LaunchKnobs knobs;
};

// how the reservations reach the waves (PtKernelArgs::queue_static)
enum class Deal : uint32_t { Shared = 0, Static = 1, Grouped = 2 };

struct LaunchPlan {
  uint32_t queue_chunk = 0;
  Deal deal = Deal::Shared;
  uint32_t queue_groups = 0;  // (grouped only)
  uint32_t grid = 1;
  uint32_t n_waves = 0;
  uint32_t cost_feedback = 0;
  uint32_t coop_max_live = 0;
  uint32_t refill_ahead = 1;  // the look-ahead refill fills empty next slots ahead of need (pt_deal.hpp); 0: lanes are served directly
};

// 256-thread workgroups while several fit per CU; one 1024-thread workgroup per CU when the list takes most of the
// 160 KiB LDS (the list kernels; `lds` = the list's LDS copy)
inline uint32_t list_block_threads(uint64_t lds) { return lds > 40 * 1024 ? 1024u : 256u; }

// WHEN the refill fills ahead (round 18).  A held next item saves decodes in proportion to how often items end (1 / spp) and
// costs drain in proportion to one item's share of a lane's work (1 / items per lane): a lane that still holds an item when the
// queue runs dry ends up to an item later than its neighbours.  Measured, look-ahead against the parent's refill on one device
// (profiles/r18_ab_runs.txt): 16-spp items at 337 / 28 items per lane -5.2 % / -2.7 %, 25-spp items at 31 per lane -4.7 %,
// 1-spp frames 0; but 64-spp items at 21 (config 5) and 18 (config 4) items per lane +3.0 % and +1.6 %, the wave log showing
// the last wave 2 % later.  So items of 32 samples or more are filled ahead only where a lane gets at least spp / 2 of them.
inline uint32_t refill_ahead(uint64_t items, int spp, uint32_t n_waves) {
  const unsigned long long lanes = (unsigned long long)n_waves * 64ull;
  return (spp < 32 || 2ull * items >= (unsigned long long)spp * lanes) ? 1u : 0u;
}

inline LaunchPlan plan_queue(const LaunchPlanIn& in);
inline LaunchPlan plan_launch(const LaunchPlanIn& in) {
  LaunchPlan P = plan_queue(in);
  P.refill_ahead = refill_ahead(in.items, in.spp, P.n_waves);
  return P;
}

inline LaunchPlan plan_queue(const LaunchPlanIn& in) {
  const LaunchKnobs& k = in.knobs;
  const uint64_t items = in.items;
  const uint32_t block = in.block;
  LaunchPlan P;
  // cost feedback for the next launch's tile order: one atomicMax per item of pass 0.  A launch of one
  // SHORT pass (the reference's 1-spp frame) would report from every item — the 64 lanes of a tile on
  // one address — and stall its waves on the atomics (vmcnt completes in order): none there.
  P.cost_feedback = (in.passes >= 2u || in.spp >= 8) ? 1u : 0u;
  if (!in.walk) {
    // tail mode (list kernels only): a turn-around costs ~(n / 64 + 1) x 60 + 60 issue slots per live ray, a step of the
    // scan ~12 n + 700 for the wave: it pays while the live rays are fewer than the ratio (484 spheres: 12 — measured
    // 155.7 / 17.21 ms per 16-pass / 1-pass launch against 157.5 / 17.46 at 16 and 158.2 / 18.10 without it)
    const uint32_t per_ray = (in.n_spheres / 64u + 1u) * 60u + 60u;
    const uint32_t lim = (12u * in.n_spheres + 700u) / per_ray;
    P.coop_max_live = lim > 16u ? 16u : lim;
    if (k.coop_max) P.coop_max_live = *k.coop_max;
  }
  int per_cu = in.per_cu < 1 ? 1 : in.per_cu;
  if (k.per_cu && *k.per_cu >= 1 && *k.per_cu <= 32) per_cu = *k.per_cu;

  // Items a wave reserves per queue atomic.  Items are numbered tile-major, so a reservation is
  // also a run of neighbouring pixels: big reservations keep a wave's lanes on one tile (more
  // coherent walks, fewer atomics), small ones deal the tail of a short launch finely.
  // Measured on config 2, grid walk, 64 passes of 16 spp: the whole frame (225 items per resident
  // lane) 153.6 / 149.9 / 148.0 / 147.3 ms with 64 / 128 / 256 / 512 items; one rank's band of eight
  // (28 items per lane) 24.0 / 22.0 / 21.1 / 21.0 / 21.1 / 21.5 / 22.9 ms with 16 ... 1024.
  {
    const unsigned long long lanes = (unsigned long long)in.num_cus * (unsigned)per_cu * block;
    P.queue_chunk = items >= 192ull * lanes ? 512u : (items >= 64ull * lanes ? 128u : (items >= 16ull * lanes ? 64u : 32u));
    // ... and to the ITEMS (round 4): the queue head is one address and takes a reservation every ~13 ns (77 M/s: a 16-pass
    // launch of 1-spp items at the reference's size never ran faster than 2.9 ms through it, 0.65 ms dealt statically); an item
    // of s samples is ~s x 27 us of a lane's time, so reservations of at least 1100 / s items keep the head below half
    // of that rate
    {
      const uint32_t spp = (uint32_t)(in.spp > 0 ? in.spp : 1);
      uint32_t c_min = 32u;
      while (c_min * spp < 1100u && c_min < 1024u) c_min *= 2u;
      if (P.queue_chunk < c_min) P.queue_chunk = c_min;
    }
    if (k.queue_chunk && *k.queue_chunk >= 1u && *k.queue_chunk <= 4096u) P.queue_chunk = *k.queue_chunk;
  }
  const unsigned long long want = (items + block - 1) / block;
  const unsigned long long resident = (unsigned long long)in.num_cus * (unsigned)per_cu;
  uint32_t grid = (uint32_t)(want < resident ? want : resident);
  if (k.grid_percent) grid = (uint32_t)((unsigned long long)grid * *k.grid_percent / 100ull);
  if (grid < 1) grid = 1;
  P.grid = grid;
  // Launches of a few items per lane (the reference's 1-spp frame: two) cannot afford the shared
  // queue: its head is ONE address, the reservations' atomics take their turn there (~25 ns each), and
  // 28 000 of them are the frame's whole 0.78 ms.  Such launches deal reservations of one tile's 64
  // items round-robin to the waves instead (no atomic; the cost-ordered tile list still spreads the
  // heavy tiles over the waves).
  P.n_waves = grid * (block / 64u);
  // WHEN to deal statically: by the SAMPLES a lane gets, not only by its items.  The queue's balance is worth its atomics once
  // a lane's share is long enough for the streams' lengths to spread; below that the static deal wins, and the reservations
  // sized for the queue head (>= 1100 / spp items) would leave most waves of a short launch without any.  Measured on the
  // reference's scene and size (7 168 waves) and on the cover scene (6 144), static / queue in ms (profiles/r05_ab_runs.txt):
  //   4 spp x 4 passes  (31 samples per lane) 0.53 / 0.78      8 spp x 4  (63) 0.99 / 1.07      25 spp x 2  (98) 1.48 / 1.47
  //   25 spp x 4 (196) 2.84 / 2.62     25 spp x 8 (392) 5.48 / 4.64     cover scene 16 spp x 1 (84) 3.50 / 3.92     x 2 (169) 5.72 / 4.68
  // -> statically below 112 samples per lane (rounds 2-4: below 8 ITEMS per lane whatever their length, which dealt the
  // paused mode's 25-spp frames statically up to 200 samples per lane: 4 of them 2.84 -> 2.62 ms).  Items of one or two
  // samples keep round 4's bound of 64 items per lane (16 passes of 1 / 2 spp at the reference's size: 0.59 / 1.08 ms
  // against 2.89 / 2.89 through the queue, whose head was the limit).
  const unsigned long long lanes_all = (unsigned long long)P.n_waves * 64ull;
  const unsigned long long spp_u = (unsigned long long)(in.spp > 0 ? in.spp : 1);
  const bool short_items = in.spp <= 2 && items < 64ull * lanes_all;
  // (round 5, with the GROUPED queue below taking the statically dealt launches from 16 samples per lane on: the shared queue
  // only wins from ~450 samples per lane — grouped / shared: 25 spp x 4 (196) 2.52 / 2.61, 64 spp x 2 (250) 3.21 / 3.42, cover
  // scene 16 spp x 2 (169) 4.47 / 4.70, x 4 (337) 8.04 / 8.31, but x 8 (674) 15.25 / 14.69 and the full frame 120.8 / 110.0:
  // long launches want the shared queue's big reservations and its balance across ALL waves)
  bool dealt = short_items || items * spp_u < 448ull * lanes_all;
  if (k.queue_static) dealt = *k.queue_static;
  if (k.cost_feedback) P.cost_feedback = *k.cost_feedback ? 1u : 0u;
  if (!dealt) return P;
  P.deal = Deal::Static;
  P.queue_chunk = 64u;
  // a statically dealt launch of ONE-sample items keeps the tile order it finds: the feedback's one atomic per pixel of pass 0
  // costs such a launch more than the order gives it (4 passes of 1 spp at the reference's size: 0.206 -> 0.185 ms; with 2, 4, 8
  // spp the cost-ordered tiles pay: 0.318 / 0.557 / 1.03 ms with feedback against 0.333 / 0.608 / 1.13 without)
  if (in.spp < 2) P.cost_feedback = 0u;
  // FEWER WAVES for the shortest launches.  A launch of a lane-step or two per resident lane is all drain: a wave ends when
  // its slowest lane does, and with fewer waves on a SIMD each step is faster and each wave deals more items to its lanes.
  // One-sample items want ~4.6 per lane, two-sample items ~3.4 — in WHOLE workgroups per CU, so that no CU carries one more
  // than its neighbours (the reference's 1280x702 frame, 1 spp: three of the seven resident workgroups per CU, 0.115 ->
  // 0.081 ms; 2 spp: four, 0.132 -> 0.116; from 4 spp on the full grid wins; re-swept in round 5 on the corrected grid:
  // 3.8 / 4.2 / 4.6 / 5.0 / 5.4 items per lane -> 0.089 / 0.088 / 0.082 / 0.091 / 0.087 ms).  Scheduling only.
  if (in.spp <= 2) {
    unsigned long long x10 = in.spp == 1 ? 46ull : 34ull;
    const std::optional<int>& x10_knob = in.spp == 1 ? k.fewer_x10_1 : k.fewer_x10_2;
    if (x10_knob && *x10_knob >= 1) x10 = (unsigned long long)*x10_knob;
    const unsigned long long per_wg = (unsigned long long)block * x10 / 10ull;
    unsigned long long fewer = (items + per_wg - 1) / per_wg;
    const unsigned long long cus = (unsigned long long)in.num_cus;
    if (fewer > cus) fewer = (fewer + cus / 2) / cus * cus;  // whole workgroups per CU
    if (fewer >= 1 && fewer < grid) {
      P.grid = (uint32_t)fewer;
      P.n_waves = P.grid * (block / 64u);
    }
  }

  // ... and between the two lies the GROUPED queue (round 5; pt_refill.hpp): G groups of waves, each with a head of its own,
  // wave w in group w % G, group g owning the reservations g, g + G, ... — a queue's balance among a group's ~28 waves at one
  // atomic per reservation on one of G = 256 addresses.  It replaces the static deal from 16 SAMPLES per lane on: below that
  // a wave takes so few reservations that the atomic's round trip, which finds the whole wave idle (all lanes of a
  // short-item launch run dry together), costs more than the balance gives.  Measured static / grouped, ms
  // (profiles/r05_ab_runs.txt): the reference's scene 16 x 1 spp 0.579 / 0.533, groups of 1- / 2-spp frames 0.0384 / 0.0351 and
  // 0.0697 / 0.0598 per frame, 8 spp x 4 0.958 / 0.889, cover scene 16 x 1 spp 2.93 / 2.55, 4 spp x 2 1.62 / 1.41; but 4 x 1 spp
  // 0.164 / 0.203, the single 1-spp frame 0.079 / 0.088, the single 4-spp frame 0.172 / 0.186.  G is the largest power of
  // two that is neither above the CU count nor above the launch's wave count (every group needs a wave: nobody else hands
  // out its reservations).
  const unsigned long long lanes_now = (unsigned long long)P.n_waves * 64ull;
  bool grouped = items * spp_u >= 16ull * lanes_now;
  if (k.queue_grouped) grouped = *k.queue_grouped;
  if (grouped) {
    uint32_t g = 1u;
    while (2u * g <= in.num_cus && 2u * g <= (uint32_t)PT_QUEUE_GROUPS_MAX && 2u * g <= P.n_waves) g *= 2u;
    P.queue_groups = g;
    P.deal = Deal::Grouped;
  }
  return P;
}
