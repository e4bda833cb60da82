// deal_shim.cpp — whole waves of the look-ahead refill on the CPU, through the dealing arithmetic and the predicates of
// csrc/pt_deal.hpp exactly as the trace kernels call them (csrc/pt_refill.hpp refill() and promote(), csrc/pt_trace_body.hpp's
// wave step), for tests/test_deal.py.  Compiled by the tests with g++: the header has no HIP include.
//
// The model: an item is a number in [0, n_items); its length in wave steps is a hash of (number, seed) in [1, max_len], and
// `drop_percent` of the items "fall outside the image" (the edge-tile drop: decoded, never run).  A wave step is refill ->
// promote -> every live lane works one step.  Waves take their steps in turn, each skipping steps at random, so the queue's
// counters are reached in many orders.  Every wave checks the invariants as it goes; the first violation ends the run.
#include "../ray_tracer_webgl_amd/csrc/pt_deal.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_launch_plan.hpp"

#include <cstdint>
#include <vector>

namespace deal_sim {

enum { OK = 0, ERR_ITEM_RANGE = 1, ERR_SLOT_OVERWRITTEN = 2, ERR_NO_PROGRESS = 3, ERR_NO_END = 4, ERR_LEFT_WITH_WORK = 5,
       ERR_POOL_LEFT_BEHIND = 6, ERR_ARGS = 7 };

inline uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

struct Lane {
  bool alive = false;
  uint32_t left = 0;                        // wave steps the current item still takes
  uint32_t nx_slab = ptdeal::kSlotEmpty;    // the next slot: the item's number stands for its decoded fields
};

struct Wave {
  Lane lane[64];
  uint32_t pool_next = 0, pool_end = 0, round = 0;
  bool dry = false, done = false;
};

struct Sim {
  uint32_t n_items, chunk, n_waves, mode, groups, seed, max_len, drop_percent;
  bool ahead = true;
  unsigned long long head = 0;
  std::vector<unsigned long long> group_heads;
  uint32_t* decoded;
  unsigned long long decode_trips = 0, decode_lanes = 0, promotions = 0, wave_steps = 0, reservations = 0;

  uint32_t length_of(uint32_t item) const { return 1u + mix(item * 2654435761u + seed) % max_len; }
  bool dropped(uint32_t item) const { return mix(item + 0x9e3779b9u * (seed + 1u)) % 100u < drop_percent; }

  // csrc/pt_refill.hpp refill()
  int refill(Wave& w, uint32_t wave) {
    for (;;) {
      unsigned long long starving = 0, mask = 0;
      bool need[64];
      for (uint32_t l = 0; l < 64; l++) {
        const bool slot_empty = w.lane[l].nx_slab == ptdeal::kSlotEmpty;
        if (ptdeal::starving(w.lane[l].alive, slot_empty, w.dry)) starving |= 1ull << l;
        need[l] = ptdeal::wants_item(w.lane[l].alive, slot_empty, w.dry, ahead);
        if (need[l]) mask |= 1ull << l;
      }
      if (starving == 0ull) return OK;
      if (ptdeal::pool_used_up(w.pool_next, w.pool_end)) {
        reservations++;
        unsigned long long base;
        if (mode == ptdeal::kQueueGrouped) {
          const uint32_t group = ptdeal::group_of(wave, groups);
          const uint32_t r = (uint32_t)group_heads[group]++;
          base = ptdeal::grouped_base(r, groups, group, chunk);
        } else if (mode == ptdeal::kQueueStatic) {
          base = ptdeal::static_base(w.round, n_waves, wave, chunk);
          w.round++;
        } else {
          base = head;
          head += chunk;
        }
        if (ptdeal::reservation_dry(base, n_items)) {
          w.dry = true;
          for (uint32_t l = 0; l < 64; l++) need[l] = false;
        } else {
          w.pool_next = (uint32_t)base;
          w.pool_end = ptdeal::reservation_end(base, chunk, n_items);
        }
      }
      const uint32_t avail = w.pool_end - w.pool_next;
      const uint32_t pool_base = w.pool_next;
      w.pool_next += ptdeal::taken(mask, avail);
      uint32_t lanes = 0;
      for (uint32_t l = 0; l < 64; l++) {
        const uint32_t rank = ptdeal::rank_of(mask, l);
        if (!ptdeal::gets_item(need[l], rank, avail)) continue;
        const uint32_t item = ptdeal::item_of(pool_base, rank);
        if (item >= n_items) return ERR_ITEM_RANGE;
        if (w.lane[l].nx_slab != ptdeal::kSlotEmpty) return ERR_SLOT_OVERWRITTEN;
        decoded[item]++;
        lanes++;
        if (!dropped(item)) w.lane[l].nx_slab = item;
      }
      if (lanes) { decode_trips++; decode_lanes += lanes; }
    }
  }

  // one wave step; csrc/pt_trace_body.hpp
  int step(Wave& w, uint32_t wave) {
    const int e = refill(w, wave);
    if (e != OK) return e;
    for (uint32_t l = 0; l < 64; l++) {  // promote()
      Lane& L = w.lane[l];
      if (ptdeal::promotes(L.alive, L.nx_slab == ptdeal::kSlotEmpty)) {
        L.left = length_of(L.nx_slab);
        L.alive = true;
        L.nx_slab = ptdeal::kSlotEmpty;
        promotions++;
      }
    }
    bool live = false;
    for (uint32_t l = 0; l < 64; l++) {
      const Lane& L = w.lane[l];
      // a lane that holds a next item works on an item in this step: nobody sits on work
      if (L.nx_slab != ptdeal::kSlotEmpty && !L.alive) return ERR_NO_PROGRESS;
      live = live || L.alive;
    }
    if (!live) {  // the wave's exit: every lane dead, every slot empty, the queue dry, nothing reserved and not dealt
      for (uint32_t l = 0; l < 64; l++)
        if (w.lane[l].nx_slab != ptdeal::kSlotEmpty) return ERR_LEFT_WITH_WORK;
      if (!w.dry) return ERR_LEFT_WITH_WORK;
      if (w.pool_next != w.pool_end) return ERR_POOL_LEFT_BEHIND;
      w.done = true;
      return OK;
    }
    wave_steps++;
    for (uint32_t l = 0; l < 64; l++) {  // the walk and the shading of one segment: every live lane moves on
      Lane& L = w.lane[l];
      if (L.alive && --L.left == 0u) L.alive = false;
    }
    return OK;
  }
};

} // namespace deal_sim

// Runs the launch to its end.  decoded[n_items] (zeroed by the caller) counts how often each item was decoded;
// stats6 = {wave steps, decode trips, lanes served by them, promotions, reservations, rounds of turns}.  Returns 0 or the
// first violated invariant (deal_sim::ERR_*).
extern "C" __attribute__((visibility("default"))) int deal_simulate(
    uint32_t n_items, uint32_t chunk, uint32_t n_waves, uint32_t mode, uint32_t groups, uint32_t seed, uint32_t max_len,
    uint32_t drop_percent, uint32_t ahead, unsigned long long max_rounds, uint32_t* decoded, unsigned long long* stats6) {
  using namespace deal_sim;
  if (chunk == 0u || n_waves == 0u || max_len == 0u || mode > 2u) return ERR_ARGS;
  if (mode == ptdeal::kQueueGrouped && (groups == 0u || (groups & (groups - 1u)) != 0u || groups > n_waves)) return ERR_ARGS;
  Sim s;
  s.n_items = n_items; s.chunk = chunk; s.n_waves = n_waves; s.mode = mode; s.groups = groups; s.seed = seed;
  s.max_len = max_len; s.drop_percent = drop_percent; s.decoded = decoded; s.ahead = ahead != 0u;
  s.group_heads.assign(mode == ptdeal::kQueueGrouped ? groups : 0u, 0ull);
  std::vector<Wave> waves(n_waves);
  unsigned long long rounds = 0;
  uint32_t running = n_waves;
  while (running != 0u) {
    if (rounds++ >= max_rounds) return ERR_NO_END;
    for (uint32_t w = 0; w < n_waves; w++) {
      if (waves[w].done) continue;
      if (mix((uint32_t)rounds * 0x01000193u + w + seed) % 4u == 0u) continue;  // this wave is late this round
      const int e = s.step(waves[w], w);
      if (e != OK) return e;
      if (waves[w].done) running--;
    }
  }
  stats6[0] = s.wave_steps; stats6[1] = s.decode_trips; stats6[2] = s.decode_lanes; stats6[3] = s.promotions;
  stats6[4] = s.reservations; stats6[5] = rounds;
  return OK;
}

// the single functions, for the tests that pin them
extern "C" __attribute__((visibility("default"))) uint32_t deal_rank_of(unsigned long long mask, uint32_t lane) { return ptdeal::rank_of(mask, lane); }
extern "C" __attribute__((visibility("default"))) uint32_t deal_taken(unsigned long long mask, uint32_t avail) { return ptdeal::taken(mask, avail); }
extern "C" __attribute__((visibility("default"))) unsigned long long deal_grouped_base(uint32_t r, uint32_t groups, uint32_t group, uint32_t chunk) {
  return ptdeal::grouped_base(r, groups, group, chunk);
}
extern "C" __attribute__((visibility("default"))) unsigned long long deal_static_base(uint32_t round, uint32_t n_waves, uint32_t wave, uint32_t chunk) {
  return ptdeal::static_base(round, n_waves, wave, chunk);
}
extern "C" __attribute__((visibility("default"))) uint32_t deal_reservation_end(unsigned long long base, uint32_t chunk, uint32_t n_items) {
  return ptdeal::reservation_end(base, chunk, n_items);
}
extern "C" __attribute__((visibility("default"))) int deal_predicates(int alive, int slot_empty, int dry, int ahead) {
  return (ptdeal::wants_item(alive != 0, slot_empty != 0, dry != 0, ahead != 0) ? 1 : 0) | (ptdeal::starving(alive != 0, slot_empty != 0, dry != 0) ? 2 : 0) |
         (ptdeal::promotes(alive != 0, slot_empty != 0) ? 4 : 0);
}

// the launch plan's decision whether a launch fills ahead (csrc/pt_launch_plan.hpp), on the plan of the whole launch
extern "C" __attribute__((visibility("default"))) uint32_t deal_plan_refill_ahead(uint64_t items, int spp, uint32_t passes, uint32_t block, int per_cu,
                                                                               uint32_t num_cus, int walk, uint32_t n_spheres) {
  LaunchPlanIn in;
  in.items = items; in.spp = spp; in.passes = passes; in.block = block; in.per_cu = per_cu; in.num_cus = num_cus; in.walk = walk != 0;
  in.n_spheres = n_spheres;
  return plan_launch(in).refill_ahead;
}
