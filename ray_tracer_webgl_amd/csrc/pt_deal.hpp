// pt_deal.hpp — the wave-level dealing of work items, as pure arithmetic: which lanes of a ballot get which item of the
// wave's reserved pool, when a reservation is taken and where it starts in each queue mode, and the predicates of the
// look-ahead refill (pt_refill.hpp).  No HIP include: the trace kernels call these functions, and tests/deal_shim.cpp runs
// whole waves of them on the CPU (tests/test_deal.py).
//
// LOOK-AHEAD: every lane holds, beside the item it works on, one DECODED next item (Path::nx_*: seed, st_s, st_t,
// slab_index, item_tile; slab_index == kSlotEmpty marks the slot empty).  A lane whose item ends takes its next item at
// once (promotes()); the item decode runs only when some lane has neither (starving()), and then for every lane whose slot
// is empty (wants_item()) — so it serves most of the wave at a time instead of the lane or two that just ran out.
// A launch of few, long items per lane does not fill ahead (pt_launch_plan.hpp refill_ahead): there a held item lengthens the
// launch's drain by more than the rarer decode saves, and the slot is only the way an item reaches its lane.
// Which lane runs an item, and when, never changes a result (pt_refill.hpp, exactness argument (i)).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_DEAL_FN __host__ __device__ __forceinline__
#else
#define PT_DEAL_FN inline
#endif

namespace ptdeal {

constexpr uint32_t kSlotEmpty = 0xffffffffu;  // Path::nx_slab of an empty next slot (no slab has 2^32 - 1 pixels x passes)
enum { kQueueShared = 0, kQueueStatic = 1, kQueueGrouped = 2 };  // PtKernelArgs::queue_static

// ---- predicates (per lane; `dry` is wave-uniform: a reservation came back empty) -------------------------------------
// the lane's next slot is to be filled by the decode: every empty slot when the launch fills ahead (`ahead`, wave-uniform, the
// launch plan's decision), else only the slot of a lane without an item — the decode then serves lanes directly, at once
PT_DEAL_FN bool wants_item(bool alive, bool slot_empty, bool dry, bool ahead) { return slot_empty && !dry && (ahead || !alive); }
// the lane has neither an item nor a next one and could still get one: any such lane makes the wave run the decode
PT_DEAL_FN bool starving(bool alive, bool slot_empty, bool dry) { return !alive && slot_empty && !dry; }
// the lane's item has ended and its next one is there: it takes it at the head of the wave step
PT_DEAL_FN bool promotes(bool alive, bool slot_empty) { return !alive && !slot_empty; }

// ---- dealing from the pool [pool_next, pool_end) to the lanes of `mask` in lane order --------------------------------
PT_DEAL_FN uint32_t popcount64(unsigned long long m) { return (uint32_t)__builtin_popcountll(m); }
// a lane's rank among the lanes of `mask`: the set bits below its own (on the device one v_mbcnt pair, which knows the lane)
PT_DEAL_FN uint32_t rank_of(unsigned long long mask, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lane;
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
#else
  return popcount64(mask & ((1ull << lane) - 1ull));
#endif
}
// items the trip takes from a pool of `avail`
PT_DEAL_FN uint32_t taken(unsigned long long mask, uint32_t avail) {
  const uint32_t cnt = popcount64(mask);
  return cnt < avail ? cnt : avail;
}
// does the lane get one in this trip, and which (lanes beyond the pool's end ask again in the next trip)
PT_DEAL_FN bool gets_item(bool need, uint32_t rank, uint32_t avail) { return need && rank < avail; }
PT_DEAL_FN uint32_t item_of(uint32_t pool_base, uint32_t rank) { return pool_base + rank; }

// ---- reservations ---------------------------------------------------------------------------------------------------
// a wave reserves when its pool is used up, never before: no item of a reservation is ever left behind
PT_DEAL_FN bool pool_used_up(uint32_t pool_next, uint32_t pool_end) { return pool_next == pool_end; }
// GROUPED queue: group g owns the reservations g, g + G, g + 2 G, ...; `r` is what the group's head counter handed out
PT_DEAL_FN unsigned long long grouped_base(uint32_t r, uint32_t groups, uint32_t group, uint32_t chunk) {
  return ((unsigned long long)r * groups + group) * (unsigned long long)chunk;
}
PT_DEAL_FN uint32_t group_of(uint32_t wave, uint32_t groups) { return wave & (groups - 1u); }  // (a power of two)
// STATIC deal: wave w takes the reservations w, w + n_waves, w + 2 n_waves, ...
PT_DEAL_FN unsigned long long static_base(uint32_t round, uint32_t n_waves, uint32_t wave, uint32_t chunk) {
  return ((unsigned long long)round * n_waves + wave) * (unsigned long long)chunk;
}
// (SHARED queue: the base is the old value of the one head counter, advanced by `chunk`)
PT_DEAL_FN bool reservation_dry(unsigned long long base, uint32_t n_items) { return base >= (unsigned long long)n_items; }
PT_DEAL_FN uint32_t reservation_end(unsigned long long base, uint32_t chunk, uint32_t n_items) {
  const unsigned long long end = base + chunk;
  return end < (unsigned long long)n_items ? (uint32_t)end : n_items;
}

} // namespace ptdeal
