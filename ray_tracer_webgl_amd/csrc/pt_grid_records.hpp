// pt_grid_records.hpp — the DEVICE form of a grid cell record (pure: no HIP runtime, no allocation; the host, the
// kernels and the CPU tests' shim compile the same functions).
//
// The host grid (pt_grid.hpp Grid::cells, and everything that exports it) keeps `first | count << 24`.  A lane that
// walks with that record decodes it in every leaf round: split first / left, build `left >= 4 ? 15 : (1 << left) - 1`,
// rebuild the record of a second round that a cell of about three entries almost never has.  All of that depends on the
// grid alone, so the upload (pt_api.hip install_grid) does it once per cell:
//
//   bits  0..22   first : the cell's first entry
//   bits 23..31   field : count <= 4   the 4-bit VALID MASK of the cell's only round, (1 << count) - 1 (0: an empty cell)
//                         count >= 5   256 | count: "long" is the record's SIGN BIT
//
// A leaf round ANDs its candidate mask with the field and has nothing pending; lanes in a long cell (a ballot of the
// sign bit, rarely set) take every candidate of the round and compute the record of the rest — `next` below, in this
// same format, so the next round decodes it the same way.  The record is exact for every count the host format can
// express (0 .. 255); `first` loses one bit, which the host checks when it builds a grid for the device (`fits`, pt_scene_image.hpp build_grid:
// a grid of 2^23 entries or more is not walked — 128 MiB of entry copies for at most 65 528 spheres).
//
// The one-layer walk reads the same records from the ring layout at the end of this file.
//
// A kernel built to test G < 4 entries per round (PT_LEAF_GROUP_GMEM, a measuring knob) goes through `round_mask` and
// `next` in every round: the same sequence, without the short cut.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PT_REC_FN __host__ __device__ inline
#else
#define PT_REC_FN inline
#endif

namespace ptrec {

constexpr uint32_t kFirstBits = 23;
constexpr uint32_t kFirstMask = (1u << kFirstBits) - 1u;
constexpr uint32_t kNone = 1u << kFirstBits;  // rec < kNone: no entries (an empty cell, or no cell under test)
constexpr uint32_t kLong = 256u;              // in the field: more than four entries, the count in the low 8 bits
// a grid's entry array (the always-tested group included) must be shorter than this: then every `first`, and the
// `first + G` of every continuation (<= first + count), fits the field
constexpr uint32_t kEntryLimit = (1u << kFirstBits) - 8u;
PT_REC_FN bool fits(uint32_t n_entries) { return n_entries < kEntryLimit; }

PT_REC_FN uint32_t field_of(uint32_t count) { return count <= 4u ? (1u << count) - 1u : (kLong | count); }
PT_REC_FN uint32_t encode(uint32_t first, uint32_t count) { return first | (field_of(count) << kFirstBits); }
PT_REC_FN uint32_t from_host(uint32_t host_rec) { return encode(host_rec & 0xffffffu, host_rec >> 24); }

PT_REC_FN uint32_t first_of(uint32_t rec) { return rec & kFirstMask; }
PT_REC_FN bool is_long(uint32_t rec) { return (int32_t)rec < 0; }
PT_REC_FN uint32_t count_of(uint32_t rec) {
  const uint32_t f = rec >> kFirstBits;
  if (f & kLong) return f & 255u;
  return (f & 1u) + ((f >> 1) & 1u) + ((f >> 2) & 1u) + ((f >> 3) & 1u);
}
PT_REC_FN uint32_t to_host(uint32_t rec) { return first_of(rec) | (count_of(rec) << 24); }

// which of the G entries at first_of(rec) a round may accept
PT_REC_FN uint32_t round_mask(uint32_t rec, uint32_t G) {
  const uint32_t all = (1u << G) - 1u;
  return is_long(rec) ? all : ((rec >> kFirstBits) & all);
}
// what is left of the cell after a round of G entries (0: nothing)
PT_REC_FN uint32_t next(uint32_t rec, uint32_t G) {
  const uint32_t left = count_of(rec);
  return left > G ? encode(first_of(rec) + G, left - G) : 0u;
}
// G = 4, as the kernels take it: every lane ANDs its 4-bit candidate mask with the field (right for a short cell and for no
// cell; a long cell's lanes replace it by `cand`) ...
PT_REC_FN uint32_t short_mask4(uint32_t rec, uint32_t cand) { return cand & (rec >> kFirstBits); }
// ... and a LONG record's rest, as the kernels' rare branch computes it (left >= 5: something is always left)
PT_REC_FN uint32_t next_long4(uint32_t rec) { return encode(first_of(rec) + 4u, ((rec >> kFirstBits) & 255u) - 4u); }

// ---- the ring layout of a ONE-LAYER grid (n[1] == 1: the two-axis walk of pt_grid_walk.hpp) -------------------------------
// The nx x nz records lie inside a border of "outside" records, (nx + 2) x (nz + 2) in all, x fastest: a walk that steps
// out of the grid sideways lands on the border, reads kOutside and ends — it needs no step counters.  kOutside is 0: no
// entries, nothing pending, and a lane that keeps it as its stale record reads the entry array's first four entries like any
// idle lane.  So that no REAL cell reads as outside, an empty real cell whose record would be 0 (first == 0: the empty cells
// in front of the first entry) is stored with first = 1; an empty cell's `first` is never used for a test.  Index 0 is the
// border's corner: never a real cell, which is what lets the walk use `cell == 0` for "over".
constexpr uint32_t kOutside = 0u;
constexpr uint32_t kRing2 = 2u;  // records a row (and a column) gains
PT_REC_FN uint64_t ring_cells(uint32_t nx, uint32_t nz) { return (uint64_t)(nx + kRing2) * (nz + kRing2); }
PT_REC_FN uint32_t ring_index(uint32_t nx, uint32_t cx, uint32_t cz) { return (cz + 1u) * (nx + kRing2) + (cx + 1u); }
PT_REC_FN uint32_t ring_record(uint32_t host_rec) {
  const uint32_t rec = from_host(host_rec);
  return rec == kOutside ? 1u : rec;
}
// out: ring_cells(nx, nz) records, all written
inline void ring_layout(const uint32_t* host_cells, uint32_t nx, uint32_t nz, uint32_t* out) {
  const uint64_t n = ring_cells(nx, nz);
  for (uint64_t k = 0; k < n; k++) out[k] = kOutside;
  for (uint32_t cz = 0; cz < nz; cz++)
    for (uint32_t cx = 0; cx < nx; cx++) out[ring_index(nx, cx, cz)] = ring_record(host_cells[(uint64_t)cz * nx + cx]);
}

}  // namespace ptrec
