// pt_buffers.hpp — the device buffers a context owns, in sets: which buffers a set holds, how they are sized for the row
// partition in place, and what a failed allocation leaves.  Host-only and HIP-free: tests/buffers_shim.cpp compiles it with
// g++ against a stand-in allocator.  The includer defines the two functions below (pt_api.hip: hipMalloc / hipFree).
//
// The contract of every set: IN PLACE FOR THE ROWS IN PLACE, OR REFUSED.  fit(extent) sizes the set's buffers; in_place(extent)
// says whether every one of them is allocated for that extent.  A buffer is freed before its successor is asked for (the two
// need not fit on the device together), so a refused allocation leaves that buffer empty and the set not in place: the calls
// that would hand the set to a kernel or a copy answer PT_ERR_CAPACITY until a later fit succeeds.  fit makes no device call
// but the allocator's; it returns which buffers are FRESH — reallocated, contents undefined — and the caller (ensure_buffers in
// pt_api.hip) zeroes or fills exactly those.  Validity that belongs to a set alone ends where the set reallocates.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>

#include "../../include/ptrace.h"
#include "pt_gather.hpp"
#include "pt_glare.hpp"

namespace ptbuf {

// the device allocator, defined by the includer: 0 = done, anything else = the runtime's error code (pt_api.hip: a hipError_t).
// A refused dev_malloc must leave no error pending in the runtime: the next good launch's error check must not find it.
int dev_malloc(void** p, size_t bytes);
int dev_free(void* p);

// A device buffer and its capacity in elements; the one owner of every allocation the library makes, freed with it.
template <class T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~DevBuf() { if (p_) (void)dev_free(p_); }
  // room for exactly n elements, contents undefined: the old buffer is freed BEFORE the new one is allocated (the two need
  // not fit on the device together); on failure it holds nothing and has capacity 0
  int reserve(size_t n) {
    int e = 0;
    if (p_) e = dev_free(p_);
    p_ = nullptr;
    cap_ = 0;
    void* q = nullptr;
    if (e == 0) e = dev_malloc(&q, n * sizeof(T));
    if (e != 0) return e;
    p_ = static_cast<T*>(q);
    cap_ = n;
    return 0;
  }
  void release() { *this = DevBuf(); }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  // allocated, for exactly n elements / for at least n
  bool holds(size_t n) const { return p_ && cap_ == n; }
  bool holds_at_least(size_t n) const { return p_ && cap_ >= n; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// What the buffers are sized for: the local pixels, the work queue's 8x8 tiles over them and the reserved passes of the
// partition in place.  A band without rows is sized as one pixel and one tile: 0 counts as 1, here and nowhere else.
struct Extent {
  size_t pix, tiles, passes;
  Extent(size_t pix_, size_t tiles_, size_t passes_) : pix(pix_ ? pix_ : 1), tiles(tiles_ ? tiles_ : 1), passes(passes_ ? passes_ : 1) {}
};

// What a fit did.
struct Fit {
  int err = 0;         // the allocator's code of the allocation that was refused (0: none was)
  bool capped = false; // refused before anything was freed: the extent is beyond the kernels' 32-bit texel index
  uint32_t fresh = 0;  // the set's bit of every buffer that was reallocated and is in place: its contents are undefined
  bool ok() const { return err == 0 && !capped; }
};

// the planes of PT_FEAT_PLANES texels per pixel are indexed with 32 bits by the kernels
inline bool planes_indexable(size_t pix) { return pix <= 0x3fffffffu / PT_FEAT_PLANES; }
inline size_t plane_texels(size_t pix) { return (size_t)PT_FEAT_PLANES * pix; }

// reserve `n` elements of `buf` inside a fit: false when refused (f.err says why), else the buffer's bit is fresh
template <class T>
inline bool refit(Fit& f, DevBuf<T>& buf, size_t n, uint32_t bit) {
  if ((f.err = buf.reserve(n)) != 0) return false;
  f.fresh |= bit;
  return true;
}

// ---- the buffers every context has --------------------------------------------------------------------------------------
// the own accumulation (>= pix; `accum` names it, or the caller's bound buffer, and never freed memory), the per-pass slabs
// (>= pix * passes), the work queue's per-tile cost and order (== tiles: an order left from another count would name tiles that
// do not exist, or miss some), the reference's two RGBA8 textures and canvas (>= pix) and the read-out staging (>= pix)
template <class Texel>
struct FrameSet {
  enum : uint32_t { ACCUM = 1, SLAB = 2, COST = 4, ORDER = 8, TEX0 = 16, TEX1 = 32, CANVAS = 64, RESOLVE = 128 };
  DevBuf<Texel> own_accum;
  Texel* accum = nullptr;  // own_accum or caller-bound (never freed here)
  size_t accum_pixels = 0;
  bool accum_bound = false;
  DevBuf<Texel> slab;
  DevBuf<uint32_t> tile_cost, tile_order;
  DevBuf<uint32_t> tex[2], canvas;
  DevBuf<Texel> resolve;

  Fit fit(const Extent& e) {
    Fit f;
    if (!accum_bound) {
      if (own_accum.capacity() < e.pix) {
        accum = nullptr;  // (before the buffer it names is freed)
        accum_pixels = 0;
        if (!refit(f, own_accum, e.pix, ACCUM)) return f;
      }
      accum = own_accum.get();
      accum_pixels = own_accum.capacity();
    }
    if (slab.capacity() < e.pix * e.passes && !refit(f, slab, e.pix * e.passes, SLAB)) return f;
    if (tile_cost.capacity() != e.tiles || tile_order.capacity() != e.tiles)
      if (!refit(f, tile_cost, e.tiles, COST) || !refit(f, tile_order, e.tiles, ORDER)) return f;
    if (canvas.capacity() < e.pix)  // (the canvas last: its capacity says all three are in place)
      if (!refit(f, tex[0], e.pix, TEX0) || !refit(f, tex[1], e.pix, TEX1) || !refit(f, canvas, e.pix, CANVAS)) return f;
    if (resolve.capacity() < e.pix) refit(f, resolve, e.pix, RESOLVE);
    return f;
  }
  bool in_place(const Extent& e) const {
    return accum && (accum_bound || own_accum.holds_at_least(e.pix)) && slab.holds_at_least(e.pix * e.passes) &&
           tile_cost.holds(e.tiles) && tile_order.holds(e.tiles) && tex[0].holds_at_least(e.pix) && tex[1].holds_at_least(e.pix) &&
           canvas.holds_at_least(e.pix) && resolve.holds_at_least(e.pix);
  }
};

// ---- the opt-in sets: nothing is held while `on` is false ---------------------------------------------------------------
// PT_OPT_ERROR_ESTIMATE: the state — two texels per local pixel, A = {mean.rgb, n} and B = {M2.rgb, k} (>= 2 pix; fresh state
// holds no passes: spp restarts) —, the tile records and their tallies (>= 2 tiles), and pt_reproject_estimate's staging of the
// state (>= 2 pix), which is held only while PT_OPT_REPROJECT is on too
template <class Texel>
struct EstimateSet {
  enum : uint32_t { STATE = 1, TILES = 2, STAGE = 4 };
  bool on = false;
  bool paused = false;  // pt_tune's measuring launches fold the plain way (it clears everything afterwards)
  int spp = 0;          // samples_per_pixel of the passes folded since the last clear (0 = none yet)
  DevBuf<Texel> state, tiles, stage;

  Fit fit(const Extent& e, bool reprojecting) {
    Fit f;
    if (!on || !reprojecting) stage.release();
    if (!on) return f;
    if (state.capacity() < 2 * e.pix) {
      spp = 0;
      if (!refit(f, state, 2 * e.pix, STATE)) return f;
    }
    if (tiles.capacity() < 2 * e.tiles && !refit(f, tiles, 2 * e.tiles, TILES)) return f;
    if (reprojecting && stage.capacity() < 2 * e.pix) refit(f, stage, 2 * e.pix, STAGE);
    return f;
  }
  bool in_place(const Extent& e, bool reprojecting) const {
    return on && state.holds_at_least(2 * e.pix) && tiles.holds_at_least(2 * e.tiles) && (!reprojecting || stage.holds_at_least(2 * e.pix));
  }
  void release() {
    on = false;
    spp = 0;
    state.release(); tiles.release(); stage.release();
  }
};

// PT_OPT_FEATURES: four planes of one texel per local pixel in one allocation, plane k at k * pix — hence sized exactly
template <class Texel>
struct FeatureSet {
  enum : uint32_t { PLANES = 1 };
  bool on = false;
  bool valid = false;  // the planes speak for the scene, uniforms and partition in place (pt_read_features)
  DevBuf<Texel> planes;

  Fit fit(const Extent& e) {
    Fit f;
    if (!on || planes.capacity() == plane_texels(e.pix)) return f;
    valid = false;
    if (!planes_indexable(e.pix)) { f.capped = true; return f; }
    refit(f, planes, plane_texels(e.pix), PLANES);
    return f;
  }
  bool in_place(const Extent& e) const { return on && planes.holds(plane_texels(e.pix)); }
  void release() {
    on = valid = false;
    planes.release();
  }
};

// PT_OPT_RAY_QUERIES: the query planes — the feature planes' layout — and the identity tile order a query launch is dealt by
// (== tiles).  Both in place or neither: the planes go before the order is touched.
template <class Texel>
struct QuerySet {
  enum : uint32_t { PLANES = 1, ORDER = 2 };
  bool on = false;
  DevBuf<Texel> planes;
  DevBuf<uint32_t> order;

  bool fits(const Extent& e) const { return planes.capacity() == plane_texels(e.pix) && order.capacity() == e.tiles; }
  Fit fit(const Extent& e) {
    Fit f;
    if (!on || fits(e)) return f;
    if (!planes_indexable(e.pix)) { f.capped = true; return f; }
    planes.release();
    if (refit(f, order, e.tiles, ORDER)) refit(f, planes, plane_texels(e.pix), PLANES);
    return f;
  }
  bool in_place(const Extent& e) const { return on && planes.holds(plane_texels(e.pix)) && order.holds(e.tiles); }
  void release() {
    on = false;
    planes.release(); order.release();
  }
};

// PT_OPT_REPROJECT: the history planes — the ids plane, then the point plane at pix, of an earlier view (== 2 pix) —, the
// uniforms they were rendered with, and the last call's three tallies {pixels_hit, pixels_kept, samples_kept}
template <class Texel>
struct HistorySet {
  enum : uint32_t { PLANES = 1, TALLY = 2 };
  bool on = false;
  bool valid = false;  // the history speaks for the scene and partition in place, and no pt_reproject has used it
  bool ran = false;    // the tallies are those of a pt_reproject (pt_reproject_stats)
  PtParams params{};
  DevBuf<Texel> planes;
  DevBuf<unsigned long long> tally;

  Fit fit(const Extent& e) {
    Fit f;
    if (!on) return f;
    if (planes.capacity() != 2 * e.pix) {
      valid = false;
      if (!refit(f, planes, 2 * e.pix, PLANES)) return f;
    }
    if (tally.capacity() < 3) refit(f, tally, 3, TALLY);
    return f;
  }
  bool in_place(const Extent& e) const { return on && planes.holds(2 * e.pix) && tally.holds_at_least(3); }
  void release() {
    on = valid = ran = false;
    planes.release(); tally.release();
  }
};

// PT_OPT_TONEMAP: the metering's tallies — 256 bins, `below`, the pixels looked at — and behind them the PtExposure record, in one
// allocation of a FIXED size: the only set whose fit does not read the extent, so no resize and no repartition touches it.  The
// record is the viewer's adaptation, not a product of the scene: `valid` (metered or set since the option came on) has no row in
// the change table of pt_ctx_state.hpp and ends only where the set is released, or reallocated after a refused allocation.
struct ExposureSet {
  enum : uint32_t { STATE = 1 };
  static constexpr size_t kTallies = 258, kWords = kTallies + sizeof(PtExposure) / sizeof(uint32_t);
  bool on = false;
  bool valid = false;
  DevBuf<uint32_t> state;

  Fit fit() {
    Fit f;
    if (!on || state.holds(kWords)) return f;
    valid = false;
    refit(f, state, kWords, STATE);
    return f;
  }
  bool in_place() const { return on && state.holds(kWords); }
  void release() {
    on = valid = false;
    state.release();
  }
};

// PT_OPT_GLARE: pt_glare's pyramid — levels 1 .. PT_GLARE_MAX_LEVELS of the local frame, level k behind level k - 1, one texel per
// level texel (ptglare::pyramid_texels: about a third of the frame) — sized exactly from the width and the rows in place, so a
// resize and a repartition refit it.  It is SCRATCH: every pt_glare writes all it reads, nothing in it outlives a call, so it
// carries no validity and has no row in the change table of pt_ctx_state.hpp, and a fresh pyramid is not zeroed.  A frame without
// rows is sized as one texel (0 counts as 1, as in Extent).
template <class Texel>
struct GlareSet {
  enum : uint32_t { PYRAMID = 1 };
  bool on = false;
  DevBuf<Texel> pyramid;

  static size_t texels(uint32_t width, uint32_t rows) {
    const size_t n = ptglare::pyramid_texels(width, rows, PT_GLARE_MAX_LEVELS);
    return n ? n : 1;
  }
  Fit fit(uint32_t width, uint32_t rows) {
    Fit f;
    if (!on || pyramid.holds(texels(width, rows))) return f;
    refit(f, pyramid, texels(width, rows), PYRAMID);
    return f;
  }
  bool in_place(uint32_t width, uint32_t rows) const { return on && pyramid.holds(texels(width, rows)); }
  void release() {
    on = false;
    pyramid.release();
  }
};

// The gather queries' workspace (pt_gather_irradiance, pt_bake_probes; no option of its own: it lives under PT_OPT_RAY_QUERIES and
// is released with the query planes): one allocation of floats — the 64 lanes' carried partial sums of the item that straddles a
// batch boundary, in TWO slots of 64 * 28 (a batch's reduce reads the slot the batch before wrote and writes the other: reader
// and writer are different waves of one launch), then the staging of the items one batch touches (K = pix / 64 + 2 of them: the PtGatherPoint going
// up, 8 floats each, and the records coming down, 28 floats each, a PtProbeSH's size) — 14 336 + 144 K bytes.  Fitted by the
// first call and again where the rows in place outgrew it; SCRATCH: nothing in it outlives a call, so it carries no validity and
// has no row in the change table of pt_ctx_state.hpp, and it is not zeroed.
struct GatherSet {
  enum : uint32_t { WORK = 1 };
  static constexpr size_t kSlot = (size_t)ptgather::kLanes * ptgather::kMaxAcc, kCarry = 2 * kSlot, kPoint = 8, kRecord = 28;
  DevBuf<float> work;

  static size_t items(const Extent& e) { return e.pix / ptgather::kMinDirections + 2; }
  static size_t floats(const Extent& e) { return kCarry + (kPoint + kRecord) * items(e); }
  Fit fit(const Extent& e) {
    Fit f;
    if (work.holds_at_least(floats(e))) return f;
    refit(f, work, floats(e), WORK);
    return f;
  }
  bool in_place(const Extent& e) const { return work.holds_at_least(floats(e)); }
  float* carry(uint32_t slot) const { return work.get() + (slot & 1u) * kSlot; }  // the two slots: a batch writes its parity's
  float* points() const { return work.get() + kCarry; }
  float* records(const Extent& e) const { return work.get() + kCarry + kPoint * items(e); }
  void release() { work.release(); }
};

// The probe lattices' two buffers (pt_bake_lattice, pt_shade_probes; no option of their own).  `points`: the generator's
// PtGatherPoint per node of a bake's slice (8 floats each) — it lives under PT_OPT_RAY_QUERIES and is released with the query
// planes.  `stage`: the staging of a HOST `probes` array of pt_shade_probes (28 floats per node, a PtProbeSH's size) — it lives
// under PT_OPT_FEATURES and is released with the feature planes.  Each is sized by the LATTICE of the call, not by the rows: fitted
// by the first call that needs it and again where a call's nodes outgrew it, in place for those nodes or refused.  SCRATCH, like
// the glare pyramid: every call writes all it reads, so neither carries validity, has a row in the change table of
// pt_ctx_state.hpp or is zeroed.
struct ProbeSet {
  enum : uint32_t { POINTS = 1, STAGE = 2 };
  static constexpr size_t kPoint = 8, kRecord = 28;
  DevBuf<float> points, stage;

  Fit fit_points(size_t nodes) {
    Fit f;
    if (!points.holds_at_least(kPoint * (nodes ? nodes : 1))) refit(f, points, kPoint * (nodes ? nodes : 1), POINTS);
    return f;
  }
  Fit fit_stage(size_t nodes) {
    Fit f;
    if (!stage.holds_at_least(kRecord * (nodes ? nodes : 1))) refit(f, stage, kRecord * (nodes ? nodes : 1), STAGE);
    return f;
  }
  bool points_in_place(size_t nodes) const { return points.holds_at_least(kPoint * (nodes ? nodes : 1)); }
  bool stage_in_place(size_t nodes) const { return stage.holds_at_least(kRecord * (nodes ? nodes : 1)); }
  void release_points() { points.release(); }
  void release_stage() { stage.release(); }
};

// PT_OPT_NEXT_EVENT: the light table of the scene in place — n records (pt_nee.hpp Light), one allocation of at least max(n, 1).
// It is sized by the SCENE, not by the rows: no resize and no repartition touches it; pt_set_spheres rebuilds it while the option
// is on, and turning the option on over an installed scene builds it.  `n` speaks for the table only while it is in place: a
// refused allocation leaves n = 0 and the buffer empty, and the render calls answer PT_ERR_CAPACITY until a later fit succeeds.
template <class Record>
struct LightSet {
  enum : uint32_t { TABLE = 1 };
  bool on = false;
  uint32_t n = 0;  // lights in the table (0: a scene without lights, or no scene yet)
  DevBuf<Record> table;

  Fit fit(uint32_t n_lights) {
    Fit f;
    n = 0;
    if (!on) return f;
    const size_t want = n_lights ? n_lights : 1u;
    if (table.capacity() < want && !refit(f, table, want, TABLE)) return f;
    n = n_lights;
    return f;
  }
  bool in_place() const { return on && table.holds_at_least(n ? n : 1u); }
  void release() {
    on = false;
    n = 0;
    table.release();
  }
};

}  // namespace ptbuf
