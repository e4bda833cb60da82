// pt_refill.hpp — where a lane's work comes from: the global work queue, the decode of a work item
// into a fragment (static/shader.vert:8, static/shader.frag:354-357, :410), and the camera ray of
// the fragment's next sample (static/shader.frag:365-370 + :342-351).
//
// EXACTNESS ARGUMENT carried by this file: (i) scheduling never changes a result — an item is one
// (pixel, pass) stream whose seed is a function of (v_position, u_time) only (:354-357), its radiance
// sum goes to its own slab slot, so WHICH lane runs it and WHEN is free; (ii) the pixel-centre and
// jitter divisions by the image size use div_core under the wave-uniform guard `wh_ok` (width and
// height in [2^-20, 2^20): numerators are odd integers >= 1 or values that are 0 or >= 2^-31 and < 1,
// inside div_core's range; a +0 numerator gives +0 either way) and the plain operators otherwise.
#pragma once
#include "pt_scene.hpp"
#include "pt_query.hpp"

namespace ptk {

// uniform divisors of the image size: kept in SGPRs for the kernel's lifetime
struct PixelDiv {
  bool wh_ok;        // wave-uniform: div_core applies to divisions by width and height
  float y_fw, y_fh;  // rcp_newton of float(width), float(height)
};
__device__ __forceinline__ PixelDiv pixel_div() {
  karg_t& K = *kargs();
  PixelDiv pd;
  pd.wh_ok = div_den_ok(K.fw) && div_den_ok(K.fh);
  pd.y_fw = u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(rcp_newton(K.fw))));
  pd.y_fh = u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(rcp_newton(K.fh))));
  return pd;
}

// start the next camera path of this lane's item: static/shader.frag:365-370 + :342-351
// the pixel jitter is divided by the image size (:367-368)
// FEAT: the first-hit feature build's ray (include/ptrace.h pt_render_features) — the pixel centre through the pinhole: the
// same dd, tt and cam_o as below with no jitter and no lens; no draw is made and the seed is neither read nor moved
// QRY: the query build's ray (include/ptrace.h pt_query_rays) — the caller's, read from the query planes behind A.slab at the
// lane's work item: the origin from PT_FEAT_POINT's plane and the direction from PT_FEAT_NORMAL's, where the host staged them.
// A lane reads its own two texels here and overwrites them in shade_segment, so nobody else touches them.  Only admitted items
// come here (query_admit below): the ray is valid and within the launch's count.
// RAD: the radiance-query build's ray (include/ptrace.h pt_query_radiance) — the caller's again, for EVERY sample of the item:
// A.slab is the pass slabs here, so the query planes the host staged the rays in arrive behind K.uuid (pt_kernel_args.h), and
// the item's place in them — its local pixel, whatever its pass — is carried in st_s as bits (the decode below puts it there:
// these builds have no other use for st_s and st_t).  The seed is the item's own, set at the decode as in every plain build,
// and stays untouched: no jitter draw and no lens draws precede ray_color.  Only admitted items come here (radiance_admit).
template <bool FEAT = false, bool QRY = false, bool RAD = false>
__device__ __forceinline__ void start_sample(Path& p, const PixelDiv& pd) {
  karg_t& K = *kargs();
  if constexpr (RAD) {
    const uint32_t j = f2u(p.st_s), plane = K.local_rows * K.width;
    const float4* rays = reinterpret_cast<const float4*>(K.uuid);
    const float4 qo = rays[2u * plane + j], qd = rays[plane + j];
    const V3 o = mk(qo.x, qo.y, qo.z), d = mk(qd.x, qd.y, qd.z);
    p.o = o; p.d = d; p.a = dot3(d, d); p.col = mk(1.0f, 1.0f, 1.0f); p.depth = 0;
    return;
  }
  if constexpr (QRY) {
    const uint32_t i = p.slab_index, plane = K.local_rows * K.width;
    const float4* planes = reinterpret_cast<const float4*>(K.slab);
    const float4 qo = planes[2u * plane + i], qd = planes[plane + i];
    const V3 o = mk(qo.x, qo.y, qo.z), d = mk(qd.x, qd.y, qd.z);
    p.o = o; p.d = d; p.a = dot3(d, d); p.col = mk(1.0f, 1.0f, 1.0f); p.depth = 0;
    return;
  }
  if constexpr (FEAT) {
    const float s = p.st_s, t = p.st_t;
    const V3 dd = mk(fma_(t, K.vertical[0], fma_(s, K.horizontal[0], K.llc[0])),
                     fma_(t, K.vertical[1], fma_(s, K.horizontal[1], K.llc[1])),
                     fma_(t, K.vertical[2], fma_(s, K.horizontal[2], K.llc[2])));
    const V3 cam_o = mk(K.origin[0], K.origin[1], K.origin[2]);
    const V3 d = mk(dd.x - cam_o.x, dd.y - cam_o.y, dd.z - cam_o.z);
    p.o = cam_o; p.d = d; p.a = dot3(d, d); p.col = mk(1.0f, 1.0f, 1.0f); p.depth = 0;
    return;
  }
  float seed = p.seed;  // (local copies, written back at the end: see pt_grid_walk.hpp)
  const float st_s = p.st_s, st_t = p.st_t;
  const bool wh_ok = pd.wh_ok;
  const float y_fw = pd.y_fw, y_fh = pd.y_fh;
  V3 o, d; float a; V3 col; int depth;
  float r0, r1;
  hash2(seed, r0, r1);
  float jx, jy;
  if (wh_ok) { jx = div_core(r0, K.fw, y_fw); jy = div_core(r1, K.fh, y_fh); }
  else { jx = r0 / K.fw; jy = r1 / K.fh; }
  float s = st_s + jx;
  float t = st_t + jy;
  V3 dd = mk(fma_(t, K.vertical[0], fma_(s, K.horizontal[0], K.llc[0])),
             fma_(t, K.vertical[1], fma_(s, K.horizontal[1], K.llc[1])),
             fma_(t, K.vertical[2], fma_(s, K.horizontal[2], K.llc[2])));
  const V3 cam_o = mk(K.origin[0], K.origin[1], K.origin[2]);
  const V3 tt = mk(dd.x - cam_o.x, dd.y - cam_o.y, dd.z - cam_o.z);
  // random_in_unit_circle :123-129 draws twice whatever the lens: the seed takes its four steps here,
  // the draws themselves are made below from a copy, where their values are needed
  float seed_l = seed;
  seed = (seed + 0.1f) + 0.1f;
  seed = (seed + 0.1f) + 0.1f;
  // LENS OFF (aperture 0: State::default, src/state.rs:102,123).  Then rd = 0 * (...) and the offset
  // off = u * rd.x + v * rd.y is a vector of zeros of either sign: origin + off is the origin bit for
  // bit (its components are not -0: host-checked, as is that u and v are finite), and tt - off is tt
  // unless a component of tt is exactly -0, where the result takes its sign from off — if that
  // happens anywhere in the wave (it practically never does) the wave runs the full form below.
  bool lens = K.lens_off == 0u; // wave-uniform
  if (!lens) {
    const uint32_t nz = 0x80000000u;
    lens = pt_ballot(f2u(tt.x) == nz || f2u(tt.y) == nz || f2u(tt.z) == nz) != 0ull;
  }
  if (lens) {
    float ua = hash1(seed_l);
    float sa, ca;
    sincos2pi(ua, sa, ca);
    float rr = sqrt_rn(hash1(seed_l));
    float rdx = K.lens_radius * (rr * ca);
    float rdy = K.lens_radius * (rr * sa);
    V3 off = mk(fma_(K.cam_v[0], rdy, K.cam_u[0] * rdx), fma_(K.cam_v[1], rdy, K.cam_u[1] * rdx),
                fma_(K.cam_v[2], rdy, K.cam_u[2] * rdx));
    d = mk(tt.x - off.x, tt.y - off.y, tt.z - off.z);
    o = mk(cam_o.x + off.x, cam_o.y + off.y, cam_o.z + off.z);
  } else {
    d = tt;
    o = cam_o;
  }
  a = dot3(d, d);
  col = mk(1.0f, 1.0f, 1.0f);
  depth = 0;
  p.seed = seed; p.o = o; p.d = d; p.a = a; p.col = col; p.depth = depth;
}

// QRY: does work item i (a local pixel of the query planes) carry a ray to walk?  Decided where the item is decoded, so that an
// item that does not is dropped like one outside the image and the wave step never begins with a lane that has nothing to walk
// (ending such a lane in start_sample needs a way back from there to the refill, and with that edge in the wave-step loop the
// six walk builds spill 28-43 vector registers: profiles/r23_kernel_resources.txt).  An item at or beyond the launch's ray count
// (dbg_selected: the overlay's field, which no build but the overlay's reads as that) is dropped without a store; an invalid
// ray (pt_query.hpp ray_valid) gets its sentinel record here and is dropped too.  The two texels are read again by
// start_sample, from the cache: a refill keeps nothing of them.
__device__ __forceinline__ bool query_admit(uint32_t i) {
  karg_t& K = *kargs();
  if (i >= (uint32_t)K.dbg_selected) return false;
  const uint32_t plane = K.local_rows * K.width;
  float4* planes = reinterpret_cast<float4*>(K.slab);
  const float4 qo = planes[2u * plane + i], qd = planes[plane + i];
  if (ptq::ray_valid(qo.x, qo.y, qo.z, qd.x, qd.y, qd.z)) return true;
  ptq::F4 t_alb, t_n, t_hp; ptq::I4 t_ids;
  ptq::invalid_texels(&t_alb, &t_n, &t_hp, &t_ids);
  planes[i] = make_float4(t_alb.x, t_alb.y, t_alb.z, t_alb.w);
  planes[plane + i] = make_float4(t_n.x, t_n.y, t_n.z, t_n.w);
  planes[2u * plane + i] = make_float4(t_hp.x, t_hp.y, t_hp.z, t_hp.w);
  reinterpret_cast<int4*>(planes)[3u * plane + i] = make_int4(t_ids.x, t_ids.y, t_ids.z, t_ids.w);
  return false;
}

// RAD: does the work item at place j (its local pixel; the passes of a place share its ray) carry a ray to walk?  Decided at the
// decode for query_admit's reason.  An item at or beyond the launch's ray count (dbg_selected, as above) or with an invalid ray
// is dropped WITHOUT a store: its slab texels stay stale, and the fold kernel (pt_radiance.hpp fold_at) decides validity again
// by the same predicate and writes the zero record.  The rays lie in the query planes behind K.uuid (start_sample RAD).
__device__ __forceinline__ bool radiance_admit(uint32_t j) {
  karg_t& K = *kargs();
  if (j >= (uint32_t)K.dbg_selected) return false;
  const uint32_t plane = K.local_rows * K.width;
  const float4* rays = reinterpret_cast<const float4*>(K.uuid);
  const float4 qo = rays[2u * plane + j], qd = rays[plane + j];
  return ptq::ray_valid(qo.x, qo.y, qo.z, qd.x, qd.y, qd.z);
}

// ---- refill: the wave pulls work items for the lanes that will need one ----------------------------
// The wave reserves A.queue_chunk consecutive items from the global queue with ONE atomic
// (a memory-side atomic moves 64 B, so per-item atomics would dominate the kernel's HBM
// traffic) and deals them to its lanes from a wave-uniform local pool (the arithmetic: pt_deal.hpp).
// LOOK-AHEAD: the item decode below costs ~115 VALU instructions for the whole wave whether one lane
// needs it or sixty, and with 16-spp items about one lane per wave step runs out.  So the decode does
// not serve the lane that ran out: every lane keeps one decoded NEXT item (Path::nx_*), a lane whose
// item ends takes it at once (promote() below), and the decode runs only when some lane has neither a
// current nor a next item — then for every lane whose next slot is empty, most of the wave.  Which lane
// runs an item and when is free (exactness argument (i)), so is when it is decoded: the decode reads
// launch constants only (frame_ctr included: the frame-advance kernel of a replayed series runs between
// trace launches, never beside one).
// Every wave reaches the "queue dry" exit: the head counter is monotone, every trip of the loop deals
// an item or finds the queue dry; a wave leaves when every lane is dead after promote(), i.e. every
// slot is empty too, which the loop below lets happen only on a dry queue.
// QRY: items that carry no ray to walk are dropped at the decode (query_admit above).
// RAD: likewise (radiance_admit above); the item's place goes to start_sample in nx_s, as bits.
template <bool COUNT, bool QRY = false, bool RAD = false>
__device__ __forceinline__ void refill(const PtKernelArgs& A, Path& p, Queue& q, const PixelDiv& pd, Tally<COUNT>& tally) {
  karg_t& K = *kargs();
  // (local copies, written back at the end: see pt_grid_walk.hpp)
  const bool alive = p.alive;
  bool dry = q.dry; // wave-uniform: a reservation came back empty, so no lane of this wave will get another item
  uint32_t nx_slab = p.nx_slab, nx_tile = p.nx_tile;
  float nx_seed = p.nx_seed, nx_s = p.nx_s, nx_t = p.nx_t;
  uint32_t pool_next = q.pool_next, pool_end = q.pool_end;
  uint32_t pool_tp0 = q.pool_tp0, pool_split = q.pool_split, pool_tile0 = q.pool_tile0, pool_tile1 = q.pool_tile1;
  uint32_t q_round = q.round;
  const bool wh_ok = pd.wh_ok;
  const float y_fw = pd.y_fw, y_fh = pd.y_fh;
  for (;;) {
    const bool slot_empty = nx_slab == ptdeal::kSlotEmpty;
    if (pt_ballot(ptdeal::starving(alive, slot_empty, dry)) == 0ull) break;
    bool need = ptdeal::wants_item(alive, slot_empty, dry, K.refill_ahead != 0u);
    const unsigned long long mask = pt_ballot(need);
    if (ptdeal::pool_used_up(pool_next, pool_end)) { // wave-uniform
      tally.flag(PT_REG_REFILL_RESERVE);
      unsigned long long base = 0;
      if (K.queue_static == 2u) {
        // GROUPED queue (short launches): the waves form G groups, group g owns the reservations g, g + G, g + 2 G, ... of the
        // tile-major list and hands them to its waves in the order they ask — the balance of a queue among a group's ~28 waves
        // with one atomic per reservation on one of G addresses (the single head of the shared queue takes a reservation
        // every ~13 ns: too slow for items of a few segments; no atomics at all — static dealing — leaves every wave
        // alone with the cost of the ~31 tiles it happens to get)
        const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const uint32_t group = ptdeal::group_of(wave, K.queue_groups);
        unsigned long long r = 0;
        if (lane_id() == 0u) r = atomicAdd(&A.counters[PT_CTR_GROUP_HEADS + 8u * group], 1ull);
        const uint32_t r_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)r);
        base = ptdeal::grouped_base(r_lo, K.queue_groups, group, A.queue_chunk);
      } else if (K.queue_static != 0u) {
        // reservations dealt round-robin, no atomics (a wave's number is the same in all its lanes)
        const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        base = ptdeal::static_base(q_round, K.n_waves, wave, A.queue_chunk);
        q_round++;
      } else {
        if (lane_id() == 0u) base = atomicAdd(&A.counters[PT_CTR_HEAD], (unsigned long long)A.queue_chunk);
      }
      // wave-uniform, and known to the compiler as such (readfirstlane): the pool bookkeeping derived
      // from it then lives in SGPRs instead of occupying VGPRs for the kernel's lifetime
      base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
             (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
      if (ptdeal::reservation_dry(base, A.n_items)) { // queue dry: no lane of this wave gets another item
        tally.queue_dry();
        dry = true;
        need = false;  // nothing to deal in this trip; the loop ends at its next test
      } else {
        pool_next = (uint32_t)base;
        pool_end = ptdeal::reservation_end(base, A.queue_chunk, A.n_items);
        // a reservation no longer than one tile's items touches at most two tiles: look their numbers
        // up once, here, instead of one dependent global load per lane in every refill
        pool_tp0 = div_by(pool_next, K.div_per_tile.m, K.div_per_tile.s1, K.div_per_tile.s2);
        pool_split = (pool_tp0 + 1u) * (64u * K.n_passes);
        const uint32_t n_tiles_w = K.tiles_x * K.tiles_y;
        pool_tile0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)K.tile_order[pool_tp0]);
        pool_tile1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)K.tile_order[pool_tp0 + 1u < n_tiles_w ? pool_tp0 + 1u : pool_tp0]);
      }
    }
    const uint32_t avail = pool_end - pool_next;
    const uint32_t rank = ptdeal::rank_of(mask, lane_id());
    const uint32_t pool_base = pool_next;
    pool_next += ptdeal::taken(mask, avail);
    if (ptdeal::gets_item(need, rank, avail)) {
      tally.flag(PT_REG_REFILL_DECODE);
      uint32_t item = ptdeal::item_of(pool_base, rank);
      uint32_t per_tile = 64u * K.n_passes;
      uint32_t tile_pos, tile; // heaviest tiles are dealt first (tile_order)
      if (K.queue_chunk <= per_tile) { // wave-uniform
        const bool second = item >= pool_split;
        tile_pos = pool_tp0 + (second ? 1u : 0u);
        const uint32_t t0 = pool_tile0, t1 = pool_tile1;  // values, not a choice between two lvalues
        tile = second ? t1 : t0;
      } else {
        tile_pos = div_by(item, K.div_per_tile.m, K.div_per_tile.s1, K.div_per_tile.s2);
        tile = K.tile_order[tile_pos];
      }
      uint32_t rem_i = item - tile_pos * per_tile;
      uint32_t pass = rem_i >> 6, l = rem_i & 63u;
      uint32_t ty = div_by(tile, K.div_tiles_x.m, K.div_tiles_x.s1, K.div_tiles_x.s2), tx = tile - ty * K.tiles_x;
      uint32_t px = tx * 8u + (l & 7u), ly = ty * 8u + (l >> 3);
      bool inside = px < K.width && ly < K.local_rows;
      if constexpr (QRY) { if (inside) inside = query_admit((pass * K.local_rows + ly) * K.width + px); }
      if constexpr (RAD) { if (inside) inside = radiance_admit(ly * K.width + px); }
      if (inside) {
        uint32_t y = ly;
        if (K.band_count > 1u) {
          uint32_t b = div_by(ly, K.div_band_rows.m, K.div_band_rows.s1, K.div_band_rows.s2), r = ly - b * K.band_rows;
          y = (b * K.band_count + K.band_index) * K.band_rows + r;
        }
        // static/shader.vert:8 + rasteriser: v_position at the pixel centre
        const float fx2 = (float)(2u * px + 1u), fy2 = (float)(2u * y + 1u); // odd integers >= 1
        float vx, vy;
        if (wh_ok) { vx = div_core(fx2, K.fw, y_fw) - 1.0f; vy = div_core(fy2, K.fh, y_fh) - 1.0f; }
        else { vx = fx2 / K.fw - 1.0f; vy = fy2 / K.fh - 1.0f; }
        // frames replayed from a hipGraph (pt_render_frames) count on the device: scalar load, constant within a launch
        const uint32_t frame_k = *(const uint32_t __attribute__((address_space(4)))*)K.frame_ctr;
        float u_time = K.time0 + (float)(K.first_pass + pass + frame_k) * K.time_step;
        // init_global_seed, static/shader.frag:354-357
        nx_seed = (float)base_hash(f2u(vx), f2u(vy)) * (1.0f / 4294967296.0f) + u_time;
        nx_s = (vx + 1.0f) * 0.5f; // :410
        nx_t = (vy + 1.0f) * 0.5f;
        if constexpr (RAD) nx_s = u2f(ly * K.width + px);  // the item's place in the staged rays, for start_sample (bits, never computed with)
        nx_slab = (pass * K.local_rows + ly) * K.width + px;
        // only the launch's first pass reports its cost (atomicMax per pixel: the tile's
        // heaviest item): plenty for ordering tiles, and a memory-side atomic moves 64 B.  Launches of
        // one short pass (the reference's 1-spp frame) report nothing: there EVERY item would, the 64
        // lanes of a tile on one address, and — loads, stores and atomics complete in order — the next
        // material load of each wave would wait for them (measured on the 1280x702 1-spp frame:
        // 85 % of the wave time in s_waitcnt).
        nx_tile = (pass == 0u && K.cost_feedback != 0u) ? tile : 0xffffffffu;
      }
      // an item that falls outside the image (edge tile) is simply dropped: the slot stays empty
    }
  }
  p.nx_slab = nx_slab; p.nx_tile = nx_tile; p.nx_seed = nx_seed; p.nx_s = nx_s; p.nx_t = nx_t;
  q.pool_next = pool_next; q.pool_end = pool_end;
  q.pool_tp0 = pool_tp0; q.pool_split = pool_split; q.pool_tile0 = pool_tile0; q.pool_tile1 = pool_tile1;
  q.round = q_round; q.dry = dry;
}

// ---- promote: a lane whose item has ended takes its decoded next item --------------------------------
// At the head of the wave step, after refill() and before the camera ray: a handful of moves, no waiting.
template <bool COUNT>
__device__ __forceinline__ void promote(Path& p, Tally<COUNT>& tally) {
  if (ptdeal::promotes(p.alive, p.nx_slab == ptdeal::kSlotEmpty)) {
    tally.flag(PT_REG_REFILL_PROMOTE);
    p.seed = p.nx_seed; p.st_s = p.nx_s; p.st_t = p.nx_t;
    p.slab_index = p.nx_slab; p.item_tile = p.nx_tile; p.item_segs = 0;
    p.sum = mk(0.f, 0.f, 0.f);
    p.sample = 0;
    p.new_path = true;
    p.alive = true;
    p.nx_slab = ptdeal::kSlotEmpty;
  }
}

} // namespace ptk
