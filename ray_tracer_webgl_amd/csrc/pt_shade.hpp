// pt_shade.hpp — what happens at the end of a segment: static/shader.frag:304-338 (miss ->
// background :289-294, hit -> hit record :166-171, front face :136-143, scatter :210-286,
// depth bookkeeping :300,:338) and the end-of-item store.
//
// EXACTNESS ARGUMENT carried by this file: the outward normal's three divisions by the radius use
// div_core under a per-lane range guard (|radius| in [2^-20, 2^20), every numerator with
// 2^-103 <= |n| < 2^76; a zero numerator takes the plain operator because its quotient's sign of
// zero comes from v_div_fixup); everything else is the oracle's operation order, statement by
// statement.  RNG draws happen exactly where the shader draws them (one random_in_unit_sphere for
// DIFFUSE :217 and METAL :240 alike — also when fuzz is 0 —, one hash1 for GLASS :267).
#pragma once
#include "pt_nee.hpp"
#include "pt_scene.hpp"

namespace ptk {

// shade the lanes whose walk / scan has finished (`p.alive && !carried`): the closest hit is
// (h.closest, h.hit) — walk kernels: the slot cw.hit_pos, whose copy of the sphere and of its
// material record are read instead of going through the list index
// RR: the opt-in Russian-roulette build of a kernel (PT_OPT_RUSSIAN_ROULETTE); the kernels without it
// carry none of its code or registers
// DBG: the opt-in debug-overlay build (pt_set_debug_overlay; pt_kernels_debug.hip), carried the same way
// FEAT: the opt-in first-hit feature build (pt_render_features; pt_kernels_features.hip): the complete hit record — or the
// miss — goes to the four planes behind A.slab and the path ends; no draw, no scatter, no colour store
// QRY: the opt-in ray-query build (pt_query_rays; pt_kernels_query.hip): FEAT's store IS its store — the planes behind A.slab are
// the query planes, the work item is the ray's place — and nothing in here differs
// NEE: the opt-in next-event build (PT_OPT_NEXT_EVENT; pt_kernels_nee.hip): one light sample at every DIFFUSE hit whose path goes
// on, its shadow ray walked as the lane's next segment (pt_scene.hpp NeeState, pt_nee.hpp has the statements); the light table
// travels in PtKernelArgs::uuid and L in dbg_selected (pt_kernel_args.h), read from the kernarg segment at the point of use
// RAD: read here only together with NEE (pt_kernels_radiance_nee.hip) and only for WHERE that table travels — a radiance-query
// build's staged rays lie behind uuid, so its table comes behind slot_uuid (pt_scene.hpp nee_light_table); the shade is NEE's
template <typename S, bool RR, bool COUNT, bool DBG = false, bool FEAT = false, bool QRY = false, bool NEE = false, bool RAD = false>
__device__ __forceinline__ void shade_segment(const PtKernelArgs& A, Path& p, const Hit& h, const Carry& cw, Tally<COUNT>& tally, typename NeeArgOf<NEE>::type ne) {
  static_assert(!NEE || (!RR && !DBG && !FEAT && !COUNT), "next-event estimation excludes roulette, the overlay, the doors and the twins");
  tally.flag(PT_REG_SHADE_ANY);
  // local copies, written back at the end (see pt_grid_walk.hpp: references would be memory to the
  // passes that run before inlining)
  bool alive = p.alive, new_path = p.new_path;
  const uint32_t slab_index = p.slab_index; const uint32_t item_tile = p.item_tile; uint32_t item_segs = p.item_segs;
  int sample = p.sample, depth = p.depth; float seed = p.seed;
  V3 o = p.o, d = p.d; float a = p.a; V3 col = p.col, sum = p.sum;
  const float closest = h.closest; const int hit = h.hit; const uint32_t hit_pos = cw.hit_pos;
  (void)hit_pos;
  item_segs++;
  if constexpr (NEE) {
    // THE SHADOW SEGMENT's end: no bounce (no draw, no depth).  The light's term is added when the closest hit along (x, omega)
    // is the light itself — by list index; a walk's hit by slot through bvh_slot_index, as the feature build reads it —, then the
    // path goes on from the same origin along the scattered ray its DIFFUSE hit drew.
    if (ne.pending()) {
      int index = hit;
      if constexpr (S::TREE) {
        if (hit >= 0 && hit_pos != 0xffffffffu) index = (int)A.bvh_slot_index[hit_pos];
      }
      karg_t* K = kargs();
      const float4 l1 = nee_light_table<RAD>(K)[2 * ne.light() + 1];  // albedo.xyz, list index
      if (hit >= 0 && index == __float_as_int(l1.w)) {
        float s3[3] = {sum.x, sum.y, sum.z};
        const float t3[3] = {col.x, col.y, col.z}, a3[3] = {l1.x, l1.y, l1.z};
        ptnee::add(s3, t3, a3, ne.wgt);
        p.sum = mk(s3[0], s3[1], s3[2]);
      }
      ne.clear_pending();
      p.d = ne.nd; p.a = dot3(ne.nd, ne.nd);
      p.item_segs = item_segs;
      return;
    }
  }
  bool finished = false; // this camera path is over
  bool nee_skip = false; // NEE: the emissive sphere reached was the light sample's to estimate
  (void)nee_skip;
  // ONE copy of what several outcomes share.  The lanes of a wave end their segments differently (sky, DIFFUSE,
  // METAL, GLASS ...) and a wave runs every branch some lane takes: the sky and GLASS both want 1 / sqrt(|d|^2), and
  // DIFFUSE, METAL and GLASS all begin their draw with the same seed step + hash.  Both are computed once, in straight
  // line for every lane (no lane masks to set up and restore: a region costs more scalar work than it saves vector work;
  // the seed moves only for the lanes that draw): State::default -1.4 %, config 5 -0.6 %, configs 2 and 4 +-0.1 %
  // (profiles/r04_ab_runs.txt).
  int mtype = -1;
  V3 hp = mk(0.f, 0.f, 0.f), n = hp, alb = hp; bool front = false; float fuzz = 0.f, ri = 1.f, inv_ri = 1.f;
  if (hit >= 0) {
    tally.flag(PT_REG_SHADE_HIT_RECORD);
    float4 g;
    if constexpr (S::TREE) { // the walk's hits come with their slot (same four floats as the list entry)
      if (hit_pos != 0xffffffffu) g = S::slot_at(A, hit_pos);
      else g = S::geom_at(A, (uint32_t)hit);
    } else {
      g = S::geom_at(A, (uint32_t)hit);
    }
    const float4* mp = reinterpret_cast<const float4*>(A.mat + hit);
    if constexpr (S::TREE) { // one load instead of index -> material (two dependent memory round trips)
      if (hit_pos != 0xffffffffu) mp = reinterpret_cast<const float4*>(A.slot_mat + hit_pos);
    }
    float4 m0 = mp[0]; // albedo.xyz, fuzz
    float4 m1 = mp[1]; // refraction_index, type, radius, 1 / refraction_index
    mtype = __float_as_int(m1.y);
    float radius = m1.z;
    fuzz = m0.w; ri = m1.x; inv_ri = m1.w;
    hp = mk(fma_(d.x, closest, o.x), fma_(d.y, closest, o.y), fma_(d.z, closest, o.z)); // hit record, :166-171
    const float nx = hp.x - g.x, ny = hp.y - g.y, nz = hp.z - g.z; // outward normal (p - centre) / radius, :168 (see above)
    V3 on;
    const float n_lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(nx), __builtin_fabsf(ny)), __builtin_fabsf(nz));
    const float n_hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(nx), __builtin_fabsf(ny)), __builtin_fabsf(nz));
    const uint32_t r_guard = div_den_ok(radius) ? f2u(0x1p76f) - f2u(0x1p-103f) : 0u;
    const bool n_odd = f2u(n_lo) - f2u(0x1p-103f) >= r_guard || f2u(n_hi) - f2u(0x1p-103f) >= r_guard;
    const float yr = rcp_newton(radius);
    on = mk(div_core(nx, radius, yr), div_core(ny, radius, yr), div_core(nz, radius, yr));
    if (__builtin_expect(pt_ballot(n_odd) != 0ull, 0)) { // (rare)
      if (n_odd) on = mk(nx / radius, ny / radius, nz / radius);
    }
    front = dot3(d, on) < 0.0f; // :137
    n = front ? on : mk(-on.x, -on.y, -on.z);
    alb = mk(m0.x, m0.y, m0.z);
    if constexpr (NEE) {
      // NO DOUBLE COUNTING: a segment that starts at a vertex where the light sample ran and ends on a LIGHT adds the emission
      // only if the light could not be sampled from there, !P(o, j).  A sphere that was hit has a finite centre and r * r; it
      // is in the table if its radius is not zero and its albedo is finite (ptnee::is_light).
      if (ne.sampled() && mtype == 3) {
        const float x3[3] = {o.x, o.y, o.z}, c3[3] = {g.x, g.y, g.z};
        float w3[3], d2;
        const bool reached = ptnee::reach(x3, c3, g.w, w3, d2);
        nee_skip = reached && radius != 0.0f && ptnee::is_finite(m0.x) && ptnee::is_finite(m0.y) && ptnee::is_finite(m0.z);
      }
    }
    if constexpr (DBG) {
      // DEBUG OVERLAY — opt-in (pt_set_debug_overlay), static/shader.frag:307-318, on the complete hit record: before the
      // PT_EMISSIVE test and before any scatter draw.  The cursor dot: |hit point - cursor| < 0.1 -> the sample is (0, 0, 1);
      // otherwise the outline of the selected sphere: uuid == selected && dot(normal, direction) > -0.05 -> (1, 0, 0).  Either
      // is the `return` of the shader: not multiplied by the throughput, and the path ends without a draw — it is
      // handed on as a material nothing recognises (:284-285: no seed step, no contribution).  Its four uniforms and the
      // uuid arrays are read from the kernarg segment HERE (pt_scene.hpp kargs): they hold no SGPR across the walk.
      karg_t* K = kargs();
      const V3 v = mk(hp.x - K->dbg_cursor[0], hp.y - K->dbg_cursor[1], hp.z - K->dbg_cursor[2]);
      const bool on_cursor = sqrt_rn(dot3(v, v)) < 0.1f;
      const int32_t* up = K->uuid + hit;  // the caller's value (PtSphere.uuid), not the list index
      if constexpr (S::TREE) {
        if (hit_pos != 0xffffffffu) up = K->slot_uuid + hit_pos;
      }
      const bool on_outline = *up == K->dbg_selected && dot3(n, d) > -0.05f;
      if (on_cursor || on_outline) {
        sum.x += on_cursor ? 0.0f : 1.0f; sum.y += 0.0f; sum.z += on_cursor ? 1.0f : 0.0f;
        mtype = 4;
      }
    }
  }
  if constexpr (FEAT) {
    // FIRST-HIT FEATURES — opt-in (PT_OPT_FEATURES, pt_render_features; include/ptrace.h has the record).  Four planes of
    // local_rows * width 16-byte texels behind A.slab, plane k at k * local_rows * width; the launch has one pass, so
    // slab_index is the local pixel.  A hit stores what the record above holds and nothing else; a miss stores what the sky
    // branch below adds for a throughput of 1.  The uuid arrays are read from the kernarg segment here, as the overlay reads them.
    karg_t* K = kargs();
    float4* planes = reinterpret_cast<float4*>(A.slab);
    const uint32_t plane = K->local_rows * K->width;
    float4 t_alb = make_float4(0.f, 0.f, 0.f, 0.f), t_n = t_alb, t_hp = t_alb;
    int4 t_ids = make_int4(-1, -1, -1, 0);
    if (hit >= 0) {
      int index = hit;
      const int32_t* up = K->uuid + hit;
      if constexpr (S::TREE) {
        if (hit_pos != 0xffffffffu) { index = (int)A.bvh_slot_index[hit_pos]; up = K->slot_uuid + hit_pos; }
      }
      t_alb = make_float4(alb.x, alb.y, alb.z, closest);
      t_n = make_float4(n.x, n.y, n.z, 0.f);
      t_hp = make_float4(hp.x, hp.y, hp.z, 0.f);
      t_ids = make_int4(index, *up, mtype, front ? 1 : 0);
    } else if (A.background_mode == 0) { // background(), :289-294, times a throughput of 1 into a sum of 0
      const float uy = d.y * inv_sqrt_rn(a);
      const float t = 0.5f * (uy + 1.0f);
      const float omt = 1.0f - t;
      t_alb = make_float4(0.0f + col.x * fma_(0.5f, t, omt), 0.0f + col.y * fma_(0.7f, t, omt), 0.0f + col.z * fma_(1.0f, t, omt), 0.f);
    }
    planes[slab_index] = t_alb;
    planes[plane + slab_index] = t_n;
    planes[2u * plane + slab_index] = t_hp;
    reinterpret_cast<int4*>(planes)[3u * plane + slab_index] = t_ids;
    p.alive = false; p.new_path = false; p.item_segs = item_segs;
    return;
  }
  const bool sky = hit < 0 && A.background_mode == 0;
  const float inv = inv_sqrt_rn(a); // background() :290, GLASS :253
  float seed_drawn = seed;
  const uint32_t draw = seed_step_hash(seed_drawn); // DIFFUSE :217, METAL :240 (hash3), GLASS :267 (hash1)
  seed = (uint32_t)mtype <= 2u ? seed_drawn : seed;
  if (hit < 0) {
    if (sky) { // background(), :289-294
      tally.flag(PT_REG_SHADE_SKY);
      float uy = d.y * inv;
      float t = 0.5f * (uy + 1.0f);
      float omt = 1.0f - t;
      sum.x += col.x * fma_(0.5f, t, omt);
      sum.y += col.y * fma_(0.7f, t, omt);
      sum.z += col.z * fma_(1.0f, t, omt);
    }
    finished = true;
  } else {
    const V3 p = hp;
    if (mtype == 0 || mtype == 1) {
      V3 rs = random_in_unit_sphere_from(draw); // both DIFFUSE (:217) and METAL (:240) draw one
      V3 nd;
      bool ok = true;
      if (mtype == 0) { // DIFFUSE :212-229
        tally.flag(PT_REG_SHADE_DIFFUSE);
        V3 ruv = normalize3(rs);
        nd = mk(n.x + ruv.x, n.y + ruv.y, n.z + ruv.z);
      } else { // METAL :232-247
        tally.flag(PT_REG_SHADE_METAL);
        V3 refl = reflect3(d, n);
        nd = mk(fma_(fuzz, rs.x, refl.x), fma_(fuzz, rs.y, refl.y), fma_(fuzz, rs.z, refl.z));
        ok = dot3(n, nd) > 0.0f;
      }
      if (ok) {
        o = p; d = nd;
        col.x *= alb.x; col.y *= alb.y; col.z *= alb.z;
      } else {
        finished = true; // absorbed: return vec3(0.) :327-329
      }
    } else if (mtype == 2) { // GLASS :250-282
      tally.flag(PT_REG_SHADE_GLASS);
      float ratio = front ? inv_ri : ri;  // :252 `1.0 / ri`: the host's quotient, same bits as the division here (pt_kernel_args.h)
      V3 ud = mk(d.x * inv, d.y * inv, d.z * inv);
      float cdot = dot3(mk(-ud.x, -ud.y, -ud.z), n);
      float cos_theta = (1.0f < cdot) ? 1.0f : cdot; // min(cdot, 1.0)
      float sin_theta = sqrt_rn(fma_(-cos_theta, cos_theta, 1.0f));
      bool cannot_refract = ratio * sin_theta > 1.0f;
      float refl_amount;
      if constexpr (S::SMALL) {  // r0 from the host: the same bits as reflectance()'s own (pt_api.hip pt_set_spheres)
        const float r0 = A.mat_r0[2u * (uint32_t)hit + (front ? 0u : 1u)];
        const float x = 1.0f - cos_theta, x2 = x * x, x5 = (x2 * x2) * x;
        refl_amount = fma_(1.0f - r0, x5, r0);
      } else {
        refl_amount = reflectance(cos_theta, ratio);
      }
      float rnd = (float)draw * (1.0f / 4294967296.0f); // hash1 :21-24
      V3 nd;
      if (cannot_refract || refl_amount > rnd) {
        nd = reflect3(ud, n);
      } else { // GLSL refract
        tally.flag(PT_REG_SHADE_GLASS_REFRACT);
        float dni = dot3(n, ud);
        float k = fma_(-(ratio * ratio), fma_(-dni, dni, 1.0f), 1.0f);
        if (k < 0.0f) {
          nd = mk(0.f, 0.f, 0.f);
        } else {
          float t = fma_(ratio, dni, sqrt_rn(k));
          nd = mk(fma_(-t, n.x, ratio * ud.x), fma_(-t, n.y, ratio * ud.y),
                  fma_(-t, n.z, ratio * ud.z));
        }
      }
      o = p; d = nd;
      col.x *= alb.x; col.y *= alb.y; col.z *= alb.z;
    } else if (mtype == 3) { // EMISSIVE (extension): radiance = throughput * emission
      if constexpr (NEE) {
        if (!nee_skip) { sum.x += col.x * alb.x; sum.y += col.y * alb.y; sum.z += col.z * alb.z; }
      } else {
        sum.x += col.x * alb.x; sum.y += col.y * alb.y; sum.z += col.z * alb.z;
      }
      finished = true;
    } else {
      finished = true; // unrecognised material absorbs, :284-285
    }
    if (!finished) {
      tally.flag(PT_REG_SHADE_CONTINUES);
      a = dot3(d, d);
      depth++;
      if (depth >= A.max_depth) { // loop bound :300 exhausted -> return color :338
        sum.x += col.x; sum.y += col.y; sum.z += col.z;
        finished = true;
      }
      if constexpr (RR) if (!finished && depth >= A.rr_min_depth) {
        // RUSSIAN ROULETTE — opt-in (PT_OPT_RUSSIAN_ROULETTE), NOT the reference's estimator sample for
        // sample: static/shader.frag:297-339 never ends a path early.  After rr_min_depth bounces a path
        // survives with probability q = min(max(throughput), 1) and, if it does, carries throughput / q:
        // E[throughput'] = q (throughput / q) = throughput, so every pixel's expectation — including the
        // `return color` term of depth exhaustion — is the reference's; only the variance and the work
        // change.  One extra hash1 draw per decision, which moves this stream's later random numbers:
        // images of this mode are compared with the oracle statistically (tests/test_gpu_roulette.py),
        // never bit for bit.
        const float q = __builtin_fminf(__builtin_fmaxf(__builtin_fmaxf(col.x, col.y), col.z), 1.0f);
        const float xi = hash1(seed);
        if (!(xi < q)) { // also ends paths whose throughput is 0 or NaN
          finished = true;
        } else {
          const float inv = 1.0f / q;
          col.x *= inv; col.y *= inv; col.z *= inv;
        }
      }
      if constexpr (NEE) {
        // THE LIGHT SAMPLE — opt-in (PT_OPT_NEXT_EVENT), after the shader's own scatter draw and depth test, at a DIFFUSE hit whose
        // path goes on, when there is a light: one hash3, a light, a direction inside the cone the light subtends (pt_nee.hpp).
        // With cos_s > 0 the lane's next segment is the shadow ray; the scattered direction waits in ne.nd.
        karg_t* K = kargs();
        const int n_lights = nee_light_count<RAD>(K);
        const bool smp = !finished && mtype == 0 && n_lights > 0;
        ne.set_sampled(smp);
        if (smp) {
          float u0, u1, u2;
          hash3(seed, u0, u1, u2);
          const int k = ptnee::choose(u0, n_lights);
          const float4 l0 = nee_light_table<RAD>(K)[2 * k];  // centre, r * r
          const float x3[3] = {o.x, o.y, o.z}, c3[3] = {l0.x, l0.y, l0.z};
          float w3[3], d2;
          if (ptnee::reach(x3, c3, l0.w, w3, d2)) {
            float sp, cp, om3[3], om;
            sincos2pi(u2, sp, cp);
            ptnee::sample(w3, d2, l0.w, u1, sp, cp, om3, om);
            const float n3[3] = {n.x, n.y, n.z};
            const float cos_s = ptnee::cos_at(n3, om3);
            if (cos_s > 0.0f) {
              ne.set_pending(k); ne.wgt = ptnee::weight(n_lights, om, cos_s);
              ne.nd = d;
              d = mk(om3[0], om3[1], om3[2]);
              a = dot3(d, d);
            }
          }
        }
      }
    }
  }
  if constexpr (NEE) { if (finished) ne.set_sampled(false); }

  if (finished) {
    tally.flag(PT_REG_SHADE_FINISHED);
    sample++;
    if (sample >= A.spp) {
      tally.flag(PT_REG_SHADE_ITEM_STORE);
      // (a plain store: the non-temporal form — global_store_dwordx4 ... nt — measured no time change and MORE written traffic,
      // config 5 WRITE_SIZE 0.87 -> 1.37 GiB per 16-pass launch against 0.53 GB of slab: profiles/r06_ab_runs.txt)
      float4 outv = make_float4(sum.x, sum.y, sum.z, (float)A.spp);
      reinterpret_cast<float4*>(A.slab)[slab_index] = outv;
      if (item_tile != 0xffffffffu) atomicMax(&A.tile_cost[item_tile], item_segs);
      alive = false;
    } else {
      new_path = true;
    }
  }
  p.alive = alive; p.new_path = new_path; p.item_segs = item_segs;
  p.sample = sample; p.depth = depth; p.seed = seed;
  p.o = o; p.d = d; p.a = a; p.col = col; p.sum = sum;
}

} // namespace ptk
