/*
 * overlay_ref.c — TEST-SIDE restatement of one pass with the shader's debug overlay (static/shader.frag:307-318), built on
 * the CPU oracle's exported pieces.  TEST INFRASTRUCTURE ONLY, compiled by tests/overlay_ref.py (-ffp-contract=off, linked
 * against oracle/libpt_oracle.so).
 *
 * The oracle's own ray_color skips the overlay, and the oracle is not to be edited, so its pixel_pass_sum is rebuilt here
 * from what it exports: ora_v_position / ora_init_seed (the pixel's seed), ora_hash2 / ora_camera_ray (one camera sample),
 * per bounce ora_hit_world (hit point, face-forward normal, uuid) -> the overlay test -> PT_EMISSIVE by the sphere's type
 * -> ora_scatter (attenuation, new ray, seed_after); an escaping ray's value is ora_ray_color with max_depth 1, which for
 * a ray that misses is background(r) (black in black-background mode) times a throughput of 1.  With the overlay off the
 * result is ora_render_pass bit for bit (tests/test_overlay_cpu.py), which is what validates the restatement.
 *
 * The overlay, DESIGN.md §3 "debug overlay": v = hit_point - cursor_point (three fp32 subtractions), l2 = dot3(v, v) (the fma
 * chain z, y, x), on the cursor when sqrtf(l2) < 0.1f -> the sample is (0, 0, 1); otherwise uuid == selected_object &&
 * dot3(normal, direction) > -0.05f -> (1, 0, 0); either ends the path, not multiplied by the throughput, seed untouched.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../include/ptrace.h"

typedef struct OraHit {
  int32_t hit;
  int32_t index; /* uuid */
  float t;
  float point[3];
  float normal[3];
  int32_t front_face;
} OraHit;

typedef struct OraScatter {
  int32_t did_scatter;
  float attenuation[3];
  float origin[3];
  float direction[3];
  float seed_after;
} OraScatter;

extern float ora_v_position(uint32_t p, uint32_t extent);
extern float ora_init_seed(float vx, float vy, float t);
extern void ora_hash2(float* seed, float out[2]);
extern void ora_camera_ray(const PtParams* p, float s, float t, float* seed, float origin[3], float dir[3]);
extern int ora_hit_world(const PtSphere* spheres, uint32_t n, const float origin[3], const float dir[3], OraHit* out);
extern int ora_scatter(const PtSphere* spheres, uint32_t n, const float origin[3], const float dir[3], float seed, OraScatter* out);
extern void ora_ray_color(const PtSphere* spheres, uint32_t n, const PtParams* p, const float origin[3], const float dir[3],
                          float* seed, float out[3], uint64_t* segments);

/* what the coverage tests ask of a case (tests/test_overlay_cpu.py) */
typedef struct OvlTally {
  uint64_t segments;            /* hit_world invocations, as the oracle counts them */
  uint64_t blue_paths;          /* paths ended on the cursor dot */
  uint64_t red_paths;           /* paths ended on the outline */
  uint64_t deep_overlay_paths;  /* of those, ended after at least one bounce */
  uint64_t selected_plain_hits; /* hits on the selected sphere that were neither (the path went on) */
} OvlTally;

typedef struct Overlay {
  int enable;
  int32_t selected;
  float cursor[3];
} Overlay;

static float dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

static const PtSphere* by_uuid(const PtSphere* s, uint32_t n, int32_t uuid) {
  for (uint32_t i = 0; i < n; i++)
    if (s[i].uuid == uuid) return &s[i];
  return 0;
}

/* ray_color, static/shader.frag:297-339, with :307-318 alive.  flags: bit 0 a blue, bit 1 a red contribution */
static void ray_color(const PtSphere* s, uint32_t n, const PtParams* p, const Overlay* ov, float o[3], float d[3], float* seed,
                      float out[3], OvlTally* tally, unsigned* flags) {
  float col[3] = {1.0f, 1.0f, 1.0f};
  for (int i = 0; i < p->max_depth; i++) {
    OraHit h;
    tally->segments++;
    if (ora_hit_world(s, n, o, d, &h)) {
      if (ov->enable) {
        const float v[3] = {h.point[0] - ov->cursor[0], h.point[1] - ov->cursor[1], h.point[2] - ov->cursor[2]};
        if (sqrtf(dot3(v, v)) < 0.1f) {
          out[0] = 0.0f; out[1] = 0.0f; out[2] = 1.0f;
          tally->blue_paths++;
          tally->deep_overlay_paths += i > 0;
          *flags |= 1u;
          return;
        }
        if (h.index == ov->selected) {
          if (dot3(h.normal, d) > -0.05f) {
            out[0] = 1.0f; out[1] = 0.0f; out[2] = 0.0f;
            tally->red_paths++;
            tally->deep_overlay_paths += i > 0;
            *flags |= 2u;
            return;
          }
          tally->selected_plain_hits++;
        }
      }
      const PtSphere* sp = by_uuid(s, n, h.index); /* the tests' scenes use unique uuids */
      if (sp && sp->type == PT_EMISSIVE) {
        out[0] = col[0] * sp->albedo[0]; out[1] = col[1] * sp->albedo[1]; out[2] = col[2] * sp->albedo[2];
        return;
      }
      OraScatter sc;
      ora_scatter(s, n, o, d, *seed, &sc);
      *seed = sc.seed_after; /* METAL draws also when it then absorbs */
      if (!sc.did_scatter) {
        out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
        return;
      }
      for (int k = 0; k < 3; k++) {
        o[k] = sc.origin[k];
        d[k] = sc.direction[k];
        col[k] = col[k] * sc.attenuation[k];
      }
    } else {
      /* background(r), or black: the oracle's ray_color for a ray that misses, depth 1, throughput 1 */
      PtParams q = *p;
      q.max_depth = 1;
      float bg[3], scratch_seed = *seed;
      uint64_t seg = 0;
      ora_ray_color(s, n, &q, o, d, &scratch_seed, bg, &seg);
      if (p->background_mode == PT_BG_BLACK) { /* `return vec3(0.)`, not a product */
        out[0] = bg[0]; out[1] = bg[1]; out[2] = bg[2];
        return;
      }
      out[0] = col[0] * bg[0]; out[1] = col[1] * bg[1]; out[2] = col[2] * bg[2];
      return;
    }
  }
  out[0] = col[0]; out[1] = col[1]; out[2] = col[2]; /* :338 */
}

static int row_owned(const PtParams* p, uint32_t y) {
  if (p->band_count <= 1 || p->band_rows == 0) return 1;
  return (y / p->band_rows) % p->band_count == p->band_index;
}

/*
 * One pass at u_time over the owned rows inside the window [x0, x1) x [y0, y1) (global pixel coordinates): ADDS each pixel's
 * radiance sum into accum (local_rows * width float4, .w += spp), ORs each pixel's flags into `flags` (local_rows * width
 * bytes, may be NULL) and adds to *tally.  cursor may be NULL with enable == 0.
 */
__attribute__((visibility("default"))) void ovl_render_pass(const PtSphere* s, uint32_t n, const PtParams* p, float u_time,
                                                            int enable, int32_t selected, const float* cursor, float* accum,
                                                            uint8_t* flags, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1,
                                                            OvlTally* tally) {
  Overlay ov = {enable, selected, {0.0f, 0.0f, 0.0f}};
  if (cursor) memcpy(ov.cursor, cursor, sizeof ov.cursor);
  if (x1 > p->width) x1 = p->width;
  if (y1 > p->height) y1 = p->height;
  const float fw = (float)p->width, fh = (float)p->height;
  uint32_t local = 0;
  for (uint32_t y = 0; y < p->height; y++) {
    if (!row_owned(p, y)) continue;
    const uint32_t ly = local++;
    if (y < y0 || y >= y1) continue;
    for (uint32_t x = x0; x < x1; x++) {
      /* pixel_pass_sum: static/shader.frag:406-413 + :360-373 up to the /spp */
      const float vx = ora_v_position(x, p->width), vy = ora_v_position(y, p->height);
      float seed = ora_init_seed(vx, vy, u_time);
      const float st_s = (vx + 1.0f) * 0.5f, st_t = (vy + 1.0f) * 0.5f;
      float sum[3] = {0.0f, 0.0f, 0.0f};
      unsigned fl = 0;
      for (int i = 0; i < p->samples_per_pixel; i++) {
        float rnd[2], o[3], d[3], c[3];
        ora_hash2(&seed, rnd);
        const float sx = st_s + rnd[0] / fw, sy = st_t + rnd[1] / fh;
        ora_camera_ray(p, sx, sy, &seed, o, d);
        ray_color(s, n, p, &ov, o, d, &seed, c, tally, &fl);
        sum[0] = sum[0] + c[0]; sum[1] = sum[1] + c[1]; sum[2] = sum[2] + c[2];
      }
      float* a = accum + 4 * ((size_t)ly * p->width + x);
      a[0] += sum[0]; a[1] += sum[1]; a[2] += sum[2]; a[3] += (float)p->samples_per_pixel;
      if (flags) flags[(size_t)ly * p->width + x] |= (uint8_t)fl;
    }
  }
}
