// radiance_main.cpp — a stand-alone program (its own main) that drives csrc/pt_radiance.hpp — the passes of a batch, the zero
// record and the fold — over EXACTLY sized heap buffers, with rays of every hostile operand class staged by pt_query.hpp's own
// pack, built with -fsanitize=address,undefined by tests/test_radiance_plan.py and run as a child process: an index one past a
// plane, a slab or the records ends it.  No GPU, no preloaded library.  Prints "radiance plan: ok" when everything held.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_radiance.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      failures++;                                                         \
    }                                                                     \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}

int main() {
  static_assert(sizeof(PtRayRadiance) == 16 && sizeof(ptq::F4) == 16, "a record is a texel");

  // ---- the passes of a batch: consecutive blocks, wrapping like the render calls' pass number ------------------------------------
  CHECK(ptr::batch_first_pass(0u, 0u, 1u) == 0u && ptr::batch_first_pass(5u, 0u, 7u) == 5u);
  CHECK(ptr::batch_first_pass(5u, 2u, 3u) == 11u);
  CHECK(ptr::batch_first_pass(0xfffffffeu, 1u, 4u) == 2u);
  CHECK(ptr::batch_first_pass(1u, 0xffffffffu, 0xffffffffu) == 2u);
  for (uint32_t b = 0; b < 5u; b++)  // the last pass of a batch is followed by the first of the next
    CHECK(ptr::batch_first_pass(9u, b, 3u) + 3u == ptr::batch_first_pass(9u, b + 1u, 3u));

  // ---- the zero record -----------------------------------------------------------------------------------------------------------
  {
    const PtRayRadiance z = ptr::zero_record();
    uint32_t u[4];
    std::memcpy(u, &z, 16);
    CHECK(u[0] == 0u && u[1] == 0u && u[2] == 0u && u[3] == 0u);
  }

  // ---- the fold over buffers of exactly n_passes * plane and 4 * plane texels and m records ---------------------------------------
  const float inf = std::numeric_limits<float>::infinity();
  const float hostile[] = {from_bits(0x7fc00000u), from_bits(0x7f800001u), inf, -inf};
  for (uint32_t plane : {1u, 63u, 64u, 65u, 777u})
    for (uint32_t n_passes : {1u, 2u, 5u})
      for (uint32_t m : {1u, plane / 2u + 1u, plane}) {
        if (m > plane) continue;
        std::vector<PtRay> rays(m);
        for (uint32_t i = 0; i < m; i++) {
          PtRay r;
          std::memset(&r, 0xff, sizeof r);  // (the pads are NaN)
          for (int c = 0; c < 3; c++) {
            r.origin[c] = (float)(i + (uint32_t)c);
            r.direction[c] = c == 2 ? -1.0f : 0.0f;
          }
          if (i % 3u == 1u) r.direction[i % 2u] = hostile[i % 4u];   // invalid: a hostile component
          if (i % 7u == 5u) r.direction[2] = -0.0f;                  // invalid: a direction of three zeros
          rays[i] = r;
        }
        std::vector<ptq::F4> planes(4u * (size_t)plane);
        const ptq::F4 mark = {-7.0f, -7.0f, -7.0f, -7.0f};
        for (auto& t : planes) t = mark;
        for (uint32_t i = 0; i < m; i++) ptq::pack_at(rays.data(), i, planes.data(), plane);
        // the slab: pass p's texel of place i is {i + p, 2 i, 0.5, 2}, stale NaNs where the ray is invalid
        std::vector<ptq::F4> slab((size_t)n_passes * plane);
        for (uint32_t p = 0; p < n_passes; p++)
          for (uint32_t i = 0; i < plane; i++) {
            const ptq::F4 t = {(float)(i + p), (float)(2u * i), 0.5f, 2.0f};
            const ptq::F4 stale = {hostile[0], inf, -inf, hostile[1]};
            const bool ok = i < m && ptq::ray_valid(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2], rays[i].direction[0],
                                                    rays[i].direction[1], rays[i].direction[2]);
            slab[(size_t)p * plane + i] = ok ? t : stale;
          }
        std::vector<PtRayRadiance> out(m);
        std::memset(out.data(), 0xa5, m * sizeof(PtRayRadiance));
        for (uint32_t i = 0; i < m; i++) ptr::fold_at(slab.data(), plane, n_passes, planes.data(), i, out.data());
        uint32_t n_invalid = 0;
        for (uint32_t i = 0; i < m; i++) {
          const bool ok = ptq::ray_valid(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2], rays[i].direction[0], rays[i].direction[1],
                                         rays[i].direction[2]);
          PtRayRadiance want = ptr::zero_record();
          if (ok)
            for (uint32_t p = 0; p < n_passes; p++) {
              want.sum[0] = want.sum[0] + (float)(i + p);
              want.sum[1] = want.sum[1] + (float)(2u * i);
              want.sum[2] = want.sum[2] + 0.5f;
              want.samples = want.samples + 2.0f;
            }
          else
            n_invalid++;
          CHECK(std::memcmp(&out[i], &want, 16) == 0);
        }
        CHECK(m < 6u || n_invalid > 0u);
      }

  // ---- the fold statement keeps the order of its adds: (big + small) + small, not big + (small + small) ---------------------------
  {
    PtRayRadiance r = ptr::zero_record();
    const ptq::F4 big = {16777216.0f, 0.0f, 0.0f, 1.0f}, one = {1.0f, 0.0f, 0.0f, 1.0f};
    ptr::fold_pass(r, big);
    ptr::fold_pass(r, one);
    ptr::fold_pass(r, one);
    CHECK(r.sum[0] == 16777216.0f && r.samples == 3.0f);
  }

  if (failures) {
    std::printf("radiance plan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("radiance plan: ok\n");
  return 0;
}
