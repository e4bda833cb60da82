// query_main.cpp — a stand-alone program (its own main) that drives csrc/pt_query.hpp — batch splitting, covered tile rows, pack,
// unpack, the sentinel and the validity predicate — over EXACTLY sized heap buffers with every hostile operand class, built with
// -fsanitize=address,undefined by tests/test_query_plan.py and run as a child process: an index one past a plane, a shift or a
// conversion that is undefined, ends it.  No GPU, no preloaded library.  Prints "query plan: ok" when everything held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_query.hpp"

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
  static_assert(sizeof(PtRay) == 32 && sizeof(PtRayHit) == 64, "the records of include/ptrace.h");
  static_assert(sizeof(ptq::F4) == 16 && sizeof(ptq::I4) == 16, "texels");

  // ---- the predicate on every hostile class, in every component ------------------------------------------------------------
  const float inf = std::numeric_limits<float>::infinity();
  const float hostile[] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7f800001u) /* signalling */, inf, -inf};
  const float tame[] = {0.0f, -0.0f, 1.0f, -1.0f, from_bits(1u) /* the smallest denormal */, from_bits(0x80000001u),
                        std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), 1e-13f, 1e7f, 2e15f};
  for (float bad : hostile)
    for (int k = 0; k < 6; k++) {
      float v[6] = {0.0f, 0.1f, 0.2f, 0.3f, -0.4f, -1.0f};
      v[k] = bad;
      CHECK(!ptq::ray_valid(v[0], v[1], v[2], v[3], v[4], v[5]));
    }
  for (float a : tame)
    for (float b : tame) {
      const bool null_direction = a == 0.0f && b == 0.0f;
      CHECK(ptq::ray_valid(b, a, b, a, b, a) == !null_direction);  // (direction {a, b, a})
      CHECK(ptq::ray_valid(a, a, a, 0.0f, -0.0f, b) == (b != 0.0f));
    }
  CHECK(!ptq::ray_valid(1.0f, 2.0f, 3.0f, 0.0f, -0.0f, 0.0f));
  CHECK(!ptq::ray_valid(1.0f, 2.0f, 3.0f, -0.0f, -0.0f, -0.0f));

  // ---- batches and tile rows: every count is covered exactly once, no launch is empty, none exceeds the planes --------------
  const uint32_t shapes[][2] = {{37, 21}, {8, 8}, {9, 1}, {1, 1}, {1920, 1080}, {1, 4097}, {65535, 3}};
  for (const auto& sh : shapes) {
    const uint32_t w = sh[0], rows = sh[1], pix = w * rows;
    const uint32_t tiles_x = (w + 7u) / 8u, tiles_y = (rows + 7u) / 8u;
    const uint32_t counts[] = {1u, 63u, 64u, 65u, pix - 1u, pix, pix + 1u, 2u * pix + 5u, 0xffffffffu};
    for (uint32_t n : counts) {
      if (n == 0u) continue;
      const uint32_t nb = ptq::n_batches(n, pix);
      uint64_t total = 0;
      const uint32_t look[] = {0u, 1u, nb / 2u, nb - 1u};
      for (uint32_t k : look) {
        if (k >= nb) continue;
        const uint32_t m = ptq::batch_rays(n, pix, k);
        CHECK(m >= 1u && m <= pix);
        CHECK(k + 1u == nb || m == pix);
        const uint32_t tr = ptq::tile_rows_covered(m, w), tc = ptq::tiles_covered(m, w);
        CHECK(tr >= 1u && tr <= tiles_y && tc == tr * tiles_x);
        CHECK((uint64_t)tr * 8u * w >= m);                            // the rows of those tiles hold every ray
        CHECK(tr == 1u || (uint64_t)(tr - 1u) * 8u * w < m);          // ... and one tile row less would not
      }
      total = (uint64_t)(nb - 1u) * pix + ptq::batch_rays(n, pix, nb - 1u);
      CHECK(total == n);
    }
  }

  // ---- pack, the sentinel, unpack: over buffers of exactly 4 * plane texels, m == plane and m < plane -----------------------
  for (uint32_t plane : {1u, 63u, 64u, 65u, 777u}) {
    for (uint32_t m : {1u, plane / 2u + 1u, plane}) {
      if (m > plane) continue;
      std::vector<PtRay> rays(m);
      for (uint32_t i = 0; i < m; i++) {
        PtRay r;
        for (int c = 0; c < 3; c++) {
          r.origin[c] = (float)(i * 8u + (uint32_t)c);
          r.direction[c] = hostile[(i + (uint32_t)c) % 5u];
        }
        r._pad0 = hostile[0];
        r._pad1 = inf;
        rays[i] = r;
      }
      std::vector<ptq::F4> planes(4u * (size_t)plane);
      const ptq::F4 mark = {-7.0f, -7.0f, -7.0f, -7.0f};
      for (auto& t : planes) t = mark;
      for (uint32_t i = 0; i < m; i++) ptq::pack_at(rays.data(), i, planes.data(), plane);
      for (uint32_t i = 0; i < plane; i++) {
        const ptq::F4 o = planes[2u * (size_t)plane + i], d = planes[(size_t)plane + i];
        if (i < m) {
          CHECK(std::memcmp(&o, rays[i].origin, 12) == 0 && std::memcmp(&d, rays[i].direction, 12) == 0);
          CHECK(ptq::bits_of(o.w) == 0u && ptq::bits_of(d.w) == 0u);  // the pads are not carried
        } else {
          CHECK(std::memcmp(&o, &mark, 16) == 0 && std::memcmp(&d, &mark, 16) == 0);
        }
        CHECK(std::memcmp(&planes[i], &mark, 16) == 0 && std::memcmp(&planes[3u * (size_t)plane + i], &mark, 16) == 0);
      }
      // every ray here is invalid: the sentinel at its texels, then the records
      for (uint32_t i = 0; i < m; i++) {
        const ptq::F4 o = planes[2u * (size_t)plane + i], d = planes[(size_t)plane + i];
        CHECK(!ptq::ray_valid(o.x, o.y, o.z, d.x, d.y, d.z));
        ptq::invalid_texels(&planes[i], &planes[(size_t)plane + i], &planes[2u * (size_t)plane + i],
                            reinterpret_cast<ptq::I4*>(planes.data() + 3u * (size_t)plane) + i);
      }
      std::vector<PtRayHit> hits(m);
      for (uint32_t i = 0; i < m; i++) ptq::unpack_at(planes.data(), plane, i, hits.data());
      for (uint32_t i = 0; i < m; i++) {
        uint32_t u[16];
        std::memcpy(u, &hits[i], 64);
        for (int k = 0; k < 16; k++) CHECK(u[k] == (k >= 12 && k < 15 ? 0xfffffffeu : 0u));
      }
      // a record with every field different comes out field for field
      const ptq::F4 a = {1.0f, 2.0f, 3.0f, 4.0f}, nn = {5.0f, 6.0f, 7.0f, 0.0f}, pp = {8.0f, 9.0f, 10.0f, 0.0f};
      const ptq::I4 ids = {11, -12, 13, 1};
      const PtRayHit h = ptq::unpack_hit(a, nn, pp, ids);
      CHECK(h.albedo[0] == 1.0f && h.albedo[2] == 3.0f && h.t == 4.0f && h.normal[1] == 6.0f && h.point[2] == 10.0f);
      CHECK(h.index == 11 && h.uuid == -12 && h.type == 13 && h.front_face == 1 && h._pad0 == 0.0f && h._pad1 == 0.0f);
    }
  }

  if (failures) {
    std::printf("query plan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("query plan: ok\n");
  return 0;
}
