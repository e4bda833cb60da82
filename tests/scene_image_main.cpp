// scene_image_main.cpp — a stand-alone program over csrc/pt_scene_image.hpp for a sanitizer build (tests/test_scene_image.py
// compiles it with -fsanitize=address,undefined and runs it): split at the list lengths around the padding's steps, per_slot
// with indices past the source, and build_grid on lists of those lengths, on a field that fits the LDS and on one that does
// not (the Morton-run layout), every array read to its end.  Exit status 0: everything agreed.
#include "../ray_tracer_webgl_amd/csrc/pt_scene_image.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static uint32_t lcg_state = 12345u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) * (1.0f / 16777216.0f); }

static std::vector<PtSphere> field(uint32_t n, float extent) {
  std::vector<PtSphere> s(n);
  for (uint32_t i = 0; i < n; i++) {
    std::memset(&s[i], 0, sizeof s[i]);
    s[i].center[0] = (unit() - 0.5f) * extent; s[i].center[1] = unit() * 0.2f * extent; s[i].center[2] = (unit() - 0.5f) * extent;
    s[i].radius = 0.1f + 0.4f * unit();
    s[i].type = (int32_t)(i % 4u);
    s[i].refraction_index = i % 3u ? 1.5f : 0.0f;
    s[i].uuid = (int32_t)(1000u + 3u * i);
  }
  return s;
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void check_split(const std::vector<PtSphere>& s) {
  const uint32_t n = (uint32_t)s.size();
  const ptscene::Split sp = ptscene::split(s.data(), n);
  CHECK(sp.geom.size() == (size_t)PT_LDS_ENTRIES(n) * 4 && sp.mat.size() == n && sp.radii.size() == n && sp.r0.size() == 2 * (size_t)n &&
        sp.uuid.size() == n && sp.regular);
  for (uint32_t i = 0; i < n; i++)
    CHECK(bits(sp.geom[4 * i + 3]) == bits(s[i].radius * s[i].radius) && sp.uuid[i] == s[i].uuid && bits(sp.mat[i].inv_ri) == bits(1.0f / s[i].refraction_index));
  for (size_t i = n; i < sp.geom.size() / 4; i++)
    CHECK(sp.geom[4 * i] == 1e15f && sp.geom[4 * i + 1] == 1e15f && sp.geom[4 * i + 2] == 1e15f && bits(sp.geom[4 * i + 3]) == 0u);
  // per_slot: every sphere once, backwards, between slots that name no sphere
  std::vector<uint32_t> index;
  index.push_back(0xffffffffu);
  for (uint32_t i = n; i-- > 0;) index.push_back(i);
  index.push_back(n);
  const std::vector<PtMatRec> m = ptscene::per_slot(index.data(), index.size(), sp.mat.data(), sp.mat.size());
  const std::vector<int32_t> u = ptscene::per_slot(index.data(), index.size(), sp.uuid.data(), sp.uuid.size());
  const PtMatRec zero{};
  CHECK(m.size() == index.size() && u.size() == index.size());
  CHECK(std::memcmp(&m.front(), &zero, sizeof zero) == 0 && std::memcmp(&m.back(), &zero, sizeof zero) == 0 && u.front() == 0 && u.back() == 0);
  for (uint32_t k = 0; k < n; k++) CHECK(std::memcmp(&m[1 + k], &sp.mat[n - 1 - k], sizeof zero) == 0 && u[1 + k] == sp.uuid[n - 1 - k]);
}

// build_grid, and everything its arrays point at
static void check_grid(const std::vector<PtSphere>& s, double factor, bool want_grid, bool want_fit) {
  const uint32_t n = (uint32_t)s.size();
  const ptscene::Split sp = ptscene::split(s.data(), n);
  ptgrid::Grid g;
  const bool ok = ptscene::build_grid(sp.geom.data(), sp.radii.data(), n, factor, &g);
  CHECK(ok == want_grid);
  if (!ok) return;
  const bool fit = PT_GRID_LDS_CELLS(ptscene::staged_cells(g)) + (size_t)g.n_entries * 16 <= walk_lds_room();
  CHECK(fit == want_fit);
  CHECK(g.cells.size() == (size_t)g.n[0] * g.n[1] * g.n[2] && g.entries.size() == (size_t)g.n_entries * 4 && g.entry_index.size() == g.n_entries);
  CHECK(ptrec::fits(g.n_entries));
  for (uint32_t rec : g.cells) CHECK((rec & 0xffffffu) + (rec >> 24) <= g.n_entries);
  const std::vector<PtMatRec> m = ptscene::per_slot(g.entry_index.data(), g.entry_index.size(), sp.mat.data(), sp.mat.size());
  for (size_t k = 0; k < m.size(); k++) {
    const uint32_t i = g.entry_index[k];
    CHECK(i < n || i == 0xffffffffu);
    if (i < n) CHECK(bits(g.entries[4 * k + 3]) == bits(sp.geom[4 * i + 3]) && bits(m[k].radius) == bits(sp.radii[i]));
  }
}

int main() {
  const uint32_t sizes[7] = {0u, 1u, 7u, 8u, 9u, 16u, 17u};
  for (uint32_t n : sizes) {
    const std::vector<PtSphere> s = field(n, 6.0f);
    check_split(s);
    check_grid(s, 3.0, n >= 16u, true);
  }
  {
    std::vector<PtSphere> s = field(9u, 6.0f);
    s[4].center[1] = 1e15f;
    CHECK(!ptscene::split(s.data(), 9u).regular);
  }
  check_grid(field(400u, 20.0f), 3.0, true, true);
  check_grid(field(12000u, 100.0f), 3.0, true, false);
  check_grid(field(12000u, 100.0f), 2.5, true, false);
  std::printf("scene image: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
