// error_plan_main.cpp — a stand-alone program over csrc/pt_error_plan.hpp and csrc/pt_tile_order.hpp for a sanitizer build
// (tests/test_error_plan.py compiles it with -fsanitize=address,undefined and runs it), through the entries of the two shims:
// at every shape of the Python test the records, tallies and flags live in exactly-sized heap arrays, so a read or write
// past a tile count is seen; then a long walk of tile-order events.  Exit status 0: everything agreed.
#include "error_plan_shim.cpp"
#include "tile_order_shim.cpp"

#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static void shape(uint32_t width, uint32_t rows) {
  const uint32_t tx = (width + 7) / 8, ty = (rows + 7) / 8, n = tx * ty;
  uint64_t pixels = 0;
  for (uint32_t t = 0; t < n; t++) {
    const uint32_t px = error_plan_tile_pixels(width, rows, tx, t);
    CHECK(px >= 1 && px <= 64);
    pixels += px;
  }
  CHECK(pixels == (uint64_t)width * rows);
  CHECK(error_plan_tile_pixels(width, rows, tx, n) == 0u);  // (a tile below the image)
  // records of ordinary tiles: every pixel counted, n = 8; then one tile short, one empty, one saturated
  std::vector<float> h(8 * (size_t)n);
  uint32_t seed = width * 977u + rows;
  for (uint32_t t = 0; t < n; t++) {
    const float px = (float)error_plan_tile_pixels(width, rows, tx, t);
    float* r = &h[4 * (size_t)t];
    float* a = &h[4 * ((size_t)n + t)];
    r[0] = (float)(lcg(&seed) % 1000u) * 1e-3f * px; r[1] = 3.0f * px; r[2] = px; r[3] = 8.0f;
    a[0] = 0.0f; a[1] = 0.0f; a[2] = 8.0f; a[3] = 0.0f;
  }
  for (int variant = 0; variant < 4; variant++) {
    std::vector<float> g(h);
    float* r = &g[0];
    float* a = &g[4 * (size_t)n];
    if (variant == 1) { a[0] = r[2]; r[0] = r[1] = r[2] = r[3] = 0.0f; a[2] = 0.0f; }         // tile 0: every pixel short
    if (variant == 2) { a[1] = r[2]; r[0] = r[1] = r[2] = r[3] = 0.0f; a[2] = 0.0f; }         // tile 0: nothing counted, nothing short
    if (variant == 3) { r[3] = 4294967296.0f; a[2] = 8589934592.0f; }                          // tile 0: n beyond 32 bits
    PtErrorStats st;
    error_plan_stats(g.data(), n, pixels, &st);
    uint64_t counted = 0;
    for (uint32_t t = 0; t < n; t++) counted += (uint64_t)g[4 * (size_t)t + 2];
    CHECK(st.pixels == pixels && st.pixels_counted == counted);
    CHECK(st.pixels_short == (variant == 1 ? (uint64_t)a[0] : 0u) && st.pixels_nonfinite == (variant == 2 ? (uint64_t)a[1] : 0u));
    CHECK(st.passes_max == (variant == 3 ? 0xffffffffu : (counted ? 8u : 0u)));
    CHECK(st.passes_min == (variant == 3 && n == 1u ? 0xffffffffu : (counted ? 8u : 0u)));
    CHECK(error_plan_reached(&st, 1e30f) == (st.pixels_short == 0 ? 1 : 0) && error_plan_reached(&st, 1e-30f) == (st.sum_e2 == 0.0 && st.pixels_short == 0 ? 1 : 0));
    std::vector<uint32_t> flags(n, 7u);
    const uint32_t loose = error_plan_select(&st, 1e30f, g.data(), n, flags.data());
    CHECK(loose == (variant == 1 ? 1u : 0u) && flags[0] == (variant == 1 ? 1u : 0u));
    const uint32_t tight = error_plan_select(&st, 1e-30f, g.data(), n, flags.data());
    uint32_t set = 0;
    for (uint32_t f : flags) { CHECK(f <= 1u); set += f; }
    CHECK(set == tight && tight <= n);
    if (variant == 2) CHECK(flags[0] == 0u);
  }
  PtErrorStats st;
  error_plan_stats(nullptr, 0, 0, &st);  // no tiles: nothing is read
  CHECK(st.rel_error == 0.0 && st.rms_error == 0.0 && st.passes_min == 0u && st.passes_max == 0u);
}

int main() {
  const uint32_t shapes[5][2] = {{64, 36}, {61, 37}, {9, 9}, {8, 8}, {1, 1}};
  for (const auto& s : shapes) shape(s[0], s[1]);
  // tile order: a walk of events of every kind, with every view
  const int n_events = 5000;
  std::vector<int> events(5 * (size_t)n_events);
  std::vector<uint32_t> out(7 * (size_t)n_events, 0xdeadbeefu);
  uint32_t seed = 12345u;
  for (int i = 0; i < n_events; i++) {
    int* e = &events[5 * (size_t)i];
    e[0] = (int)(lcg(&seed) % 5u);
    e[1] = e[0] == EV_FRAMES ? (int)(1u + lcg(&seed) % 8u) : (int)(lcg(&seed) % 2u);
    e[2] = e[0] == EV_FRAMES ? (int)(lcg(&seed) % 9u) : (int)(lcg(&seed) % 2u);
    e[3] = (int)(1u + lcg(&seed) % 100u);
    e[4] = (int)(lcg(&seed) % 2u);
  }
  CHECK(tile_order_run(events.data(), n_events, out.data()) == 0);
  for (int i = 0; i < n_events; i++) {
    const uint32_t* o = &out[7 * (size_t)i];
    for (int k = 0; k < 6; k++) CHECK(o[k] <= 1u);
    if (o[1]) CHECK(o[0] == 1u);                    // costs are zeroed only for the order kernel that follows
    if (o[0] && events[5 * (size_t)i] != EV_UNIFORM) CHECK(o[3] == 1u && o[4] == 0u);
    if (o[2]) CHECK(o[5] == 1u && o[6] == 0u);
  }
  std::printf("error plan: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
