// glare_main.cpp — a stand-alone program over csrc/pt_glare.hpp's host loop (ptglare::run) on EXACTLY sized heap arrays, for
// -fsanitize=address,undefined: an index past a level, a clamp that misses or a scratch buffer too small is a report, not a
// wrong bit.  tests/test_glare_ref.py builds it and runs it as a child; nothing sanitized is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../ray_tracer_webgl_amd/csrc/pt_glare.hpp"

using ptglare::F4;

static uint32_t g_state = 12345u;
static float rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

static int check(uint32_t w, uint32_t h, uint32_t levels, int from_accum, float threshold) {
  PtGlareOptions o = PT_GLARE_OPTIONS_DEFAULT;
  o.levels = levels;
  o.threshold = threshold;
  for (uint32_t k = 0; k < (uint32_t)PT_GLARE_MAX_LEVELS; k++) o.weight[k] = 1.0f / (float)levels;
  if (!ptglare::options_valid(o)) return 1;
  const size_t n = (size_t)w * h, np = ptglare::pyramid_texels(w, h, levels);
  std::unique_ptr<F4[]> src(new F4[n]), out(new F4[n]), scratch(new F4[np ? np : 1]);
  for (size_t i = 0; i < n; i++) {
    const float cnt = from_accum ? (float)(i % 4) : -1.0f;
    src[i] = F4{rnd() * 20.0f, rnd() * 2.0f, rnd(), cnt};
  }
  if (n > 2) {
    src[1].x = NAN;
    src[n - 1].y = INFINITY;
  }
  ptglare::run(src.get(), w, h, from_accum != 0, o, out.get(), scratch.get());
  for (size_t i = 0; i < n; i++) {
    if (out[i].w != 1.0f) return 2;
    const bool own = n > 2 && (i == 1 || i == n - 1);  // (a bad pixel may stay bad; no other pixel may turn bad)
    if (!own && !(std::isfinite(out[i].x) && std::isfinite(out[i].y) && std::isfinite(out[i].z))) return 3;
  }
  // in place over the source: the same bits
  std::unique_ptr<F4[]> again(new F4[n]);
  std::memcpy(again.get(), src.get(), n * sizeof(F4));
  ptglare::run(again.get(), w, h, from_accum != 0, o, again.get(), scratch.get());
  if (std::memcmp(again.get(), out.get(), n * sizeof(F4)) != 0) {
    for (size_t i = 0; i < n; i++)  // (NaN payloads aside)
      if (std::memcmp(&again[i], &out[i], sizeof(F4)) != 0 && !(std::isnan(again[i].x) || std::isnan(again[i].y) || std::isnan(again[i].z))) return 4;
  }
  return 0;
}

int main() {
  static const uint32_t sizes[6][2] = {{1, 1}, {1, 7}, {3, 5}, {17, 16}, {33, 130}, {64, 36}};
  static const uint32_t levels[4] = {1, 2, 5, 8};
  for (const auto& s : sizes)
    for (uint32_t l : levels)
      for (int from_accum = 0; from_accum < 2; from_accum++)
        for (float thr : {0.0f, 1.5f})
          if (int rc = check(s[0], s[1], l, from_accum, thr)) {
            std::printf("glare: %ux%u levels %u accum %d threshold %g: failure %d\n", s[0], s[1], l, from_accum, (double)thr, rc);
            return 1;
          }
  // a frame without pixels touches nothing
  PtGlareOptions o = PT_GLARE_OPTIONS_DEFAULT;
  ptglare::run(nullptr, 0, 5, false, o, nullptr, nullptr);
  ptglare::run(nullptr, 5, 0, false, o, nullptr, nullptr);
  std::printf("glare: ok\n");
  return 0;
}
