// nee_main.cpp — a stand-alone program over csrc/pt_nee.hpp for -fsanitize=address,undefined: the light table of exactly sized
// heap lists (a NaN centre, an infinite and a zero radius, a NaN albedo, a negative radius among them) and the sweep of
// tests/nee_sweep.hpp through choose / reach / sample / weight / add — a conversion out of range, an index past the table or a
// non-finite direction is a report, not a wrong bit.  tests/test_nee_ref.py builds it and runs it as a child; nothing sanitized
// is loaded into Python.
#include <cmath>
#include <cstdio>
#include <memory>

#include "../ray_tracer_webgl_amd/csrc/pt_kernel_args.h"
#include "../ray_tracer_webgl_amd/csrc/pt_nee.hpp"
#include "nee_sweep.hpp"

static int table_check() {
  // list lengths 0, 1 and 7; the lights are 1 (negative radius) and 5
  for (uint32_t n : {0u, 1u, 7u}) {
    std::unique_ptr<float[]> geom(new float[n ? 4 * n : 1]);
    std::unique_ptr<PtMatRec[]> mat(new PtMatRec[n ? n : 1]());
    for (uint32_t i = 0; i < n; i++) {
      const float r = i == 1 ? -0.5f : (i == 2 ? 0.0f : (i == 3 ? INFINITY : 0.25f + (float)i));
      geom[4 * i] = i == 4 ? NAN : (float)i; geom[4 * i + 1] = 1.0f; geom[4 * i + 2] = -(float)i;
      geom[4 * i + 3] = r * r;
      mat[i].type = i == 0 ? 0 : 3;
      mat[i].radius = r;
      mat[i].albedo[0] = 1.0f; mat[i].albedo[1] = i == 6 ? NAN : 2.0f; mat[i].albedo[2] = 3.0f;
    }
    const uint32_t L = ptnee::lights_of(geom.get(), mat.get(), n, (ptnee::Light*)nullptr);
    const uint32_t want = n == 7 ? 2u : 0u;
    if (L != want) return 1;
    std::unique_ptr<ptnee::Light[]> out(new ptnee::Light[L ? L : 1]);
    if (ptnee::lights_of(geom.get(), mat.get(), n, out.get()) != L) return 2;
    if (L == 2 && !(out[0].index == 1 && out[1].index == 5 && out[0].r2 == 0.25f && out[1].c[2] == -5.0f)) return 3;
  }
  return 0;
}

int main() {
  if (int rc = table_check()) { std::printf("nee: table failure %d\n", rc); return 1; }
  size_t held = 0, weightless = 0;
  for (const neesweep::Case& k : neesweep::cases()) {
    const int light = ptnee::choose(k.u0, k.L);
    if (light < 0 || light >= k.L) { std::printf("nee: light %d of %d\n", light, k.L); return 1; }
    float w[3], d2;
    if (!ptnee::reach(k.x, k.c, k.r2, w, d2)) continue;
    held++;
    const float ang = 6.2831855f * k.u2;
    float omega[3], om;
    ptnee::sample(w, d2, k.r2, k.u1, std::sin(ang), std::cos(ang), omega, om);
    const float cos_s = ptnee::cos_at(k.n, omega);
    const float wgt = ptnee::weight(k.L, om, cos_s);
    if (!(std::isfinite(omega[0]) && std::isfinite(omega[1]) && std::isfinite(omega[2]) && std::isfinite(wgt))) {
      std::printf("nee: a direction or weight that is not finite\n");
      return 1;
    }
    if (!(om >= 0.0f && om <= 1.0f)) { std::printf("nee: om %g\n", (double)om); return 1; }
    const float len2 = omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2];
    if (!(std::fabs(len2 - 1.0f) < 1e-4f)) { std::printf("nee: |omega|^2 = %g\n", (double)len2); return 1; }
    if (om == 0.0f) weightless++;
    float sum[3] = {0.5f, 0.25f, 0.125f};
    const float t[3] = {0.5f, 0.5f, 0.5f}, a[3] = {4.0f, 3.0f, 2.0f};
    ptnee::add(sum, t, a, wgt);
  }
  if (!held || !weightless) { std::printf("nee: the sweep misses an edge (%zu held, %zu weightless)\n", held, weightless); return 1; }
  std::printf("nee: ok\n");
  return 0;
}
