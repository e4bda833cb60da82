// nee_sweep.hpp — THE SWEEP of light-sample inputs that tests/test_nee_ref.py (through tests/nee_shim.cpp) and
// tests/nee_main.cpp (under the sanitizers) both walk: one list, stated once.  A case is a point x with a normal n, a light
// {c, r2} of a table of L, and the draw (u0, u1, u2).  The edges:
//   d2 == r2 and one ulp either side (P flips); r2 of a negative radius; a far light whose cosmax rounds to 1 (om = 0, weight 0);
//   a light one ulp inside its own reach (the LEAST cosmax there is: r2 < d2 makes r2 / d2 <= 1 - 2^-24, so cosmax never rounds
//   to 0 — its floor is sqrt(2^-24)); u at 0, at 1 - 2^-24 and at 1 (hash3 rounds 2^31 - 1 up to 2^31); w along +z and -z (the
//   frame's pole), along the axes and oblique; normals that give cos_s of either sign and exactly 0; L of 1, 2 and 65 with u0 at
//   every bin edge k / L and one ulp below it.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace neesweep {

struct Case {
  float x[3], n[3], c[3], r2;
  int L;
  float u0, u1, u2;
};

inline std::vector<Case> cases() {
  std::vector<Case> out;
  const float top = 1.0f - 0x1p-24f;
  const float us[5] = {0.0f, 0.25f, 0.6180339f, top, 1.0f};
  struct Geo { float x[3], c[3], r2; };
  std::vector<Geo> geos;
  auto geo = [&](float x0, float x1, float x2, float c0, float c1, float c2, float r2) { geos.push_back(Geo{{x0, x1, x2}, {c0, c1, c2}, r2}); };
  // d2 == 4 exactly: r2 at 4 and one ulp either side
  geo(0, 0, 0, 0, 0, 2, std::nextafterf(4.0f, 0.0f));
  geo(0, 0, 0, 0, 0, 2, 4.0f);
  geo(0, 0, 0, 0, 0, 2, std::nextafterf(4.0f, 8.0f));
  geo(0, 0, 0, 0, 0, -2, std::nextafterf(4.0f, 0.0f));  // ... and at the frame's pole, z = (0, 0, -1)
  geo(0, 0, 0, 0, 0, -3, (-1.5f) * (-1.5f));            // a negative radius: r * r
  geo(0, 0, 0, 0, 0, 3, 1.0f);
  geo(0, 0, 0, 3, 0, 0, 1.0f);
  geo(0, 0, 0, 0, -3, 0, 1.0f);
  geo(1.5f, -0.25f, 0.75f, -2.0f, 3.5f, 1.25f, 0.81f);   // oblique
  geo(0.1f, 0.2f, 0.3f, 0.1f, 0.2f, 1.0e5f, 1.0f);       // far: cosmax rounds to 1, weight 0
  geo(0, 0, 0, 1.0e-3f, 2.0e-3f, -1.0e-3f, 1.0e-9f);     // small scales
  geo(0, 0, 0, 1.0f, 1.0f, 1.0f, 2.9999998f);            // just inside the reach, oblique (d2 == 3)
  geo(0, 0, 0, 0.5f, 0.5f, 0.5f, 1.0f);                  // inside the light: !P
  const float ns[6][3] = {{0, 0, 1}, {0, 0, -1}, {1, 0, 0}, {0, 1, 0}, {0.6f, 0.0f, 0.8f}, {-0.57735f, -0.57735f, -0.57735f}};
  for (const Geo& g : geos)
    for (const auto& n : ns)
      for (float u1 : us)
        for (float u2 : us)
          out.push_back(Case{{g.x[0], g.x[1], g.x[2]}, {n[0], n[1], n[2]}, {g.c[0], g.c[1], g.c[2]}, g.r2, 2, 0.5f, u1, u2});
  // the bins of L = 1, 2, 65
  const int Ls[3] = {1, 2, 65};
  for (int L : Ls)
    for (int k = 0; k <= L; k++) {
      const float e = (float)k / (float)L;
      for (float u0 : {std::nextafterf(e, -1.0f), e, std::nextafterf(e, 2.0f)})
        if (u0 >= 0.0f && u0 <= 1.0f) out.push_back(Case{{0, 0, 0}, {0, 0, 1}, {0, 0.5f, 3}, 1.0f, L, u0, 0.3f, 0.7f});
    }
  // and a run of unremarkable ones (a fixed linear congruential sequence)
  uint32_t st = 0x2545F491u;
  auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(st >> 8) * (1.0f / 16777216.0f); };
  for (int i = 0; i < 400; i++) {
    Case k;
    for (int j = 0; j < 3; j++) { k.x[j] = 4.0f * rnd() - 2.0f; k.n[j] = 2.0f * rnd() - 1.0f; k.c[j] = 8.0f * rnd() - 4.0f; }
    const float len = std::sqrt(k.n[0] * k.n[0] + k.n[1] * k.n[1] + k.n[2] * k.n[2]) + 1e-6f;
    for (int j = 0; j < 3; j++) k.n[j] /= len;
    k.r2 = 0.01f + 2.0f * rnd();
    k.L = 1 + (int)(rnd() * 7.0f);
    k.u0 = rnd(); k.u1 = rnd(); k.u2 = rnd();
    out.push_back(k);
  }
  return out;
}

}  // namespace neesweep
